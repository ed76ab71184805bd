// ProNet tower (pocket / struct_graph modality; ref struct_graph_encoder.py:5-42 plugs in dig.threedgraph.method.ProNet): the radius graph, its
// by-source twin, the per-edge geometric features, the fused edge-weighted convolution in both directions, and the fp32 row ops of the node side.
// Everything is fp32 FMAs: the tower trains from scratch at h = 128 and its contractions over the feature width (<= 48) are too short for an MFMA tile.
//
// Layout (oneprot_amd/pronet.py): edges are stored by TARGET in a fixed-width table nbr int32 [N, 32] (sources ascending, -1 behind deg[i]); edge
// (i, e) is "slot" s = i * 32 + e, and every per-edge array is indexed by the slot.  The backward needs the same edges by SOURCE: src_off int32
// [N + 1] and src_list int32 [32 N] of slots, targets ascending -- so that da[j] is one ordered sum and no float atomic is needed.
// w_e = W2 W1 f_e is never written: the convolution kernels hold row c of the folded operand (WfT [F, h], column c) in registers, one thread per
// channel, and form w_e[c] from the edge's feature row in LDS.
#include "philox.h"
#include "../../include/oneprot_hip.h"

#define PN_SLOTS ONEPROT_PRONET_SLOTS

// ---- graph ------------------------------------------------------------------------------------------------------------------------------------------
// One thread per target: scan the target's own graph in index order and keep the first `cap` sources in range, which is the rule of torch_cluster's
// GPU radius() (the lowest indices survive the cap).  d^2 <= r^2 in fp32, no FMA contraction, so that the host restatement can repeat it.
__global__ void __launch_bounds__(128) k_pronet_radius_graph(const float* __restrict__ ca, const int* __restrict__ ptr, const int* __restrict__ batch,
                                                             int* __restrict__ nbr, int* __restrict__ deg, int N, float r2, int cap) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= N) return;
  const int g = batch[i], j0 = ptr[g], j1 = ptr[g + 1];
  const float x = ca[3 * i], y = ca[3 * i + 1], z = ca[3 * i + 2];
  int n = 0;
  for (int j = j0; j < j1 && n < cap; ++j) {
    if (j == i) continue;
    const float dx = ca[3 * j] - x, dy = ca[3 * j + 1] - y, dz = ca[3 * j + 2] - z;
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    if (d2 <= r2) nbr[(size_t)i * PN_SLOTS + n++] = j;
  }
  deg[i] = n;
  for (int e = n; e < PN_SLOTS; ++e) nbr[(size_t)i * PN_SLOTS + e] = -1;
}

// slot of source j in target i's (ascending) row, or -1
__device__ __forceinline__ int pn_find(const int* __restrict__ row, int n, int j) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row[mid] < j) lo = mid + 1; else hi = mid;
  }
  return (lo < n && row[lo] == j) ? lo : -1;
}
// One thread per source: walk the source's graph in target order.  fill == 0 counts (cnt[j]), fill == 1 writes the slots behind src_off[j].
__global__ void __launch_bounds__(128) k_pronet_by_source(const int* __restrict__ ptr, const int* __restrict__ batch, const int* __restrict__ nbr,
                                                          const int* __restrict__ deg, int* __restrict__ cnt, const int* __restrict__ src_off,
                                                          int* __restrict__ src_list, int N, int fill) {
  const int j = blockIdx.x * 128 + threadIdx.x;
  if (j >= N) return;
  const int g = batch[j], i0 = ptr[g], i1 = ptr[g + 1];
  int n = 0;
  const int base = fill ? src_off[j] : 0;
  for (int i = i0; i < i1; ++i) {
    if (i == j) continue;
    const int e = pn_find(nbr + (size_t)i * PN_SLOTS, deg[i], j);
    if (e >= 0) {
      if (fill) src_list[base + n] = i * PN_SLOTS + e;
      ++n;
    }
  }
  if (!fill) cnt[j] = n;
}
// exclusive scan of cnt[0 .. N) into off[0 .. N] by one work-group: a contiguous chunk per thread, then a scan of the 1024 chunk sums
__global__ void __launch_bounds__(1024) k_pronet_scan(const int* __restrict__ cnt, int* __restrict__ off, int N) {
  __shared__ int s[1024];
  const int t = threadIdx.x, per = (N + 1023) / 1024, a = t * per, b = min(N, a + per);
  int sum = 0;
  for (int k = a; k < b; ++k) sum += cnt[k];
  s[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? s[t - o] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  int run = s[t] - sum;
  for (int k = a; k < b; ++k) { off[k] = run; run += cnt[k]; }
  if (t == 1023) off[N] = s[1023];
}

extern "C" int oneprot_radius_graph(const float* ca, const int* graph_ptr, const int* batch, int* nbr, int* deg, int N, int n_graphs, float cutoff,
                                    int max_num_neighbors, void* stream) {
  if (!ca || !graph_ptr || !batch || !nbr || !deg || N <= 0 || n_graphs <= 0 || N > (1 << 26) || !(cutoff > 0.f) || max_num_neighbors < 1 ||
      max_num_neighbors > PN_SLOTS) return OP_EINVAL;
  hipLaunchKernelGGL(k_pronet_radius_graph, dim3((N + 127) / 128), dim3(128), 0, (hipStream_t)stream, ca, graph_ptr, batch, nbr, deg, N, cutoff * cutoff,
                     max_num_neighbors);
  return launch_status();
}
extern "C" int oneprot_graph_by_source(const int* graph_ptr, const int* batch, const int* nbr, const int* deg, int* count_ws, int* src_off, int* src_list,
                                       int N, int n_graphs, void* stream) {
  if (!graph_ptr || !batch || !nbr || !deg || !count_ws || !src_off || !src_list || N <= 0 || n_graphs <= 0 || N > (1 << 26)) return OP_EINVAL;
  const dim3 grid((N + 127) / 128);
  hipLaunchKernelGGL(k_pronet_by_source, grid, dim3(128), 0, (hipStream_t)stream, graph_ptr, batch, nbr, deg, count_ws, (const int*)nullptr, (int*)nullptr, N, 0);
  hipLaunchKernelGGL(k_pronet_scan, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const int*)count_ws, src_off, N);
  hipLaunchKernelGGL(k_pronet_by_source, grid, dim3(128), 0, (hipStream_t)stream, graph_ptr, batch, nbr, deg, (int*)nullptr, (const int*)src_off, src_list, N, 1);
  return launch_status();
}

// ---- edge features ----------------------------------------------------------------------------------------------------------------------------------
struct pn_v3 { float x, y, z; };
__device__ __forceinline__ pn_v3 pn_ld(const float* __restrict__ p, int i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ pn_v3 pn_sub(pn_v3 a, pn_v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ pn_v3 pn_cross(pn_v3 a, pn_v3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float pn_dot(pn_v3 a, pn_v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float pn_norm(pn_v3 a) { return sqrtf(pn_dot(a, a)); }
__device__ __forceinline__ float pn_j0(float x) { return x < 1e-3f ? 1.f - x * x * (1.f / 6.f) : sinf(x) / x; }
__device__ __forceinline__ float pn_j1(float x) {
  if (x < 0.25f) { const float x2 = x * x; return x * (1.f / 3.f) * (1.f - x2 * 0.1f * (1.f - x2 * (1.f / 28.f))); }     // the closed form cancels there
  float s, c;
  sincosf(x, &s, &c);
  return (s / x - c) / x;
}
// two standard normals from two Philox words (Box-Muller on 23-bit uniforms (k + 1/2) 2^-23, which fp32 holds exactly)
__device__ __forceinline__ void pn_box_muller(unsigned w0, unsigned w1, float& n0, float& n1) {
  const float u1 = ((float)(w0 >> 9) + 0.5f) * (1.f / 8388608.f), u2 = ((float)(w1 >> 9) + 0.5f) * (1.f / 8388608.f);
  const float r = sqrtf(-2.f * logf(u1));
  float s, c;
  sincosf(6.283185307179586f * u2, &s, &c);
  n0 = r * c; n1 = r * s;
}
__device__ __forceinline__ float pn_clip(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// consts: [0, 2 nr) the Bessel zeros z_{l,n} (l major), [2 nr, 4 nr) the normalisers sqrt(2) / |j_{l+1}(z_{l,n})|, [4 nr, 4 nr + np / 2) the frequencies f_k
__global__ void __launch_bounds__(256) k_pronet_edge_features(const float* __restrict__ ca, const float* __restrict__ cn, const float* __restrict__ cc,
                                                              const int* __restrict__ nbr, const int* __restrict__ deg, const float* __restrict__ consts,
                                                              float* __restrict__ f0, float* __restrict__ f1, float* __restrict__ f2, int N, int nr, int np,
                                                              float inv_cutoff, int noise, float sigma, float clip, unsigned long long seed,
                                                              unsigned long long stream_id) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= (long long)N * PN_SLOTS) return;
  const int i = (int)(s / PN_SLOTS), e = (int)(s % PN_SLOTS);
  const int F0 = 4 * nr, F1 = 6 * nr, F2 = np;
  float* o0 = f0 + s * F0; float* o1 = f1 + s * F1; float* o2 = f2 + s * F2;
  if (e >= deg[i]) {
    for (int k = 0; k < F0; ++k) o0[k] = 0.f;
    for (int k = 0; k < F1; ++k) o1[k] = 0.f;
    for (int k = 0; k < F2; ++k) o2[k] = 0.f;
    return;
  }
  const int j = nbr[s];
  const int r0 = i == 0 ? N - 1 : i - 1, r1 = i == N - 1 ? 0 : i + 1;
  const pn_v3 pi = pn_ld(ca, i), pj = pn_ld(ca, j);
  const pn_v3 v = pn_sub(pj, pi), u0 = pn_sub(pn_ld(ca, r0), pi), u1 = pn_sub(pn_ld(ca, r1), pi);
  const float dist = pn_norm(v);
  const float theta = atan2f(pn_norm(pn_cross(v, u0)), pn_dot(v, u0));
  const pn_v3 p1 = pn_cross(u0, u1), p2 = pn_cross(u0, v);
  const float phi = atan2f(pn_dot(pn_cross(p1, p2), u0) / pn_norm(u0), pn_dot(p1, p2));
  // Euler angles between the backbone frames of i and j
  const pn_v3 x1 = pn_sub(pn_ld(cn, i), pi), x2 = pn_sub(pn_ld(cn, j), pj);
  const pn_v3 z1 = pn_cross(x1, pn_cross(x1, pn_sub(pn_ld(cc, i), pi))), z2 = pn_cross(x2, pn_cross(x2, pn_sub(pn_ld(cc, j), pj)));
  const float l1 = pn_norm(z1) + 1e-7f, l2 = pn_norm(z2) + 1e-7f;
  const pn_v3 nn = pn_cross(z1, z2);
  float ang[3];
  ang[0] = atan2f(pn_dot(pn_cross(x1, nn), z1) / l1, pn_dot(x1, nn));
  ang[1] = atan2f(pn_norm(nn), pn_dot(z1, z2));
  ang[2] = atan2f(pn_dot(pn_cross(nn, x2), z2) / l2, pn_dot(nn, x2));
  if (noise) {
    unsigned w[4];
    philox_block((uint64_t)s, seed, stream_id, w);
    float n[4];
    pn_box_muller(w[0], w[1], n[0], n[1]);
    pn_box_muller(w[2], w[3], n[2], n[3]);
#pragma unroll
    for (int k = 0; k < 3; ++k) ang[k] += pn_clip(sigma * n[k], clip);
  }
  const float d = dist * inv_cutoff;
  float st, ct, sp, cp;
  sincosf(theta, &st, &ct);
  sincosf(phi, &sp, &cp);
  const float Y[4] = {0.28209479f, 0.48860251f * ct, 0.48860251f * st * cp, 0.48860251f * st * sp};
  const float ca3[3] = {cosf(ang[0]), cosf(ang[1]), cosf(ang[2])};
  for (int n = 0; n < nr; ++n) {
    const float rb0 = consts[2 * nr + n] * pn_j0(consts[n] * d), rb1 = consts[3 * nr + n] * pn_j1(consts[nr + n] * d);
    // feature0[a, b, n] = Y[2 a + b] * rbf[b, n]: the published pairing
    o0[n] = Y[0] * rb0; o0[nr + n] = Y[1] * rb1; o0[2 * nr + n] = Y[2] * rb0; o0[3 * nr + n] = Y[3] * rb1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o1[k * 2 * nr + n] = 0.28209479f * rb0; o1[k * 2 * nr + nr + n] = 0.48860251f * ca3[k] * rb1; }
  }
  const float delta = (float)(j - i);
  for (int k = 0; k < np / 2; ++k) {
    float sn, cs;
    sincosf(delta * consts[4 * nr + k], &sn, &cs);
    o2[k] = cs; o2[np / 2 + k] = sn;
  }
}
extern "C" int oneprot_pronet_edge_features(const float* ca, const float* cn, const float* cc, const int* nbr, const int* deg, const float* consts, float* f0,
                                            float* f1, float* f2, int N, int num_radial, int num_pos_emb, float cutoff, int noise, float sigma, float clip,
                                            uint64_t seed, uint64_t stream_id, void* stream) {
  if (!ca || !cn || !cc || !nbr || !deg || !consts || !f0 || !f1 || !f2 || N <= 0 || N > (1 << 26) || num_radial < 1 || num_radial > 8 || num_pos_emb < 2 ||
      (num_pos_emb & 1) || num_pos_emb > 48 || !(cutoff > 0.f)) return OP_EINVAL;
  const long long slots = (long long)N * PN_SLOTS;
  hipLaunchKernelGGL(k_pronet_edge_features, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ca, cn, cc, nbr, deg, consts, f0, f1, f2, N,
                     num_radial, num_pos_emb, 1.f / cutoff, noise, sigma, clip, (unsigned long long)seed, (unsigned long long)stream_id);
  return launch_status();
}

// ---- the fused convolution -----------------------------------------------------------------------------------------------------------------------------
// out[t, c] = sum over the edges k of row t of (sum_f WfT[f, c] feat[slot_k, f]) * v[node_k, c]; one thread per channel c, blockDim.x = h.
//   by_source 0 (forward, m = sum_e w_e * a_j):   row t = target i, slot_k = i * 32 + k, node_k = nbr[slot_k]
//   by_source 1 (backward, da = sum_e dm_i * w_e): row t = source j, slot_k = src_list[src_off[j] + k], node_k = slot_k / 32
// The sum runs in list order (sources / targets ascending) in one fmaf chain per (t, c): two runs give the same bits.
template <int FMAX>
__global__ void __launch_bounds__(256) k_pronet_edge_conv(const float* __restrict__ feat, const float* __restrict__ WfT, const float* __restrict__ v,
                                                          const int* __restrict__ nbr, const int* __restrict__ deg, const int* __restrict__ src_off,
                                                          const int* __restrict__ src_list, float* __restrict__ out, int N, int h, int F, int by_source) {
  __shared__ float sf[PN_SLOTS][FMAX];
  __shared__ int snode[PN_SLOTS];
  const int c = threadIdx.x;
  float w[FMAX];
#pragma unroll
  for (int f = 0; f < FMAX; ++f) w[f] = f < F ? WfT[(size_t)f * h + c] : 0.f;
  for (int t = blockIdx.x; t < N; t += gridDim.x) {
    const int first = by_source ? src_off[t] : 0;
    const int n = by_source ? src_off[t + 1] - first : deg[t];
    float acc = 0.f;
    for (int base = 0; base < n; base += PN_SLOTS) {
      const int cnt = min(PN_SLOTS, n - base);
      __syncthreads();
      for (int idx = c; idx < cnt * FMAX; idx += h) {
        const int e = idx / FMAX, f = idx - e * FMAX;
        const size_t slot = by_source ? (size_t)src_list[first + base + e] : (size_t)t * PN_SLOTS + base + e;
        sf[e][f] = f < F ? feat[slot * F + f] : 0.f;
      }
      if (c < cnt) snode[c] = by_source ? src_list[first + base + c] / PN_SLOTS : nbr[(size_t)t * PN_SLOTS + base + c];
      __syncthreads();
      for (int e = 0; e < cnt; ++e) {
        const float vv = v[(size_t)snode[e] * h + c];
        float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
#pragma unroll
        for (int f = 0; f < FMAX; f += 4) {
          w0 = fmaf(w[f], sf[e][f], w0); w1 = fmaf(w[f + 1], sf[e][f + 1], w1); w2 = fmaf(w[f + 2], sf[e][f + 2], w2); w3 = fmaf(w[f + 3], sf[e][f + 3], w3);
        }
        acc = fmaf((w0 + w1) + (w2 + w3), vv, acc);
      }
    }
    out[(size_t)t * h + c] = acc;
  }
}
// dWfT[f, c] = sum_e dm[i, c] a[j, c] feat[slot, f]: work-group b owns the targets [b * per, (b + 1) * per) and writes part[b, f, c]
template <int FMAX>
__global__ void __launch_bounds__(256) k_pronet_edge_conv_bwd_w(const float* __restrict__ feat, const float* __restrict__ a, const float* __restrict__ dm,
                                                                const int* __restrict__ nbr, const int* __restrict__ deg, float* __restrict__ part, int N,
                                                                int h, int F, int per) {
  __shared__ float sf[PN_SLOTS][FMAX];
  __shared__ int snode[PN_SLOTS];
  const int c = threadIdx.x;
  float acc[FMAX];
#pragma unroll
  for (int f = 0; f < FMAX; ++f) acc[f] = 0.f;
  const int t0 = blockIdx.x * per, t1 = min(N, t0 + per);
  for (int t = t0; t < t1; ++t) {
    const int cnt = deg[t];
    __syncthreads();
    for (int idx = c; idx < cnt * FMAX; idx += h) {
      const int e = idx / FMAX, f = idx - e * FMAX;
      sf[e][f] = f < F ? feat[((size_t)t * PN_SLOTS + e) * F + f] : 0.f;
    }
    if (c < cnt) snode[c] = nbr[(size_t)t * PN_SLOTS + c];
    __syncthreads();
    const float d = dm[(size_t)t * h + c];
    for (int e = 0; e < cnt; ++e) {
      const float g = d * a[(size_t)snode[e] * h + c];
#pragma unroll
      for (int f = 0; f < FMAX; ++f) acc[f] = fmaf(g, sf[e][f], acc[f]);
    }
  }
#pragma unroll
  for (int f = 0; f < FMAX; ++f)
    if (f < F) part[((size_t)blockIdx.x * F + f) * h + c] = acc[f];
}
__global__ void __launch_bounds__(256) k_pronet_part_sum(const float* __restrict__ part, float* __restrict__ out, int nb, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += part[(size_t)b * n + k];
  out[k] = s;
}

static inline bool pn_conv_shape_ok(int N, int h, int F) { return N > 0 && N <= (1 << 26) && h >= 64 && h <= 256 && (h & 63) == 0 && F >= 1 && F <= 48; }
#define PN_CONV_DISPATCH(LAUNCH) do { if (F <= 16) { LAUNCH(16); } else if (F <= 24) { LAUNCH(24); } else if (F <= 36) { LAUNCH(36); } else { LAUNCH(48); } } while (0)

static int pn_conv(const float* feat, const float* WfT, const float* v, const int* nbr, const int* deg, const int* src_off, const int* src_list, float* out, int N,
                   int h, int F, int by_source, void* stream) {
  const int blocks = N < 4096 ? N : 4096;
#define L(FM) hipLaunchKernelGGL((k_pronet_edge_conv<FM>), dim3(blocks), dim3(h), 0, (hipStream_t)stream, feat, WfT, v, nbr, deg, src_off, src_list, out, N, h, F, by_source)
  PN_CONV_DISPATCH(L);
#undef L
  return launch_status();
}
extern "C" int oneprot_edge_conv_fwd(const float* feat, const float* WfT, const float* a, const int* nbr, const int* deg, float* m, int N, int h, int F, void* stream) {
  if (!feat || !WfT || !a || !nbr || !deg || !m || !pn_conv_shape_ok(N, h, F)) return OP_EINVAL;
  return pn_conv(feat, WfT, a, nbr, deg, nullptr, nullptr, m, N, h, F, 0, stream);
}
extern "C" int oneprot_edge_conv_bwd_x(const float* feat, const float* WfT, const float* dm, const int* src_off, const int* src_list, float* da, int N, int h, int F,
                                       void* stream) {
  if (!feat || !WfT || !dm || !src_off || !src_list || !da || !pn_conv_shape_ok(N, h, F)) return OP_EINVAL;
  return pn_conv(feat, WfT, dm, nullptr, nullptr, src_off, src_list, da, N, h, F, 1, stream);
}
static inline int pn_bwd_w_blocks(int N) { const int b = (N + 15) / 16; return b < 512 ? b : 512; }
extern "C" size_t oneprot_edge_conv_bwd_w_workspace(int N, int h, int F) {
  if (!pn_conv_shape_ok(N, h, F)) return 0;
  return (size_t)pn_bwd_w_blocks(N) * F * h * sizeof(float);
}
extern "C" int oneprot_edge_conv_bwd_w(const float* feat, const float* a, const float* dm, const int* nbr, const int* deg, float* dWfT, void* workspace,
                                       size_t workspace_bytes, int N, int h, int F, void* stream) {
  if (!feat || !a || !dm || !nbr || !deg || !dWfT || !workspace || !pn_conv_shape_ok(N, h, F) || workspace_bytes < oneprot_edge_conv_bwd_w_workspace(N, h, F) ||
      ((uintptr_t)workspace & 3)) return OP_EINVAL;
  const int nb = pn_bwd_w_blocks(N), per = (N + nb - 1) / nb;
  float* part = (float*)workspace;
#define L(FM) hipLaunchKernelGGL((k_pronet_edge_conv_bwd_w<FM>), dim3(nb), dim3(h), 0, (hipStream_t)stream, feat, a, dm, nbr, deg, part, N, h, F, per)
  PN_CONV_DISPATCH(L);
#undef L
  hipLaunchKernelGGL(k_pronet_part_sum, dim3((F * h + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)part, dWfT, nb, F * h);
  return launch_status();
}

// ---- node-side row ops ------------------------------------------------------------------------------------------------------------------------------------
// x0[i, c] = W[c, z_i] + sum_k W[c, 26 + k] bb[i, k] + b[c] (W fp32 [h, 32] = Linear(26 + 6 -> h).weight); feat_out (optional) [N, 32] = [one_hot(z_i, 26), bb_i],
// the operand of the weight-gradient GEMM.  An id outside 0..25 contributes no column (the host type refuses it).
__global__ void __launch_bounds__(256) k_pronet_embed_fwd(const int64_t* __restrict__ z, const float* __restrict__ bb, const float* __restrict__ W,
                                                          const float* __restrict__ b, float* __restrict__ x0, float* __restrict__ feat_out, int N, int h) {
  const int i = blockIdx.x, zi = (int)z[i];
  const bool ok = zi >= 0 && zi < 26;
  float bv[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) bv[k] = bb[(size_t)i * 6 + k];
  for (int c = threadIdx.x; c < h; c += blockDim.x) {
    float acc = b[c] + (ok ? W[(size_t)c * 32 + zi] : 0.f);
#pragma unroll
    for (int k = 0; k < 6; ++k) acc = fmaf(W[(size_t)c * 32 + 26 + k], bv[k], acc);
    x0[(size_t)i * h + c] = acc;
  }
  if (feat_out && threadIdx.x < 32) {
    const int k = threadIdx.x;
    feat_out[(size_t)i * 32 + k] = k < 26 ? ((ok && k == zi) ? 1.f : 0.f) : bv[k - 26];
  }
}
extern "C" int oneprot_pronet_embed_fwd(const int64_t* z, const float* bb, const float* W, const float* b, float* x0, float* feat_out, int N, int h, void* stream) {
  if (!z || !bb || !W || !b || !x0 || N <= 0 || h <= 0) return OP_EINVAL;
  hipLaunchKernelGGL(k_pronet_embed_fwd, dim3(N), dim3(h < 256 ? (h + 63) / 64 * 64 : 256), 0, (hipStream_t)stream, z, bb, W, b, x0, feat_out, N, h);
  return launch_status();
}

__device__ __forceinline__ float pn_act(float z, int act) {
  if (act == 1) return z / (1.f + __expf(-z));
  if (act == 2) return fmaxf(z, 0.f);
  return z;
}
__device__ __forceinline__ float pn_act_grad(float z, int act) {
  if (act == 1) { const float s = 1.f / (1.f + __expf(-z)); return s + z * s * (1.f - s); }
  if (act == 2) return z > 0.f ? 1.f : 0.f;
  return 1.f;
}
// z[r, c] += bias[c] in place (the pre-activation the backward needs); y[r * ldy + c] = act(z[r, c]) (+ resid[r, c])
__global__ void __launch_bounds__(256) k_pronet_bias_act(float* __restrict__ z, const float* __restrict__ bias, const float* __restrict__ resid, float* __restrict__ y,
                                                         long long total, int n, int ldy, int act) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= total) return;
  const long long r = k / n;
  const int c = (int)(k - r * n);
  float v = z[k];
  if (bias) { v += bias[c]; z[k] = v; }
  if (y) {
    float o = pn_act(v, act);
    if (resid) o += resid[k];
    y[r * ldy + c] = o;
  }
}
// dz[r, c] = dy[r * ldy + c] * act'(z[r, c])
__global__ void __launch_bounds__(256) k_pronet_act_bwd(const float* __restrict__ dy, const float* __restrict__ z, float* __restrict__ dz, long long total, int n, int ldy,
                                                        int act) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= total) return;
  const long long r = k / n;
  const int c = (int)(k - r * n);
  dz[k] = dy[r * ldy + c] * pn_act_grad(z[k], act);
}
extern "C" int oneprot_pronet_bias_act(float* z, const float* bias, const float* resid, float* y, int64_t M, int n, int ldy, int act, void* stream) {
  if (!z || M <= 0 || n <= 0 || act < 0 || act > 2 || (y && ldy < n) || (!y && !bias)) return OP_EINVAL;
  const long long total = (long long)M * n;
  hipLaunchKernelGGL(k_pronet_bias_act, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, bias, resid, y, total, n, ldy, act);
  return launch_status();
}
extern "C" int oneprot_pronet_act_bwd(const float* dy, const float* z, float* dz, int64_t M, int n, int ldy, int act, void* stream) {
  if (!dy || !z || !dz || M <= 0 || n <= 0 || act < 0 || act > 2 || ldy < n) return OP_EINVAL;
  const long long total = (long long)M * n;
  hipLaunchKernelGGL(k_pronet_act_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, z, dz, total, n, ldy, act);
  return launch_status();
}

// y[e] = x[e] + clip(sigma * normal(e), +-clip): four elements per Philox block (counter = e / 4), Box-Muller on its word pairs
__global__ void __launch_bounds__(256) k_pronet_noise_add(const float* __restrict__ x, float* __restrict__ y, long long n4, float sigma, float clip,
                                                          unsigned long long seed, unsigned long long stream_id) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= n4) return;
  unsigned w[4];
  philox_block((uint64_t)q, seed, stream_id, w);
  float n[4];
  pn_box_muller(w[0], w[1], n[0], n[1]);
  pn_box_muller(w[2], w[3], n[2], n[3]);
  const float4 v = reinterpret_cast<const float4*>(x)[q];
  reinterpret_cast<float4*>(y)[q] = make_float4(v.x + pn_clip(sigma * n[0], clip), v.y + pn_clip(sigma * n[1], clip), v.z + pn_clip(sigma * n[2], clip),
                                                v.w + pn_clip(sigma * n[3], clip));
}
extern "C" int oneprot_clipped_normal_add_f32(const float* x, float* y, int64_t n, float sigma, float clip, uint64_t seed, uint64_t stream_id, void* stream) {
  if (!x || !y || n <= 0 || (n & 3) || (((uintptr_t)x | (uintptr_t)y) & 15) || !(sigma >= 0.f) || !(clip >= 0.f)) return OP_EINVAL;
  const long long n4 = n / 4;
  hipLaunchKernelGGL(k_pronet_noise_add, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, n4, sigma, clip, (unsigned long long)seed,
                     (unsigned long long)stream_id);
  return launch_status();
}

// y[g, c] = sum of x[i, c] over i in [ptr[g], ptr[g + 1]) in index order; backward dx[i, c] = dy[batch[i], c]
__global__ void __launch_bounds__(256) k_pronet_segment_sum(const float* __restrict__ x, const int* __restrict__ ptr, float* __restrict__ y, int d) {
  const int g = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= d) return;
  float s = 0.f;
  for (int i = ptr[g]; i < ptr[g + 1]; ++i) s += x[(size_t)i * d + c];
  y[(size_t)g * d + c] = s;
}
__global__ void __launch_bounds__(256) k_pronet_segment_bcast(const float* __restrict__ dy, const int* __restrict__ batch, float* __restrict__ dx, long long total, int d) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= total) return;
  const long long i = k / d;
  dx[k] = dy[(size_t)batch[i] * d + (k - i * d)];
}
extern "C" int oneprot_segment_sum_f32(const float* x, const int* graph_ptr, float* y, int n_graphs, int d, void* stream) {
  if (!x || !graph_ptr || !y || n_graphs <= 0 || d <= 0) return OP_EINVAL;
  hipLaunchKernelGGL(k_pronet_segment_sum, dim3(n_graphs, (d + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, graph_ptr, y, d);
  return launch_status();
}
extern "C" int oneprot_segment_sum_bwd_f32(const float* dy, const int* batch, float* dx, int N, int d, void* stream) {
  if (!dy || !batch || !dx || N <= 0 || d <= 0) return OP_EINVAL;
  const long long total = (long long)N * d;
  hipLaunchKernelGGL(k_pronet_segment_bcast, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, batch, dx, total, d);
  return launch_status();
}

// Column sums of an fp32 [M, n] matrix (the bias gradients of the node linears: M = every node of the batch).  Blocked summation in a fixed order:
// a work-group owns 64 columns x 256 rows, a thread eight interleaved 8-row pieces combined as a tree, then the four row lanes, then the row
// chunks (again eight accumulators and a tree) -- no serial chain is longer than 8, so equal rows (the readout's backward broadcasts one row per
// graph) do not pile their rounding up as one long chain does.
__device__ __forceinline__ float pn_tree8(const float (&a)[8]) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }
__global__ void __launch_bounds__(256) k_pronet_colsum(const float* __restrict__ x, float* __restrict__ part, int M, int n) {
  __shared__ float s[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = blockIdx.x * 64 + tx;
  const int r0 = blockIdx.y * 256, r1 = min(M, r0 + 256);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < n) {
    int k = 0;
    for (int r = r0 + ty; r < r1; r += 4, ++k) a[k & 7] += x[(size_t)r * n + c];
  }
  s[ty][tx] = pn_tree8(a);
  __syncthreads();
  if (ty == 0 && c < n) part[(size_t)blockIdx.y * n + c] = (s[0][tx] + s[1][tx]) + (s[2][tx] + s[3][tx]);
}
__global__ void __launch_bounds__(256) k_pronet_colsum_final(const float* __restrict__ part, float* __restrict__ out, int nb, int n) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < nb; ++b) a[b & 7] += part[(size_t)b * n + c];
  out[c] = pn_tree8(a);
}
extern "C" size_t oneprot_colsum_f32_workspace(int64_t M, int n) {
  if (M <= 0 || n <= 0 || M > ((int64_t)1 << 30)) return 0;
  return (size_t)((M + 255) / 256) * n * sizeof(float);
}
extern "C" int oneprot_colsum_f32(const float* x, float* out, void* workspace, size_t workspace_bytes, int64_t M, int n, void* stream) {
  const size_t need = oneprot_colsum_f32_workspace(M, n);
  if (!x || !out || !workspace || !need || workspace_bytes < need || ((uintptr_t)workspace & 3) || (M + 255) / 256 > 65535) return OP_EINVAL;
  const int nb = (int)((M + 255) / 256);
  hipLaunchKernelGGL(k_pronet_colsum, dim3((n + 63) / 64, nb), dim3(256), 0, (hipStream_t)stream, x, (float*)workspace, (int)M, n);
  hipLaunchKernelGGL(k_pronet_colsum_final, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, out, nb, n);
  return launch_status();
}

// ---- weight gradients of the node linears ---------------------------------------------------------------------------------------------------------------
// dW[n, k] = sum_r dz[r, n] x[r, k] (autograd's `dz.t() @ x`), the contraction running over M = every node of the batch.  oneprot_sgemm makes that ONE
// fmaf chain of M terms per element in (n / 64) (k / 64) work-groups: at M = 8193 its rounding is 6 to 36 times that of a blocked fp32 sum, and four
// work-groups walk 8193 rows each.  Here a work-group owns a 64 x 64 tile of dW and `per` rows (128, or M / 256 for more than 32 768 rows), four
// outputs a side per thread as in sgemm.hip, and writes slab part[b]; the slabs are summed by k_pronet_colsum_final (eight accumulators and a tree).
// Rows behind the slab are staged as zeros: fmaf(0, 0, acc) is exact.  A fixed order throughout: two runs give the same bits.
#define PN_WG_BK 32
__global__ void __launch_bounds__(256) k_pronet_wgrad(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ part, int M, int n, int k,
                                                      int per) {
  __shared__ float sA[PN_WG_BK][64 + 4];
  __shared__ float sB[PN_WG_BK][64 + 4];
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int r0 = blockIdx.z * per, r1 = min(M, r0 + per);
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int rb = r0; rb < r1; rb += PN_WG_BK) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < PN_WG_BK * 64 / 256; ++it) {
      const int idx = tid + it * 256, kk = idx >> 6, cc = idx & 63, r = rb + kk;
      sA[kk][cc] = (r < r1 && m0 + cc < n) ? dz[(size_t)r * n + m0 + cc] : 0.f;
      sB[kk][cc] = (r < r1 && n0 + cc < k) ? x[(size_t)r * k + n0 + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < PN_WG_BK; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = sA[kk][ty * 4 + i]; b[i] = sB[kk][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gm = m0 + ty * 4 + i;
    if (gm >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gn = n0 + tx * 4 + j;
      if (gn < k) part[((size_t)blockIdx.z * n + gm) * k + gn] = acc[i][j];
    }
  }
}
static inline bool pn_wgrad_shape_ok(int64_t M, int n, int k) { return M > 0 && M <= ((int64_t)1 << 26) && n > 0 && n <= 4096 && k > 0 && k <= 4096; }
static inline int pn_wgrad_rows(int64_t M) { const int q = (int)(((M + 255) / 256 + 63) / 64 * 64); return q > 128 ? q : 128; }
extern "C" size_t oneprot_wgrad_f32_workspace(int64_t M, int n, int k) {
  if (!pn_wgrad_shape_ok(M, n, k)) return 0;
  const int per = pn_wgrad_rows(M);
  return (size_t)((M + per - 1) / per) * n * k * sizeof(float);
}
extern "C" int oneprot_wgrad_f32(const float* dz, const float* x, float* dW, void* workspace, size_t workspace_bytes, int64_t M, int n, int k, void* stream) {
  const size_t need = oneprot_wgrad_f32_workspace(M, n, k);
  if (!dz || !x || !dW || !workspace || !need || workspace_bytes < need || ((uintptr_t)workspace & 3)) return OP_EINVAL;
  const int per = pn_wgrad_rows(M), nb = (int)((M + per - 1) / per);
  hipLaunchKernelGGL(k_pronet_wgrad, dim3((k + 63) / 64, (n + 63) / 64, nb), dim3(256), 0, (hipStream_t)stream, dz, x, (float*)workspace, (int)M, n, k, per);
  hipLaunchKernelGGL(k_pronet_colsum_final, dim3((n * k + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dW, nb, n * k);
  return launch_status();
}
