// MSA Transformer tower (esm_msa1b_t12_100M_UR50S architecture; ref msa_encoder.py:36 calls it through fair-esm: MSATransformer.forward,
// AxialTransformerLayer, RowSelfAttention, ColumnSelfAttention, LearnedPositionalEmbedding).  Forward only, eval mode: the reference freezes the tower.
// The dense layers and LayerNorms are the library's NT GEMM / LayerNorm entry points; this file holds what they cannot express:
//   oneprot_msa_embed_fwd    token + learned position (per-row scan over the non-pad tokens) + MSA-row embedding, LayerNorm, padded positions zeroed
//   oneprot_msa_row_scores   tied row attention: one L x L score map per (MSA, head), contracted over (row r, channel c) -- K extent R * 64
//   oneprot_msa_row_context  softmax over the keys of that map (row-0 key mask), then P . V_r for every row r (P and V^T through a workspace)
//   oneprot_msa_col_attn     column attention: for each (MSA, column, head) attention over the R rows, rows a whole MSA row apart in memory
//
// LAYOUTS.  Tokens are numbered t = (b * R + r) * L + l.  qkv is the bf16 [T, 3 * H * 64] output of ONE oneprot_gemm_bf16_nt (ONEPROT_EPI_BF16 + bias) on the
// stacked q / k / v weights: row t holds q (columns h * 64 + c), then k (H * 64 + h * 64 + c), then v (2 * H * 64 + h * 64 + c); no re-layout pass.
// key_bias is oneprot_key_padding_bias of the tokens: fp32 [T], 0 = token, anything else = padding.  S is fp32 [B, H, L, L].  ctx is bf16 [T, H * 64],
// the A operand of the out-projection GEMM.  hd = 64 only.
//
// MFMA: v_mfma_f32_16x16x32_bf16; lane l holds A[row l & 15][k = 8 (l >> 4) + e] and B[k = 8 (l >> 4) + e][col l & 15], e = 0..7: for q and k that is one
// 16-byte load straight from the 128-byte head row.  V is summed over its row index, so it is transposed first ([channel][key]): in LDS for the column
// attention, into the workspace for the row attention.
// Every reduction runs in a fixed order inside one work-group (no split along K chosen by the grid, no atomics): an MSA's result does not depend on
// what else is in the batch.  Masked keys are excluded (probability 0) instead of biased by -10000: the two differ only where every key of a query is
// masked, i.e. at padded positions, which then hold 0 -- finite, as the next layer's tied scores need.
//
// TRAIN-MODE DROPOUT (oneprot_msa_row_context_dropout, oneprot_msa_col_attn_dropout): fair-esm applies nn.Dropout(attention_dropout) to the probabilities
// of both attentions between the softmax and the product with V; the reference runs the frozen tower that way in every training step (Lightning's
// module.train() undoes msa_encoder.py:30).  The DROP = true instantiations of k_msa_row_softmax and k_msa_col_attn apply the per-element hash mask of
// attn_drop.h to the normalised probability in fp32, before its one rounding to bf16; maximum and sum are those of the undropped softmax.
//   row    one mask element per (b, h, i, j), shared by the R rows (the attention is tied):  attn_keep(q = i, k = j, bh = (b_first + b) * H + h),
//          b_first = the MSA's place in the batch when the host hands over a group of whole MSAs: the grouping cannot change a bit
//   column one per (b, h, l, i, j):  attn_keep(q = i, k = j, bh = (b * H + h) * L + l)   (< 2^26: B * H <= 65535, L <= 1024)
// The DROP = false instantiations are the kernels as they were.
//
// RAGGED BATCHES (the oneprot_msa_*_ragged entry points): a stream of MSAs, each a dense R_b x L_b block at its own depth and length (host type
// oneprot_amd.packing.PackedMsa).  One kernel body behind two geometry decoders, as AttnSlab (attention.hip) and row_seg (rowops.hip) do it:
//   MsaUniform  today's index arithmetic: MSA b of a [B, R, L] batch
//   MsaRagged   row g of a device table int64 [n, 8] = {tok0, R_b, L_b, s0, p0, vt0, b, 0}: the block's first token in the stream, its shape, where its
//               S [H, L_b, L_b] (fp32 elements of S), P [H, L_b, Lp_b] and Vt [H, R_b, 64, Lp_b] (bf16 elements of the workspace) start, and the MSA's
//               index for the dropout stream.  The host orders the table longest MSA first, so that no long MSA starts last.
// The ragged launches use the grid of the largest MSA of the call; a work-group outside its own MSA's extent leaves as a whole before the first barrier
// (an empty work-group costs a dispatch, no memory traffic: against a work list it saves the list and one dependent load per work-group).
// Dropping an MSA's trailing all-pad rows and columns cannot change a bit of what remains: a dropped row has q = 0 and is an excluded key, a dropped
// column is a masked key, and both only ever added exact zeros to the fixed-order sums.
#include "common.h"
#include "attn_drop.h"
#include "../../include/oneprot_hip.h"
#include <float.h>

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// ---------------------------------------------------------------------------------------------------------------- geometry decoders
struct MsaGeo { size_t tok0; int R, L, Lp, b; size_t s0, p0, vt0; };
struct MsaUniform {
  int R, L, Lp, H;
  __device__ __forceinline__ MsaGeo at(int b) const {
    return {(size_t)b * R * L, R, L, Lp, b, (size_t)b * H * L * L, (size_t)b * H * L * Lp, (size_t)b * H * R * 64 * Lp};
  }
};
struct MsaRagged {
  const long long* tab;
  __device__ __forceinline__ MsaGeo at(int g) const {
    const long long* e = tab + (size_t)g * 8;
    const int L = (int)e[2];
    return {(size_t)e[0], (int)e[1], L, (L + 31) & ~31, (int)e[6], (size_t)e[3], (size_t)e[4], (size_t)e[5]};
  }
};

__device__ __forceinline__ bf8_t msa_frag(const bf16_t* p) { return __builtin_bit_cast(bf8_t, *reinterpret_cast<const u32x4*>(p)); }
__device__ __forceinline__ bf8_t msa_zero_frag() { return __builtin_bit_cast(bf8_t, u32x4{0u, 0u, 0u, 0u}); }
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// reductions over the 16 lanes that share lane >> 4 (the columns of one accumulator row)
__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- embedding
// One wave per token.  position = (number of non-pad tokens of the row up to and including this one) + pad_id, pad_id for padding
// (fair-esm LearnedPositionalEmbedding / make_positions); d <= 2048.
// VAR (ragged stream): T = T_pad; token t belongs to the MSA b with cu[b] <= t < cu[b + 1] (binary search, n <= 65535), whose rows are rlen[b] long; its row
// index and its position count run inside that block.  Rows from cu[n] on are the tail: written as 0.
#define EMB_MAXV 32
template <bool VAR>
__global__ void __launch_bounds__(256) k_msa_embed(const long long* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ posw,
                                                   const float* __restrict__ roww, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   float* __restrict__ x, long long T, int R, int L, int d, int vocab, int n_pos, int pad_id, float eps,
                                                   const int* __restrict__ cu = nullptr, const int* __restrict__ rlen = nullptr, int n = 0, int n_rows = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long t = (long long)blockIdx.x * 4 + wave;
  if (t >= T) return;                                    // whole wave; the kernel has no barrier
  int l, r;
  if constexpr (!VAR) {
    const long long row = t / L;
    l = (int)(t - row * L);
    r = (int)(row % R);
  } else {
    int lo = 0, hi = n;                                  // the last b with cu[b] <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (cu[mid] <= t) lo = mid; else hi = mid;
    }
    const int Lb = rlen[lo], off = (int)(t - cu[lo]);
    if (t >= cu[n] || Lb <= 0 || off < 0) {              // tail rows (and a malformed table): zeros
      for (int c = lane; c < d; c += 64) x[(size_t)t * d + c] = 0.f;
      return;
    }
    r = min(off / Lb, n_rows - 1);
    l = off % Lb;
  }
  const long long* rid = ids + (t - l);
  int cnt = 0;
  for (int j = lane; j <= l; j += 64) cnt += rid[j] != pad_id ? 1 : 0;
  cnt = wave_sum_int(cnt);
  long long id = rid[l];
  const bool padded = id == pad_id;
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  int pos = padded ? pad_id : cnt + pad_id;
  pos = pos < 0 ? 0 : (pos >= n_pos ? n_pos - 1 : pos);
  const float* pt = tok + (size_t)id * d;
  const float* pp = posw + (size_t)pos * d;
  const float* pr = roww + (size_t)r * d;
  float v[EMB_MAXV];
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < EMB_MAXV; ++e) {
    const int c = lane + 64 * e;
    v[e] = c < d ? pt[c] + pp[c] + pr[c] : 0.f;
    s += v[e];
  }
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < EMB_MAXV; ++e) {
    const int c = lane + 64 * e;
    const float dv = c < d ? v[e] - mean : 0.f;
    q += dv * dv;
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)d + eps);
  float* px = x + (size_t)t * d;
#pragma unroll
  for (int e = 0; e < EMB_MAXV; ++e) {
    const int c = lane + 64 * e;
    if (c < d) px[c] = padded ? 0.f : (v[e] - mean) * rstd * gamma[c] + beta[c];
  }
}

// ---------------------------------------------------------------------------------------------------------------- tied row scores
// grid (L/128, L/128, B * H) rounded up; four waves, each a 64 x 64 quadrant of the 128 x 128 tile (16 accumulator tiles per wave: eight 16-byte fragment
// loads feed sixteen MFMAs per k-step); rows r in ascending order, two k-steps of 32 channels each.
template <class G>
__global__ void __launch_bounds__(256) k_msa_row_scores(const bf16_t* __restrict__ qkv, const float* __restrict__ kb, float* __restrict__ S, const G geo, int H,
                                                        float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave & 1, wc = wave >> 1;
  const int bh = blockIdx.z, b = bh / H, h = bh - b * H;
  const MsaGeo mg = geo.at(b);
  const int R = mg.R, L = mg.L;
  const int i0 = blockIdx.y * 128 + wr * 64, j0 = blockIdx.x * 128 + wc * 64;
  if (i0 >= L || j0 >= L) return;                        // whole wave; the kernel has no barrier
  const int ld = 3 * H * 64, fr = lane & 15, kq = (lane >> 4) * 8;
  int ia[4], ja[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    ia[t] = min(i0 + t * 16 + fr, L - 1);                // rows past L read row L - 1 (in bounds) and are not stored
    ja[t] = min(j0 + t * 16 + fr, L - 1);
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t tok0 = mg.tok0;
  for (int r = 0; r < R; ++r) {
    const size_t row = tok0 + (size_t)r * L;
    bool padq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) padq[t] = kb[row + ia[t]] != 0.f;      // q of a padded position counts as zero
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf8_t fa[4], fb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        fa[t] = msa_frag(qkv + (row + ia[t]) * ld + h * 64 + ks * 32 + kq);
        if (padq[t]) fa[t] = msa_zero_frag();
        fb[t] = msa_frag(qkv + (row + ja[t]) * ld + (H + h) * 64 + ks * 32 + kq);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = MFMA16(fa[a], fb[c], acc[a][c]);
    }
  }
  float* Sb = S + mg.s0 + (size_t)h * L * L;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = i0 + a * 16 + (lane >> 4) * 4 + reg, j = j0 + c * 16 + fr;
        if (i < L && j < L) Sb[(size_t)i * L + j] = acc[a][c][reg] * scale;
      }
}

// ---------------------------------------------------------------------------------------------------------------- tied row context
// Three launches through a caller-provided workspace (oneprot_msa_row_context_workspace): Lp = L rounded up to 32,
//   P  bf16 [B, H, L, Lp]       the probabilities, one wave per row: softmax over the keys row 0 holds, zeros at masked keys and past L
//   Vt bf16 [B, H, R, 64, Lp]   V transposed (channel x key, zeros past L): the product sums over V's row index, so its fragments must run along the keys
// and then ctx^T = Vt . P^T as a plain tile product with both fragments loaded straight from global memory (16 bytes per lane).
#define RC_MAXL ONEPROT_MSA_MAX_LEN
template <bool DROP, class G>
__global__ void __launch_bounds__(256) k_msa_row_softmax(const float* __restrict__ S, const float* __restrict__ kb, bf16_t* __restrict__ P, const G geo, int H,
                                                         int b_first, const AttnDrop dr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave, bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const MsaGeo mg = geo.at(b);
  const int L = mg.L, Lp = mg.Lp;
  if (i >= L) return;                                    // whole wave; the kernel has no barrier
  const size_t tok0 = mg.tok0;                           // row 0 of the MSA: the key mask (fair-esm RowSelfAttention: padding_mask[:, 0])
  const float* Si = S + mg.s0 + ((size_t)h * L + i) * L;
  float v[RC_MAXL / 64];
  float m = -FLT_MAX;
#pragma unroll
  for (int t = 0; t < RC_MAXL / 64; ++t) {
    const int j = lane + 64 * t;
    const bool ok = j < L && kb[tok0 + min(j, L - 1)] == 0.f;
    v[t] = ok ? Si[min(j, L - 1)] : -FLT_MAX;
    m = fmaxf(m, v[t]);
  }
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < RC_MAXL / 64; ++t) {
    v[t] = v[t] == -FLT_MAX ? 0.f : __expf(v[t] - m);
    sum += v[t];
  }
  sum = wave_sum(sum);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;         // every key masked (row 0 all padding): probabilities 0, context 0 (finite)
  bf16_t* Pi = P + mg.p0 + ((size_t)h * L + i) * Lp;
#pragma unroll
  for (int t = 0; t < RC_MAXL / 64; ++t) {
    const int j = lane + 64 * t;
    if (DROP) {                                            // fair-esm RowSelfAttention: dropout_module(attn_probs); one mask for all R rows
      const bool keep = attn_keep((unsigned)i, (unsigned)j, (unsigned)((b_first + mg.b) * H + h), dr);
      if (j < Lp) Pi[j] = keep ? f2bf(v[t] * inv * dr.scale) : (bf16_t)0;
    } else {
      if (j < Lp) Pi[j] = f2bf(v[t] * inv);
    }
  }
}

// grid (Lp / 32, R, B * H): a 32-key x 64-channel tile of V through LDS
#define VT_S 40                    // bf16 per LDS row [channel][32 keys]: 80 bytes, 16-byte aligned
template <class G>
__global__ void __launch_bounds__(256) k_msa_v_transpose(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ Vt, const G geo, int H) {
  __shared__ __attribute__((aligned(16))) bf16_t sT[64 * VT_S];
  const int tid = threadIdx.x, kc = blockIdx.x * 32, r = blockIdx.y, bh = blockIdx.z, b = bh / H, h = bh - b * H;
  const MsaGeo mg = geo.at(b);
  const int R = mg.R, L = mg.L, Lp = mg.Lp;
  if (kc >= Lp || r >= R) return;                        // whole work-group (ragged: a tile past this MSA's own extent), before the barrier
  const int key = tid >> 3, cg = (tid & 7) * 8, j = kc + key;
  u32x4 w = *reinterpret_cast<const u32x4*>(qkv + (mg.tok0 + (size_t)r * L + min(j, L - 1)) * (size_t)(3 * H * 64) + (2 * H + h) * 64 + cg);
  if (j >= L) w = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sT[(cg + 2 * e) * VT_S + key] = (bf16_t)(w[e] & 0xffffu);
    sT[(cg + 2 * e + 1) * VT_S + key] = (bf16_t)(w[e] >> 16);
  }
  __syncthreads();
  const int c = tid >> 2, part = (tid & 3) * 8;
  *reinterpret_cast<u32x4*>(Vt + mg.vt0 + (((size_t)h * R + r) * 64 + c) * Lp + kc + part) = *reinterpret_cast<const u32x4*>(sT + c * VT_S + part);
}

// grid (L / 64 rounded up, R / 4 rounded up, B * H): wave w forms the 64 queries x 64 channels of row r = 4 blockIdx.y + w, transposed (channel x query) so
// that a lane ends up with four consecutive channels of one query: one 8-byte store.  Keys in ascending order.
template <class G>
__global__ void __launch_bounds__(256) k_msa_row_pv(const bf16_t* __restrict__ P, const bf16_t* __restrict__ Vt, bf16_t* __restrict__ ctx, const G geo, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, g = lane >> 4, kq = g * 8;
  const int bh = blockIdx.z, b = bh / H, h = bh - b * H, r = blockIdx.y * 4 + wave, i0 = blockIdx.x * 64;
  const MsaGeo mg = geo.at(b);
  const int R = mg.R, L = mg.L, Lp = mg.Lp;
  if (r >= R || i0 >= L) return;                         // whole wave; the kernel has no barrier
  const bf16_t* pP[4];
  const bf16_t* pV[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    pP[t] = P + mg.p0 + ((size_t)h * L + min(i0 + t * 16 + fr, L - 1)) * Lp + kq;      // queries past L read row L - 1 and are not stored
    pV[t] = Vt + mg.vt0 + (((size_t)h * R + r) * 64 + t * 16 + fr) * Lp + kq;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < Lp; kc += 32) {
    bf8_t fp[4], fv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      fp[t] = msa_frag(pP[t] + kc);
      fv[t] = msa_frag(pV[t] + kc);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = MFMA16(fv[nt], fp[mt], acc[nt][mt]);
  }
  const size_t row = mg.tok0 + (size_t)r * L;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int i = i0 + mt * 16 + fr;
    if (i < L) {
      bf16_t* po = ctx + (row + i) * (size_t)(H * 64) + h * 64 + g * 4;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) *reinterpret_cast<u32x2*>(po + nt * 16) = u32x2{pack2bf(acc[nt][mt][0], acc[nt][mt][1]), pack2bf(acc[nt][mt][2], acc[nt][mt][3])};
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- column attention
// grid (H, L, B): one work-group per (MSA, column, head); its R query rows in tiles of 16, wave w takes tiles w, w + 4.  V (R x 64, zeros up to a multiple
// of 32 rows) sits transposed in LDS for all four waves; a wave's probabilities go through its own LDS rows to become the B operand of ctx^T = V^T . P^T.
#define CA_MAXR 128
#define CA_S (CA_MAXR + 8)          // bf16 per LDS row: 272 bytes, 16-byte aligned
// ldrop: the column stride of the dropout stream (the padded batch's L; the uniform decoder's own L)
template <bool DROP, class G>
__global__ void __launch_bounds__(256) k_msa_col_attn(const bf16_t* __restrict__ qkv, const float* __restrict__ kb, bf16_t* __restrict__ ctx, const G geo, int H,
                                                      int ldrop, float scale, const AttnDrop dr) {
  __shared__ __attribute__((aligned(16))) bf16_t sV[64 * CA_S];
  __shared__ __attribute__((aligned(16))) bf16_t sP[4][16 * CA_S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, g = lane >> 4, kq = g * 8;
  const int h = blockIdx.x, l = blockIdx.y;
  const MsaGeo mg = geo.at(blockIdx.z);
  const int R = mg.R, L = mg.L, b = mg.b;
  if (l >= L) return;                                     // whole work-group (ragged: a column past this MSA's own length), before the first barrier
  const int Rp = (R + 31) & ~31, ntile = (R + 15) >> 4, ld = 3 * H * 64;
  const size_t tok0 = mg.tok0 + l;                        // token of row r: tok0 + r * L
  for (int idx = tid; idx < Rp * 8; idx += 256) {
    const int key = idx >> 3, cg = (idx & 7) * 8;
    u32x4 w = *reinterpret_cast<const u32x4*>(qkv + (tok0 + (size_t)min(key, R - 1) * L) * ld + (2 * H + h) * 64 + cg);
    if (key >= R) w = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sV[(cg + 2 * e) * CA_S + key] = (bf16_t)(w[e] & 0xffffu);
      sV[(cg + 2 * e + 1) * CA_S + key] = (bf16_t)(w[e] >> 16);
    }
  }
  __syncthreads();
  bf16_t* sPw = sP[wave];
  for (int t0 = 0; t0 < ntile; t0 += 4) {                 // uniform trip count: every wave reaches the barrier
    const int t = t0 + wave;
    const bool act = t < ntile;
    if (act) {
      const bf16_t* pq = qkv + (tok0 + (size_t)min(t * 16 + fr, R - 1) * L) * ld + h * 64 + kq;
      const bf8_t q0 = msa_frag(pq), q1 = msa_frag(pq + 32);
      f32x4 s[CA_MAXR / 16];
      bool ok[CA_MAXR / 16];
#pragma unroll
      for (int nt = 0; nt < CA_MAXR / 16; ++nt) {
        s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        ok[nt] = false;
        if (nt * 16 < R) {                                 // uniform over the work-group
          const int j = nt * 16 + fr;
          const size_t tk = tok0 + (size_t)min(j, R - 1) * L;
          const bf16_t* pk = qkv + tk * ld + (H + h) * 64 + kq;
          s[nt] = MFMA16(q0, msa_frag(pk), s[nt]);
          s[nt] = MFMA16(q1, msa_frag(pk + 32), s[nt]);
          ok[nt] = j < R && kb[tk] == 0.f;                 // padded keys are excluded
        }
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {                  // query row g * 4 + reg of the tile; its keys: one per (nt, lane & 15)
        float m = -FLT_MAX;
#pragma unroll
        for (int nt = 0; nt < CA_MAXR / 16; ++nt) m = ok[nt] ? fmaxf(m, s[nt][reg] * scale) : m;
        m = row16_max(m);
        float sum = 0.f;
#pragma unroll
        for (int nt = 0; nt < CA_MAXR / 16; ++nt) {
          const float e = ok[nt] ? __expf(s[nt][reg] * scale - m) : 0.f;
          s[nt][reg] = e;
          sum += e;
        }
        sum = row16_sum(sum);
        const float inv = sum > 0.f ? 1.f / sum : 0.f;     // every key masked: probabilities 0, context 0 (finite)
#pragma unroll
        for (int nt = 0; nt < CA_MAXR / 16; ++nt)
          if (nt * 16 < Rp) {
            if (DROP) {                                    // fair-esm ColumnSelfAttention: dropout_module(attn_probs), one mask element per (b, h, l, i, j)
              const bool keep = attn_keep((unsigned)(t * 16 + g * 4 + reg), (unsigned)(nt * 16 + fr), (unsigned)((b * H + h) * ldrop + l), dr);
              sPw[(g * 4 + reg) * CA_S + nt * 16 + fr] = keep ? f2bf(s[nt][reg] * inv * dr.scale) : (bf16_t)0;
            } else {
              sPw[(g * 4 + reg) * CA_S + nt * 16 + fr] = f2bf(s[nt][reg] * inv);
            }
          }
      }
    }
    __syncthreads();
    if (act) {
      f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kc = 0; kc < Rp; kc += 32) {
        const bf8_t fp = msa_frag(sPw + fr * CA_S + kc + kq);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = MFMA16(msa_frag(sV + (nt * 16 + fr) * CA_S + kc + kq), fp, acc[nt]);
      }
      const int i = t * 16 + fr;
      if (i < R) {
        bf16_t* po = ctx + (tok0 + (size_t)i * L) * (size_t)(H * 64) + h * 64 + g * 4;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) *reinterpret_cast<u32x2*>(po + nt * 16) = u32x2{pack2bf(acc[nt][0], acc[nt][1]), pack2bf(acc[nt][2], acc[nt][3])};
      }
    }
    __syncthreads();
  }
}


// ---------------------------------------------------------------------------------------------------------------- host
static inline bool msa_shape_ok(int B, int R, int L, int H, int hd) {
  return B > 0 && R > 0 && L > 0 && H > 0 && hd == 64 && (int64_t)B * R * L <= 0x7fffffff && (int64_t)B * H <= 65535;
}
// a ragged call: n MSAs behind a 16-byte aligned table, the grid bounds max_R / max_L of the call's largest block
static inline bool msa_ragged_ok(const int64_t* geo, int n, int max_R, int max_L, int H, int hd) {
  return geo && !((uintptr_t)geo & 15) && n > 0 && max_R > 0 && max_R <= 65535 && max_L > 0 && max_L <= ONEPROT_MSA_MAX_LEN && H > 0 && hd == 64 && (int64_t)n * H <= 65535;
}
static inline bool msa_tail_ok(int T_tokens, int T_pad) { return T_tokens > 0 && T_tokens <= T_pad; }
// the stream's tail rows of ctx [T_pad, H * 64] hold 0 after every ragged attention call, as oneprot_attn_varlen_fwd leaves them
static inline bool msa_zero_tail(void* ctx, int T_tokens, int T_pad, int H, hipStream_t s) {
  if (T_tokens == T_pad) return true;
  return hipMemsetAsync((bf16_t*)ctx + (size_t)T_tokens * H * 64, 0, (size_t)(T_pad - T_tokens) * H * 64 * sizeof(bf16_t), s) == hipSuccess;
}

extern "C" int oneprot_msa_embed_fwd(const int64_t* tokens, const float* tok_table, const float* pos_table, const float* row_table, const float* gamma,
                                     const float* beta, float* x, int B, int R, int L, int d, int vocab, int n_pos, int n_rows, int pad_id, float eps,
                                     void* stream) {
  if (!tokens || !tok_table || !pos_table || !row_table || !gamma || !beta || !x) return OP_EINVAL;
  if (B <= 0 || R <= 0 || L <= 0 || d <= 0 || d > 64 * EMB_MAXV || vocab <= 0 || pad_id < 0 || R > n_rows || L + pad_id + 1 > n_pos) return OP_EINVAL;
  const int64_t T = (int64_t)B * R * L;
  if (T > 0x7fffffff) return OP_EINVAL;
  hipLaunchKernelGGL(k_msa_embed<false>, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const long long*)tokens, tok_table, pos_table, row_table,
                     gamma, beta, x, (long long)T, R, L, d, vocab, n_pos, pad_id, eps, (const int*)nullptr, (const int*)nullptr, 0, n_rows);
  return launch_status();
}

extern "C" int oneprot_msa_embed_ragged_fwd(const int64_t* tokens, const int* cu_tokens, const int* row_lens, const float* tok_table, const float* pos_table,
                                            const float* row_table, const float* gamma, const float* beta, float* x, int n, int T_pad, int max_R, int max_L, int d,
                                            int vocab, int n_pos, int n_rows, int pad_id, float eps, void* stream) {
  if (!tokens || !cu_tokens || !row_lens || !tok_table || !pos_table || !row_table || !gamma || !beta || !x) return OP_EINVAL;
  if (n <= 0 || n > 65535 || T_pad <= 0 || max_R <= 0 || max_L <= 0 || d <= 0 || d > 64 * EMB_MAXV || vocab <= 0 || pad_id < 0 || max_R > n_rows ||
      max_L + pad_id + 1 > n_pos)
    return OP_EINVAL;
  hipLaunchKernelGGL(k_msa_embed<true>, dim3((unsigned)(((int64_t)T_pad + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const long long*)tokens, tok_table, pos_table,
                     row_table, gamma, beta, x, (long long)T_pad, 0, 0, d, vocab, n_pos, pad_id, eps, cu_tokens, row_lens, n, n_rows);
  return launch_status();
}

extern "C" int oneprot_msa_row_scores(const void* qkv, const float* key_bias, float* S, int B, int R, int L, int H, int hd, float scale, void* stream) {
  if (!qkv || !key_bias || !S || !msa_shape_ok(B, R, L, H, hd) || L > ONEPROT_MSA_MAX_LEN || ((uintptr_t)qkv & 15)) return OP_EINVAL;
  const unsigned nt = (unsigned)((L + 127) / 128);
  hipLaunchKernelGGL(k_msa_row_scores<MsaUniform>, dim3(nt, nt, (unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, key_bias, S,
                     MsaUniform{R, L, (L + 31) & ~31, H}, H, scale);
  return launch_status();
}

extern "C" int oneprot_msa_row_scores_ragged(const void* qkv, const float* key_bias, float* S, const int64_t* geo, int n, int max_L, int H, int hd, float scale,
                                             void* stream) {
  if (!qkv || !key_bias || !S || !msa_ragged_ok(geo, n, 1, max_L, H, hd) || ((uintptr_t)qkv & 15)) return OP_EINVAL;
  const unsigned nt = (unsigned)((max_L + 127) / 128);
  hipLaunchKernelGGL(k_msa_row_scores<MsaRagged>, dim3(nt, nt, (unsigned)(n * H)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, key_bias, S,
                     MsaRagged{(const long long*)geo}, H, scale);
  return launch_status();
}

static inline size_t msa_p_bytes(int B, int L, int H) { return (size_t)B * H * L * ((L + 31) & ~31) * sizeof(bf16_t); }

extern "C" size_t oneprot_msa_row_context_workspace(int B, int R, int L, int H) {
  if (B <= 0 || R <= 0 || L <= 0 || H <= 0 || L > ONEPROT_MSA_MAX_LEN) return 0;
  return msa_p_bytes(B, L, H) + (size_t)B * H * R * 64 * ((L + 31) & ~31) * sizeof(bf16_t);
}

extern "C" size_t oneprot_msa_row_context_ragged_workspace(int64_t sum_l_lp, int64_t sum_r_lp, int H) {
  if (sum_l_lp <= 0 || sum_r_lp <= 0 || H <= 0 || (sum_l_lp & 31) || (sum_r_lp & 31)) return 0;
  return ((size_t)sum_l_lp + (size_t)sum_r_lp * 64) * H * sizeof(bf16_t);
}

static const AttnDrop kNoDrop = AttnDrop{0u, 0u, 0u, 1.0f};

// the three launches of the tied row context behind either decoder; n MSAs, grid bounds (max_R, max_L); dr = null: the undropped softmax
template <class G>
static void msa_row_context_kernels(const float* S, const void* qkv, const float* key_bias, void* ctx, bf16_t* P, bf16_t* Vt, const G geo, int n, int max_R, int max_L,
                                    int H, int b_first, const AttnDrop* dr, hipStream_t s) {
  const int Lp = (max_L + 31) & ~31;
  const dim3 gs((unsigned)((max_L + 3) / 4), (unsigned)(n * H));
  if (dr) hipLaunchKernelGGL((k_msa_row_softmax<true, G>), gs, dim3(256), 0, s, S, key_bias, P, geo, H, b_first, *dr);
  else hipLaunchKernelGGL((k_msa_row_softmax<false, G>), gs, dim3(256), 0, s, S, key_bias, P, geo, H, 0, kNoDrop);
  hipLaunchKernelGGL(k_msa_v_transpose<G>, dim3((unsigned)(Lp / 32), (unsigned)max_R, (unsigned)(n * H)), dim3(256), 0, s, (const bf16_t*)qkv, Vt, geo, H);
  hipLaunchKernelGGL(k_msa_row_pv<G>, dim3((unsigned)((max_L + 63) / 64), (unsigned)((max_R + 3) / 4), (unsigned)(n * H)), dim3(256), 0, s, (const bf16_t*)P,
                     (const bf16_t*)Vt, (bf16_t*)ctx, geo, H);
}

static int msa_row_context_launch(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes, int B, int R, int L, int H,
                                  int hd, int b_first, const AttnDrop* dr, void* stream) {
  if (!S || !qkv || !key_bias || !ctx || !workspace || !msa_shape_ok(B, R, L, H, hd) || L > ONEPROT_MSA_MAX_LEN || R > 65535 ||
      (((uintptr_t)qkv | (uintptr_t)ctx | (uintptr_t)workspace) & 15))
    return OP_EINVAL;
  if (workspace_bytes < oneprot_msa_row_context_workspace(B, R, L, H)) return OP_EINVAL;
  // P and Vt each start at their own base: the uniform decoder's p0 / vt0 count from there
  msa_row_context_kernels(S, qkv, key_bias, ctx, (bf16_t*)workspace, (bf16_t*)((char*)workspace + msa_p_bytes(B, L, H)), MsaUniform{R, L, (L + 31) & ~31, H}, B, R, L, H,
                          b_first, dr, (hipStream_t)stream);
  return launch_status();
}

// ragged: p0 and vt0 of the table both count bf16 elements from the start of the workspace
static int msa_row_context_ragged_launch(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes, const int64_t* geo,
                                         int n, int max_R, int max_L, int64_t sum_l_lp, int64_t sum_r_lp, int H, int hd, int T_tokens, int T_pad, int b_first,
                                         const AttnDrop* dr, void* stream) {
  if (!S || !qkv || !key_bias || !ctx || !workspace || !msa_ragged_ok(geo, n, max_R, max_L, H, hd) || !msa_tail_ok(T_tokens, T_pad) ||
      (((uintptr_t)qkv | (uintptr_t)ctx | (uintptr_t)workspace) & 15))
    return OP_EINVAL;
  const size_t need = oneprot_msa_row_context_ragged_workspace(sum_l_lp, sum_r_lp, H);
  if (need == 0 || workspace_bytes < need) return OP_EINVAL;
  msa_row_context_kernels(S, qkv, key_bias, ctx, (bf16_t*)workspace, (bf16_t*)workspace, MsaRagged{(const long long*)geo}, n, max_R, max_L, H, b_first, dr,
                          (hipStream_t)stream);
  if (!msa_zero_tail(ctx, T_tokens, T_pad, H, (hipStream_t)stream)) return OP_ELAUNCH;
  return launch_status();
}

extern "C" int oneprot_msa_row_context(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes, int B, int R,
                                       int L, int H, int hd, void* stream) {
  return msa_row_context_launch(S, qkv, key_bias, ctx, workspace, workspace_bytes, B, R, L, H, hd, 0, nullptr, stream);
}

extern "C" int oneprot_msa_row_context_dropout(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes, int B,
                                               int R, int L, int H, int hd, int b_first, float p, uint64_t seed, uint64_t stream_id, void* stream) {
  AttnDrop dr;
  if (attn_drop_make(p, seed, stream_id, dr) != OP_OK || b_first < 0 || B <= 0 || H <= 0 || ((int64_t)b_first + B) * H > 65535) return OP_EINVAL;
  return msa_row_context_launch(S, qkv, key_bias, ctx, workspace, workspace_bytes, B, R, L, H, hd, b_first, dr.thr16 ? &dr : nullptr, stream);
}

extern "C" int oneprot_msa_row_context_ragged(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes,
                                              const int64_t* geo, int n, int max_R, int max_L, int64_t sum_l_lp, int64_t sum_r_lp, int H, int hd, int T_tokens,
                                              int T_pad, void* stream) {
  return msa_row_context_ragged_launch(S, qkv, key_bias, ctx, workspace, workspace_bytes, geo, n, max_R, max_L, sum_l_lp, sum_r_lp, H, hd, T_tokens, T_pad, 0, nullptr,
                                       stream);
}

extern "C" int oneprot_msa_row_context_ragged_dropout(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes,
                                                      const int64_t* geo, int n, int max_R, int max_L, int64_t sum_l_lp, int64_t sum_r_lp, int H, int hd,
                                                      int T_tokens, int T_pad, int b_first, float p, uint64_t seed, uint64_t stream_id, void* stream) {
  AttnDrop dr;
  if (attn_drop_make(p, seed, stream_id, dr) != OP_OK || b_first < 0 || n <= 0 || H <= 0 || ((int64_t)b_first + n) * H > 65535) return OP_EINVAL;
  return msa_row_context_ragged_launch(S, qkv, key_bias, ctx, workspace, workspace_bytes, geo, n, max_R, max_L, sum_l_lp, sum_r_lp, H, hd, T_tokens, T_pad, b_first,
                                       dr.thr16 ? &dr : nullptr, stream);
}

static int msa_col_attn_launch(const void* qkv, const float* key_bias, void* ctx, int B, int R, int L, int H, int hd, float scale, const AttnDrop* dr, void* stream) {
  if (!qkv || !key_bias || !ctx || !msa_shape_ok(B, R, L, H, hd) || R < 2 || R > ONEPROT_MSA_MAX_ROWS || L > 65535 || B > 65535 ||
      (((uintptr_t)qkv | (uintptr_t)ctx) & 15))
    return OP_EINVAL;
  const dim3 grid((unsigned)H, (unsigned)L, (unsigned)B);
  const MsaUniform geo{R, L, (L + 31) & ~31, H};
  if (dr) hipLaunchKernelGGL((k_msa_col_attn<true, MsaUniform>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, key_bias, (bf16_t*)ctx, geo, H, L, scale, *dr);
  else hipLaunchKernelGGL((k_msa_col_attn<false, MsaUniform>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, key_bias, (bf16_t*)ctx, geo, H, L, scale, kNoDrop);
  return launch_status();
}

// ragged: R_b = 1 is accepted (one live key: P = 1, ctx = v -- what the padded kernel gives that MSA inside a deeper batch)
static int msa_col_attn_ragged_launch(const void* qkv, const float* key_bias, void* ctx, const int64_t* geo, int n, int max_R, int max_L, int H, int hd, float scale,
                                      int l_stride, int T_tokens, int T_pad, const AttnDrop* dr, void* stream) {
  if (!qkv || !key_bias || !ctx || !msa_ragged_ok(geo, n, max_R, max_L, H, hd) || max_R > ONEPROT_MSA_MAX_ROWS || !msa_tail_ok(T_tokens, T_pad) ||
      (((uintptr_t)qkv | (uintptr_t)ctx) & 15))
    return OP_EINVAL;
  const dim3 grid((unsigned)H, (unsigned)max_L, (unsigned)n);
  const MsaRagged g{(const long long*)geo};
  if (dr) hipLaunchKernelGGL((k_msa_col_attn<true, MsaRagged>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, key_bias, (bf16_t*)ctx, g, H, l_stride, scale, *dr);
  else hipLaunchKernelGGL((k_msa_col_attn<false, MsaRagged>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, key_bias, (bf16_t*)ctx, g, H, l_stride, scale, kNoDrop);
  if (!msa_zero_tail(ctx, T_tokens, T_pad, H, (hipStream_t)stream)) return OP_ELAUNCH;
  return launch_status();
}

extern "C" int oneprot_msa_col_attn(const void* qkv, const float* key_bias, void* ctx, int B, int R, int L, int H, int hd, float scale, void* stream) {
  return msa_col_attn_launch(qkv, key_bias, ctx, B, R, L, H, hd, scale, nullptr, stream);
}

extern "C" int oneprot_msa_col_attn_dropout(const void* qkv, const float* key_bias, void* ctx, int B, int R, int L, int H, int hd, float scale, float p, uint64_t seed,
                                            uint64_t stream_id, void* stream) {
  AttnDrop dr;
  if (attn_drop_make(p, seed, stream_id, dr) != OP_OK || L > ONEPROT_MSA_MAX_LEN) return OP_EINVAL;      // (b * H + h) * L + l stays below 2^26
  return msa_col_attn_launch(qkv, key_bias, ctx, B, R, L, H, hd, scale, dr.thr16 ? &dr : nullptr, stream);
}

extern "C" int oneprot_msa_col_attn_ragged(const void* qkv, const float* key_bias, void* ctx, const int64_t* geo, int n, int max_R, int max_L, int H, int hd, float scale,
                                           int T_tokens, int T_pad, void* stream) {
  return msa_col_attn_ragged_launch(qkv, key_bias, ctx, geo, n, max_R, max_L, H, hd, scale, max_L, T_tokens, T_pad, nullptr, stream);
}

extern "C" int oneprot_msa_col_attn_ragged_dropout(const void* qkv, const float* key_bias, void* ctx, const int64_t* geo, int n, int max_R, int max_L, int H, int hd,
                                                   float scale, int T_tokens, int T_pad, int l_stride, float p, uint64_t seed, uint64_t stream_id, void* stream) {
  AttnDrop dr;      // (b * H + h) * l_stride + l stays below 2^26: n * H <= 65535, l_stride <= 1024
  if (attn_drop_make(p, seed, stream_id, dr) != OP_OK || l_stride < max_L || l_stride > ONEPROT_MSA_MAX_LEN) return OP_EINVAL;
  return msa_col_attn_ragged_launch(qkv, key_bias, ctx, geo, n, max_R, max_L, H, hd, scale, l_stride, T_tokens, T_pad, dr.thr16 ? &dr : nullptr, stream);
}
