// The downstream MLP probe (ref src/saprot_fit_mlp.py): "few rows" fp32 kernels.  A batch of the probe is 32 or 64 rows (at most ONEPROT_PROBE_MAX_BATCH for
// BatchNorm), the layers are 1280 x 512 x 256 x <= 1943 wide, and a training step is ~40 MFLOP: what it costs is the number of launches, not arithmetic.  So a
// work-group of the forward owns ALL rows of a column tile and finishes bias, BatchNorm statistics, activation, dropout and the residual sum in its epilogue, and
// the backward of norm + activation + dropout is one launch that owns whole columns as well.  Everything is fp32 fmaf chains in a fixed order (the logits feed a
// threshold search), no float atomics, and two runs give the same bits.  The dropout mask is the element rule of philox.h over the flat [M, n] index,
// regenerated in the backward and never stored.
#include "philox.h"
#include "../../include/oneprot_hip.h"

enum { PN_NONE = 0, PN_BN_TRAIN = 1, PN_BN_EVAL = 2, PN_LN = 3 };
enum { PA_ID = 0, PA_RELU = 1, PA_GELU = 2, PA_LEAKY = 3 };
#define PB_EPS 1e-5f            // nn.BatchNorm1d / nn.LayerNorm default eps
#define PB_MOMENTUM 0.1f        // nn.BatchNorm1d default momentum
typedef unsigned long long ull_t;

__device__ __forceinline__ float probe_act(float a, int act) {
  if (act == PA_RELU) return a <= 0.f ? 0.f : a;                                             // (NaN stays NaN)
  if (act == PA_GELU) return 0.5f * a * (1.0f + erff(a * 0.70710678118654752f));
  if (act == PA_LEAKY) return a <= 0.f ? 0.01f * a : a;
  return a;
}
__device__ __forceinline__ float probe_act_grad(float a, int act) {
  if (act == PA_RELU) return a > 0.f ? 1.f : 0.f;
  if (act == PA_GELU) return 0.5f * (1.0f + erff(a * 0.70710678118654752f)) + a * 0.3989422804014327f * expf(-0.5f * a * a);
  if (act == PA_LEAKY) return a > 0.f ? 1.f : 0.01f;
  return 1.f;
}
// element e of the flat [M, n] index under the element rule of philox.h
__device__ __forceinline__ float probe_drop(float y, size_t e, unsigned thr, float scale, ull_t seed, ull_t stream_id) {
  if (thr == 0u) return y;                                                                   // p = 0: scale is 1 and every element is kept
  return philox_slice16(e, seed, stream_id) >= thr ? y * scale : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Z[M, n] = gather(X, idx)[M, k] W[n, k]^T + b, epilogue Y = dropout(act(norm(Z))) (+ R).  Replaces the nn.Linear -> nn.BatchNorm1d -> activation -> nn.Dropout
// run of ref saprot_fit_mlp.py:74-92 and the residual sum of :110-113.  256 threads own a tile of 64 RM rows x 4 CN columns; thread (ty, tx) holds rows
// ty + 64 i and columns 4-or-2 tx + j.  K runs in slices of BK = 128 / RM through LDS, the next slice in flight during the multiply (as k_sgemm).
template <int RM, int CN>
__global__ void __launch_bounds__(256) k_probe_linear_fwd(const float* __restrict__ X, const int* __restrict__ idx, const float* __restrict__ W, const float* __restrict__ b,
                                                          float* __restrict__ Z, float* __restrict__ Y, const float* __restrict__ R, const int* __restrict__ ridx,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ mean, float* __restrict__ rstd,
                                                          float* rmean, float* rvar, int M, int n, int k, int norm, int act, unsigned thr, float scale, ull_t seed, ull_t stream_id) {
  constexpr int TM = 64 * RM, TN = 4 * CN, BK = 128 / RM;
  constexpr int NA = TM * BK / 256, NB = (TN * BK + 255) / 256;
  __shared__ float sA[BK][TM + 1];
  __shared__ float sB[BK][TN + 1];
  __shared__ int sRow[TM];
  __shared__ float sStat[2][TN];
  const int tid = threadIdx.x, tx = tid & 3, ty = tid >> 2;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  for (int r = tid; r < TM; r += 256) {
    const int gm = m0 + r;
    sRow[r] = gm < M ? (idx ? idx[gm] : gm) : -1;
  }
  __syncthreads();
  float acc[RM][CN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < CN; ++j) acc[i][j] = 0.f;
  float ra[NA], rb[NB];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int it = 0; it < NA; ++it) {
      const int e = tid + it * 256, mm = e / BK, kk = e % BK;
      const int row = sRow[mm];
      ra[it] = (row >= 0 && k0 + kk < k) ? X[(size_t)row * k + k0 + kk] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      const int e = tid + it * 256, nn = e / BK, kk = e % BK;
      rb[it] = (nn < TN && n0 + nn < n && k0 + kk < k) ? W[(size_t)(n0 + nn) * k + k0 + kk] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < k; k0 += BK) {
#pragma unroll
    for (int it = 0; it < NA; ++it) {
      const int e = tid + it * 256;
      sA[e % BK][e / BK] = ra[it];
    }
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      const int e = tid + it * 256;
      if (e / BK < TN) sB[e % BK][e / BK] = rb[it];
    }
    __syncthreads();
    if (k0 + BK < k) fetch(k0 + BK);
#pragma unroll 8
    for (int kk = 0; kk < BK; ++kk) {
      float a[RM], w[CN];
#pragma unroll
      for (int i = 0; i < RM; ++i) a[i] = sA[kk][ty + 64 * i];
#pragma unroll
      for (int j = 0; j < CN; ++j) w[j] = sB[kk][tx * CN + j];
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < CN; ++j) acc[i][j] = fmaf(a[i], w[j], acc[i][j]);
    }
    __syncthreads();
  }
  // ---- epilogue: bias, pre-norm Z
#pragma unroll
  for (int j = 0; j < CN; ++j) {
    const int gn = n0 + tx * CN + j;
    const float bj = (b && gn < n) ? b[gn] : 0.f;
#pragma unroll
    for (int i = 0; i < RM; ++i) {
      acc[i][j] += bj;
      const int gm = m0 + ty + 64 * i;
      if (Z && gm < M && gn < n) Z[(size_t)gm * n + gn] = acc[i][j];
    }
  }
  if (!Y) return;
  if (norm == PN_BN_TRAIN) {
    // the whole batch of a column is in this work-group (gridDim.y == 1, M <= TM): two-pass mean and biased variance, G = 256 / TN threads per column,
    // each over rows g, g + G, ... in order, then a butterfly over the G partials
    float* sZ = &sA[0][0];                                                // TM x TN, behind the last __syncthreads of the K loop
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < CN; ++j) sZ[(ty + 64 * i) * TN + tx * CN + j] = acc[i][j];
    __syncthreads();
    constexpr int G = 256 / TN;
    const int c = tid / G, g = tid % G;
    float s = 0.f;
    for (int r = g; r < M; r += G) s += sZ[r * TN + c];
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mu = s / (float)M;
    float v = 0.f;
    for (int r = g; r < M; r += G) { const float d = sZ[r * TN + c] - mu; v = fmaf(d, d, v); }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const float var = v / (float)M, rs = 1.0f / sqrtf(var + PB_EPS);
    if (g == 0) {
      sStat[0][c] = mu; sStat[1][c] = rs;
      const int gn = n0 + c;
      if (gn < n) {
        if (mean) mean[gn] = mu;
        if (rstd) rstd[gn] = rs;
        if (rmean) rmean[gn] = (1.0f - PB_MOMENTUM) * rmean[gn] + PB_MOMENTUM * mu;
        if (rvar) rvar[gn] = (1.0f - PB_MOMENTUM) * rvar[gn] + PB_MOMENTUM * (var * ((float)M / (float)(M - 1)));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < CN; ++j) {
    const int cl = tx * CN + j, gn = n0 + cl;
    if (gn >= n) continue;
    float mu = 0.f, rs = 1.f, ga = 1.f, be = 0.f;
    if (norm == PN_BN_TRAIN) { mu = sStat[0][cl]; rs = sStat[1][cl]; }
    if (norm == PN_BN_EVAL) { mu = rmean[gn]; rs = 1.0f / sqrtf(rvar[gn] + PB_EPS); }
    if (norm != PN_NONE) { ga = gamma[gn]; be = beta[gn]; }
#pragma unroll
    for (int i = 0; i < RM; ++i) {
      const int lr = ty + 64 * i, gm = m0 + lr;
      if (gm >= M) continue;
      float a = acc[i][j];
      if (norm != PN_NONE) a = fmaf((a - mu) * rs, ga, be);
      const size_t e = (size_t)gm * n + gn;
      float y = probe_drop(probe_act(a, act), e, thr, scale, seed, stream_id);
      if (R) y += R[(size_t)(ridx ? ridx[gm] : gm) * n + gn];
      Y[e] = y;
    }
  }
}

extern "C" int oneprot_probe_linear_fwd(const float* x, const int* idx, const float* w, const float* b, float* z, float* y, const float* resid, const int* resid_idx,
                                        const float* gamma, const float* beta, float* mean, float* rstd, float* running_mean, float* running_var, int M, int n, int k,
                                        int norm, int act, float p, uint64_t seed, uint64_t stream_id, void* stream) {
  unsigned thr; float scale;
  if (!x || !w || (!z && !y) || M < 1 || n < 1 || k < 1 || norm < PN_NONE || norm > PN_BN_EVAL || act < PA_ID || act > PA_LEAKY || !dropout_thr_scale(p, thr, scale)) return OP_EINVAL;
  if (norm != PN_NONE && (!y || !gamma || !beta)) return OP_EINVAL;
  if (norm == PN_BN_TRAIN && (M < 2 || M > ONEPROT_PROBE_MAX_BATCH)) return OP_EINVAL;      // nn.BatchNorm1d: "Expected more than 1 value per channel"
  if (norm == PN_BN_EVAL && (!running_mean || !running_var)) return OP_EINVAL;
#define PB_FWD(RM, CN) hipLaunchKernelGGL((k_probe_linear_fwd<RM, CN>), dim3((n + 4 * CN - 1) / (4 * CN), (M + 64 * RM - 1) / (64 * RM)), dim3(256), 0, (hipStream_t)stream, \
    x, idx, w, b, z, y, resid, resid_idx, gamma, beta, mean, rstd, running_mean, running_var, M, n, k, norm, act, thr, scale, (ull_t)seed, (ull_t)stream_id)
  if (M <= 64) PB_FWD(1, 2);
  else if (M <= 128) PB_FWD(2, 4);
  else PB_FWD(4, 4);
#undef PB_FWD
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// LayerNorm (eps 1e-5) + activation + dropout (+ R) in one pass over the rows of Z, a wave per row (ref saprot_fit_mlp.py:79-90 with use_layer_norm)
__global__ void __launch_bounds__(256) k_probe_rownorm_fwd(const float* __restrict__ Z, const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ Y,
                                                           const float* __restrict__ R, const int* __restrict__ ridx, float* __restrict__ mean, float* __restrict__ rstd,
                                                           int M, int n, int act, unsigned thr, float scale, ull_t seed, ull_t stream_id) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* z = Z + (size_t)row * n;
  float s = 0.f;
  for (int c = lane; c < n; c += 64) s += z[c];
  const float mu = wave_sum(s) / (float)n;
  float v = 0.f;
  for (int c = lane; c < n; c += 64) { const float d = z[c] - mu; v = fmaf(d, d, v); }
  const float rs = 1.0f / sqrtf(wave_sum(v) / (float)n + PB_EPS);
  const float* r = R ? R + (size_t)(ridx ? ridx[row] : row) * n : nullptr;
  for (int c = lane; c < n; c += 64) {
    const size_t e = (size_t)row * n + c;
    float y = probe_drop(probe_act(fmaf((z[c] - mu) * rs, gamma[c], beta[c]), act), e, thr, scale, seed, stream_id);
    if (r) y += r[c];
    Y[e] = y;
  }
  if (lane == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
}

extern "C" int oneprot_probe_rownorm_act_fwd(const float* z, const float* gamma, const float* beta, float* y, const float* resid, const int* resid_idx, float* mean,
                                             float* rstd, int M, int n, int act, float p, uint64_t seed, uint64_t stream_id, void* stream) {
  unsigned thr; float scale;
  if (!z || !gamma || !beta || !y || M < 1 || n < 1 || act < PA_ID || act > PA_LEAKY || !dropout_thr_scale(p, thr, scale)) return OP_EINVAL;
  hipLaunchKernelGGL(k_probe_rownorm_fwd, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, z, gamma, beta, y, resid, resid_idx, mean, rstd, M, n, act, thr, scale,
                     (ull_t)seed, (ull_t)stream_id);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Backward of Y = dropout(act(norm(Z))): u = dY * mask * act'(a) is dL/da, a = norm(Z).  A work-group of the column part owns 16 columns and walks every row:
// the two column sums s1 = sum u, s2 = sum u xhat ARE dbeta / dgamma and feed the BatchNorm (train) backward dz = gamma rstd (u - s1 / M - xhat s2 / M).
// (autograd's backward of ref saprot_fit_mlp.py:107-108.)  For LayerNorm the column part only writes the two sums; the rows are the row part's.
struct ProbeBwdArgs {
  const float *dY, *Z, *gamma, *beta, *mean, *rstd;
  float *dZ, *dgamma, *dbeta;
  int M, n, norm, act;
  unsigned thr; float scale; ull_t seed, stream_id;
};
__device__ __forceinline__ float probe_u(const ProbeBwdArgs& A, int row, int col, float mu, float rs, float ga, float be, float& xhat) {
  const size_t e = (size_t)row * A.n + col;
  const float z = A.Z[e];
  xhat = (z - mu) * rs;
  const float a = A.norm == PN_NONE ? z : fmaf(xhat, ga, be);
  const float u = probe_drop(A.dY[e], e, A.thr, A.scale, A.seed, A.stream_id);
  return u * probe_act_grad(a, A.act);
}
__device__ void probe_bwd_cols(const ProbeBwdArgs& A, int col_block) {
  __shared__ float red[2][16][17];
  const int tid = threadIdx.x, c = tid & 15, rg = tid >> 4, col = col_block * 16 + c;
  const bool live = col < A.n;
  float ga = 1.f, be = 0.f, mu = 0.f, rs = 1.f, s1 = 0.f, s2 = 0.f, xhat;
  if (A.norm != PN_NONE) {
    if (live) {
      ga = A.gamma[col]; be = A.beta[col];
      if (A.norm == PN_BN_TRAIN) { mu = A.mean[col]; rs = A.rstd[col]; }
      if (A.norm == PN_BN_EVAL) { mu = A.mean[col]; rs = 1.0f / sqrtf(A.rstd[col] + PB_EPS); }      // eval: the running mean and the running VARIANCE are handed in
      for (int r0 = rg; r0 < A.M; r0 += 128) {                  // eight rows at a time into a partial of their own: the chain stays short at any M
        float p1 = 0.f, p2 = 0.f;
        for (int r = r0; r < A.M && r < r0 + 128; r += 16) {
          if (A.norm == PN_LN) { mu = A.mean[r]; rs = A.rstd[r]; }
          const float u = probe_u(A, r, col, mu, rs, ga, be, xhat);
          p1 += u; p2 = fmaf(u, xhat, p2);
        }
        s1 += p1; s2 += p2;
      }
    }
    red[0][rg][c] = s1; red[1][rg][c] = s2;
    __syncthreads();
    for (int o = 8; o > 0; o >>= 1) {
      if (rg < o) { red[0][rg][c] += red[0][rg + o][c]; red[1][rg][c] += red[1][rg + o][c]; }
      __syncthreads();
    }
    s1 = red[0][0][c]; s2 = red[1][0][c];
    if (rg == 0 && live) {
      if (A.dbeta) A.dbeta[col] = s1;
      if (A.dgamma) A.dgamma[col] = s2;
    }
  }
  if (A.norm == PN_LN || !live) return;
  const float invM = 1.0f / (float)A.M;
  for (int r = rg; r < A.M; r += 16) {
    const float u = probe_u(A, r, col, mu, rs, ga, be, xhat);
    float dz = u;
    if (A.norm == PN_BN_TRAIN) dz = ga * rs * (u - s1 * invM - xhat * (s2 * invM));
    if (A.norm == PN_BN_EVAL) dz = ga * rs * u;
    A.dZ[(size_t)r * A.n + col] = dz;
  }
}
__global__ void __launch_bounds__(256) k_probe_norm_act_bwd(ProbeBwdArgs A) { probe_bwd_cols(A, blockIdx.x); }

// LayerNorm: blocks [0, col_blocks) are the column part (dgamma, dbeta), the rest walk the rows, a wave per row: g = u gamma, dz = rstd (g - mean(g) - xhat mean(g xhat))
__global__ void __launch_bounds__(256) k_probe_rownorm_act_bwd(ProbeBwdArgs A, int col_blocks) {
  if ((int)blockIdx.x < col_blocks) { probe_bwd_cols(A, blockIdx.x); return; }
  const int lane = threadIdx.x & 63, row = ((int)blockIdx.x - col_blocks) * 4 + (threadIdx.x >> 6);
  if (row >= A.M) return;
  const float mu = A.mean[row], rs = A.rstd[row];
  float s1 = 0.f, s2 = 0.f, xhat;
  {
    // no contraction in here: g must be the SAME rounded product in both passes.  Fused into `g - s1` it would be the unrounded one, and the residue of that
    // rounding, times rstd (316 where a row has no variance), would stand where the exact result is 0.
#pragma clang fp contract(off)
    for (int c = lane; c < A.n; c += 64) {
      const float g = probe_u(A, row, c, mu, rs, A.gamma[c], A.beta[c], xhat) * A.gamma[c];
      s1 += g; s2 = fmaf(g, xhat, s2);
    }
    s1 = wave_sum(s1) / (float)A.n; s2 = wave_sum(s2) / (float)A.n;
    for (int c = lane; c < A.n; c += 64) {
      const float g = probe_u(A, row, c, mu, rs, A.gamma[c], A.beta[c], xhat) * A.gamma[c];
      A.dZ[(size_t)row * A.n + c] = rs * ((g - s1) - xhat * s2);
    }
  }
}

extern "C" int oneprot_probe_norm_act_bwd(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* rstd, float* dz,
                                          float* dgamma, float* dbeta, int M, int n, int norm, int act, float p, uint64_t seed, uint64_t stream_id, void* stream) {
  ProbeBwdArgs A{dy, z, gamma, beta, mean, rstd, dz, dgamma, dbeta, M, n, norm, act, 0u, 1.f, (ull_t)seed, (ull_t)stream_id};
  if (!dy || !z || !dz || M < 1 || n < 1 || norm < PN_NONE || norm > PN_BN_EVAL || act < PA_ID || act > PA_LEAKY || !dropout_thr_scale(p, A.thr, A.scale)) return OP_EINVAL;
  if (norm != PN_NONE && (!gamma || !beta || !mean || !rstd)) return OP_EINVAL;
  if (norm == PN_BN_TRAIN && M < 2) return OP_EINVAL;
  hipLaunchKernelGGL(k_probe_norm_act_bwd, dim3((n + 15) / 16), dim3(256), 0, (hipStream_t)stream, A);
  return launch_status();
}

extern "C" int oneprot_probe_rownorm_act_bwd(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* rstd, float* dz,
                                             float* dgamma, float* dbeta, int M, int n, int act, float p, uint64_t seed, uint64_t stream_id, void* stream) {
  ProbeBwdArgs A{dy, z, gamma, beta, mean, rstd, dz, dgamma, dbeta, M, n, PN_LN, act, 0u, 1.f, (ull_t)seed, (ull_t)stream_id};
  if (!dy || !z || !gamma || !beta || !mean || !rstd || !dz || M < 1 || n < 1 || act < PA_ID || act > PA_LEAKY || !dropout_thr_scale(p, A.thr, A.scale)) return OP_EINVAL;
  const int col_blocks = (dgamma || dbeta) ? (n + 15) / 16 : 0;
  hipLaunchKernelGGL(k_probe_rownorm_act_bwd, dim3(col_blocks + (M + 3) / 4), dim3(256), 0, (hipStream_t)stream, A, col_blocks);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dW[n, k] = dZ[M, n]^T gather(X, idx)[M, k], db[n] = column sums of dZ (autograd's backward of nn.Linear, ref saprot_fit_mlp.py:75,95,99).  The contraction is
// the batch, so the work is spread over the n k outputs: 64 x 64 tiles, 4 x 4 per thread, the rows in slices of 32 and in order.
__global__ void __launch_bounds__(256) k_probe_bwd_w(const float* __restrict__ dZ, const float* __restrict__ X, const int* __restrict__ idx, float* __restrict__ dW,
                                                     float* __restrict__ db, int M, int n, int k) {
  __shared__ float sD[32][64];
  __shared__ float sX[32][64];
  __shared__ float sP[4][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  float bsum = 0.f;
  for (int m0 = 0; m0 < M; m0 += 32) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int e = tid + it * 256, mm = e >> 6, cc = e & 63, row = m0 + mm;
      const bool valid = row < M;
      sD[mm][cc] = (valid && n0 + cc < n) ? dZ[(size_t)row * n + n0 + cc] : 0.f;
      const int xr = valid ? (idx ? idx[row] : row) : 0;
      sX[mm][cc] = (valid && k0 + cc < k) ? X[(size_t)xr * k + k0 + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int mm = 0; mm < 32; ++mm) {
      float d[4], x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { d[i] = sD[mm][ty * 4 + i]; x[i] = sX[mm][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(d[i], x[j], acc[i][j]);
    }
    if (db && blockIdx.x == 0) {                                            // block-uniform.  Four partials of eight rows per slice, a fixed tree over them,
      const int c = tid & 63, q = tid >> 6;                                 // then the slices in order: a short chain at any M (rows past M hold 0)
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s += sD[q * 8 + i][c];
      sP[q][c] = s;
      __syncthreads();
      if (tid < 64) bsum += (sP[0][tid] + sP[1][tid]) + (sP[2][tid] + sP[3][tid]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gn = n0 + ty * 4 + i;
    if (gn >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gk = k0 + tx * 4 + j;
      if (gk < k) dW[(size_t)gn * k + gk] = acc[i][j];
    }
  }
  if (db && blockIdx.x == 0 && tid < 64 && n0 + tid < n) db[n0 + tid] = bsum;
}

extern "C" int oneprot_probe_linear_bwd_w(const float* dz, const float* x, const int* idx, float* dw, float* db, int M, int n, int k, void* stream) {
  if (!dz || !x || !dw || M < 1 || n < 1 || k < 1) return OP_EINVAL;
  hipLaunchKernelGGL(k_probe_bwd_w, dim3((k + 63) / 64, (n + 63) / 64), dim3(256), 0, (hipStream_t)stream, dz, x, idx, dw, db, M, n, k);
  return launch_status();
}

// dA[M, k] = dZ[M, n] W[n, k]: 32 x 32 tiles, 2 x 2 per thread, n in slices of 32 with the next slice in flight
__global__ void __launch_bounds__(256) k_probe_bwd_x(const float* __restrict__ dZ, const float* __restrict__ W, float* __restrict__ dA, int M, int n, int k) {
  __shared__ float sD[32][33];
  __shared__ float sW[32][33];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  float rd[4], rw[4];
  auto fetch = [&](int q0) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = tid + it * 256, r = e >> 5, c = e & 31;
      rd[it] = (m0 + r < M && q0 + c < n) ? dZ[(size_t)(m0 + r) * n + q0 + c] : 0.f;
      rw[it] = (q0 + r < n && c0 + c < k) ? W[(size_t)(q0 + r) * k + c0 + c] : 0.f;
    }
  };
  fetch(0);
  for (int q0 = 0; q0 < n; q0 += 32) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = tid + it * 256;
      sD[e >> 5][e & 31] = rd[it]; sW[e >> 5][e & 31] = rw[it];
    }
    __syncthreads();
    if (q0 + 32 < n) fetch(q0 + 32);
#pragma unroll 8
    for (int q = 0; q < 32; ++q) {
      const float d0 = sD[ty * 2][q], d1 = sD[ty * 2 + 1][q], w0 = sW[q][tx * 2], w1 = sW[q][tx * 2 + 1];
      acc[0][0] = fmaf(d0, w0, acc[0][0]); acc[0][1] = fmaf(d0, w1, acc[0][1]);
      acc[1][0] = fmaf(d1, w0, acc[1][0]); acc[1][1] = fmaf(d1, w1, acc[1][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gm = m0 + ty * 2 + i, gc = c0 + tx * 2 + j;
      if (gm < M && gc < k) dA[(size_t)gm * k + gc] = acc[i][j];
    }
}

extern "C" int oneprot_probe_linear_bwd_x(const float* dz, const float* w, float* da, int M, int n, int k, void* stream) {
  if (!dz || !w || !da || M < 1 || n < 1 || k < 1) return OP_EINVAL;
  hipLaunchKernelGGL(k_probe_bwd_x, dim3((k + 31) / 32, (M + 31) / 32), dim3(256), 0, (hipStream_t)stream, dz, w, da, M, n, k);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The three losses of ref saprot_fit_mlp.py:163-169,184 and their gradient (the mean already in it): per-work-group fp64 partials, then one ordered finish that
// adds weight x mean loss to loss_sum[0].  The number of work-groups depends on (M, C, kind) alone, so two runs give the same bits.
#define PB_LOSS_MAX_BLOCKS 256
__device__ __forceinline__ double probe_block_sum(double v, double* red) {      // fixed tree over the 256 threads; the result in every thread
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}
__global__ void __launch_bounds__(256) k_probe_loss_elem(const float* __restrict__ X, const float* __restrict__ T, const int* __restrict__ idx, float* __restrict__ dX,
                                                         double* __restrict__ partial, int M, int C, int kind, float inv) {
  __shared__ double red[256];
  const size_t total = (size_t)M * C;
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t row = e / C, col = e - row * C;
    const float x = X[e], y = T[(size_t)(idx ? idx[row] : (int)row) * C + col];
    float l, d;
    if (kind == 0) {                                                    // F.binary_cross_entropy_with_logits, the stable form
      const float t = expf(-fabsf(x));
      l = fmaxf(x, 0.f) - x * y + log1pf(t);
      const float sg = x >= 0.f ? 1.0f / (1.0f + t) : t / (1.0f + t);
      d = (sg - y) * inv;
      if (x != x) l = x;                                                // fmaxf drops a NaN: keep it
    } else {                                                            // F.mse_loss
      const float df = x - y;
      l = df * df;
      d = 2.0f * df * inv;
    }
    acc += (double)l;
    if (dX) dX[e] = d;
  }
  const double s = probe_block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// F.cross_entropy with int64 labels: a wave per row, row log-sum-exp
__global__ void __launch_bounds__(256) k_probe_loss_ce(const float* __restrict__ X, const int64_t* __restrict__ labels, const int* __restrict__ idx, float* __restrict__ dX,
                                                       double* __restrict__ partial, int M, int C, float inv) {
  __shared__ double red[256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc = 0.0;
  for (int row = blockIdx.x * 4 + w; row < M; row += gridDim.x * 4) {
    const float* x = X + (size_t)row * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(x[c] - mx);
    const float lg = logf(wave_sum(se));                                 // log-softmax as (x - max) - log(sum): nothing is rounded at the size of the logits
    const int64_t lab = labels[idx ? idx[row] : row];
    const bool ok = lab >= 0 && lab < C;
    if (lane == 0) acc += ok ? (double)(lg - (x[lab] - mx)) : (double)NAN;   // a label outside [0, C) is never read through: the loss turns NaN
    if (dX)
      for (int c = lane; c < C; c += 64) dX[(size_t)row * C + c] = (expf((x[c] - mx) - lg) - ((int64_t)c == lab ? 1.f : 0.f)) * inv;
  }
  const double s = probe_block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ void __launch_bounds__(64) k_probe_loss_finish(const double* __restrict__ partial, int blocks, double factor, double* __restrict__ loss_sum) {
  double s = 0.0;
  for (int i = threadIdx.x; i < blocks; i += 64) s += partial[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) loss_sum[0] += s * factor;
}

extern "C" size_t oneprot_probe_loss_workspace(void) { return PB_LOSS_MAX_BLOCKS * sizeof(double); }

extern "C" int oneprot_probe_loss_fwd_bwd(const float* logits, const float* target, const int64_t* labels, const int* idx, float* dlogits, void* loss_bytes,
                                          void* workspace, int M, int C, int kind, float weight, void* stream) {
  if (!logits || !loss_bytes || !workspace || M < 1 || C < 1 || kind < 0 || kind > 2) return OP_EINVAL;
  if ((kind == 2 ? !labels : !target) || (((uintptr_t)loss_bytes | (uintptr_t)workspace) & 7)) return OP_EINVAL;
  const size_t total = (size_t)M * C;
  const double denom = kind == 2 ? (double)M : (double)total;
  int blocks;
  if (kind == 2) {
    blocks = (M + 3) / 4;
    if (blocks > PB_LOSS_MAX_BLOCKS) blocks = PB_LOSS_MAX_BLOCKS;
    hipLaunchKernelGGL(k_probe_loss_ce, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, labels, idx, dlogits, (double*)workspace, M, C, (float)(1.0 / denom));
  } else {
    const size_t want = (total + 1023) / 1024;
    blocks = want > PB_LOSS_MAX_BLOCKS ? PB_LOSS_MAX_BLOCKS : (int)want;
    hipLaunchKernelGGL(k_probe_loss_elem, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, target, idx, dlogits, (double*)workspace, M, C, kind, (float)(1.0 / denom));
  }
  hipLaunchKernelGGL(k_probe_loss_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, blocks, (double)weight / denom, (double*)loss_bytes);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// torch.optim.AdamW (ref saprot_fit_mlp.py:205-207): decoupled decay p <- p (1 - lr wd), then the Adam update.  Any n.
__global__ void __launch_bounds__(256) k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n, float decay, float b1,
                                               float omb1, float b2, float omb2, float eps, float step_size, float bc2_sqrt) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float gg = g[i];
    const float mm = b1 * m[i] + omb1 * gg;
    const float vv = b2 * v[i] + omb2 * gg * gg;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p[i] = p[i] * decay - step_size * (mm / denom);
    m[i] = mm; v[i] = vv;
  }
}
// The betas travel as 1 - beta: 0.999 rounded to fp32 is off by 1.3e-8, which is 1.3e-5 of the 1 - beta2 = 0.001 that weighs g^2 (and of the bias correction
// 1 - beta2^step at small steps); 0.001 rounded to fp32 gives both to 5e-8.
extern "C" int oneprot_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float one_minus_beta1, float one_minus_beta2, float eps,
                                  float weight_decay, int step, void* stream) {
  if (!p || !g || !m || !v || n <= 0 || step < 1 || !(one_minus_beta1 > 0.f) || !(one_minus_beta1 <= 1.f) || !(one_minus_beta2 > 0.f) || !(one_minus_beta2 <= 1.f)) return OP_EINVAL;
  const double b1 = 1.0 - (double)one_minus_beta1, b2 = 1.0 - (double)one_minus_beta2;
  const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
  size_t blocks = ((size_t)n + 255) / 256; if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_adamw, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (size_t)n, (float)(1.0 - (double)lr * (double)weight_decay), (float)b1,
                     one_minus_beta1, (float)b2, one_minus_beta2, eps, (float)((double)lr / bc1), (float)sqrt(bc2));
  return launch_status();
}
