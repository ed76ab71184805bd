// LayerNorm backward, one token row per wave: the row body shared by k_layernorm_bwd (rowops.hip) and the LayerNorm role of k_gemm_tn8_ln (gemm_tn.hip),
// and the fixed-order reduction of the dgamma / dbeta partials both end in.
//   g = dy * gamma ; dx = rstd * (g - mean_d(g) - xhat * mean_d(g * xhat)) ; dgamma += dy * xhat ; dbeta += dy
// The body takes the row's operands from a SOURCE: LnBwdDirect loads them where the arithmetic asks for them (the one-row-at-a-time form of
// k_layernorm_bwd, whose 4-5 resident waves per SIMD cover the latency), LnBwdRow hands out what ln_bwd_row_load requested earlier (a kernel that loads
// later rows before it finishes the current one keeps those rows in flight under its arithmetic).  The arithmetic is one sequence of operations either way:
// dx and its bf16 copy do not depend on the source.
#pragma once
#include "common.h"

// DY_MODE 0: dy bf16 [T,d]   1: dy fp32 [T,d]   2, 3: dy[t,:] = dpool[dyrow, :] * w  (pooled-gradient broadcast; the caller finds dyrow)
template <int DY_MODE, int X_BF16, int NV>
struct LnBwdDirect {
  const void* __restrict__ dy; const void* __restrict__ x; const float* add_to;
  size_t row, dyrow; int d;
  float4 av[NV];
  __device__ __forceinline__ void begin(int lane, int nv4) {
#ifndef LN_BWD_LATE_ADD
    // the residual-gradient rows are requested together with x and dy: one exposed round trip per row instead of two (they are only needed after
    // the two wave reductions, but a load issued there starts a second latency that the 4-5 resident waves per SIMD do not cover)
    if (add_to) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv4) av[i] = reinterpret_cast<const float4*>(add_to + row * d)[c];
      }
    }
#endif
  }
  __device__ __forceinline__ auto xraw(int i, int c) const {
    if constexpr (X_BF16) return reinterpret_cast<const u32x2*>((const bf16_t*)x + row * d)[c];
    else return reinterpret_cast<const float4*>((const float*)x + row * d)[c];
  }
  __device__ __forceinline__ auto dyraw(int i, int c) const {
    if constexpr (DY_MODE == 0) return reinterpret_cast<const u32x2*>((const bf16_t*)dy + row * d)[c];
    else if constexpr (DY_MODE == 1) return reinterpret_cast<const float4*>((const float*)dy + row * d)[c];
    else return reinterpret_cast<const float4*>((const float*)dy + dyrow * d)[c];
  }
  // (re-read per row from L1: 12 registers fewer -> one more wave per SIMD)
  __device__ __forceinline__ float4 gamma4(int i, int c, const float* __restrict__ gamma) const { return reinterpret_cast<const float4*>(gamma)[c]; }
  __device__ __forceinline__ float4 add(int i, int c) const {
#ifdef LN_BWD_LATE_ADD
    return reinterpret_cast<const float4*>(add_to + row * d)[c];
#else
    return av[i];
#endif
  }
};

// a row of the form the towers' backward runs (dy bf16, x fp32), requested ahead of its arithmetic
template <int NV>
struct LnBwdRow {
  float4 xv[NV]; u32x2 dyp[NV]; float4 av[NV];
  float mean, rstd;
};
// ... as a source, with gamma held in registers by the kernel: a gamma load inside the arithmetic would be the newest load of the wave, and waiting for it
// (loads return in order) would wait for every row requested ahead as well
template <int NV>
struct LnBwdRowSrc {
  const LnBwdRow<NV>& r; const float4 (&gm)[NV];
  __device__ __forceinline__ float4 xraw(int i, int) const { return r.xv[i]; }
  __device__ __forceinline__ u32x2 dyraw(int i, int) const { return r.dyp[i]; }
  __device__ __forceinline__ float4 gamma4(int i, int, const float*) const { return gm[i]; }
  __device__ __forceinline__ float4 add(int i, int) const { return r.av[i]; }
};
// Every load is issued by every lane, whatever the width and whether or not there is an add_to: lanes past the row re-read its last float4, and without an
// add_to the x row is read in its place (results unused).  A load under a branch would be a load the wait counters cannot count on -- the compiler then waits
// for ALL loads before the first use, and the rows requested ahead would no longer be in flight under the arithmetic.
template <int NV>
__device__ __forceinline__ void ln_bwd_row_load(LnBwdRow<NV>& r, int row, const bf16_t* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean_in,
                                                const float* __restrict__ rstd_in, const float* add_to, int lane, int nv4, int d) {
  r.mean = mean_in[row];
  r.rstd = rstd_in[row];
  const float* ap = add_to ? add_to : x;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = min(lane + 64 * i, nv4 - 1);
    r.av[i] = reinterpret_cast<const float4*>(ap + (size_t)row * d)[c];
    r.xv[i] = reinterpret_cast<const float4*>(x + (size_t)row * d)[c];
    r.dyp[i] = reinterpret_cast<const u32x2*>(dy + (size_t)row * d)[c];
  }
}

__device__ __forceinline__ float4 ln_bwd_f4(const float4& v) { return v; }
__device__ __forceinline__ float4 ln_bwd_f4(const u32x2& p) { return make_float4(bflo(p.x), bfhi(p.x), bflo(p.y), bfhi(p.y)); }

// dx_out[row] = (has_add ? src.add : 0) + dx (the add_to row may be the dx_out row itself), optional bf16 copy; dg / db += this row's dgamma / dbeta terms
template <int DY_MODE, int NV, class Src>
__device__ __forceinline__ void ln_bwd_row(const Src& src, int row, float mean, float rstd, float w, const float* __restrict__ gamma, bool has_add, float* dx_out,
                                           bf16_t* __restrict__ dx_bf16, float4 (&dg)[NV], float4 (&db)[NV], int lane, int nv4, int d, float inv_d) {
  float4 xh[NV], g[NV];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < nv4) {
      const float4 xv = ln_bwd_f4(src.xraw(i, c));
      float4 dyv = ln_bwd_f4(src.dyraw(i, c));
      if (DY_MODE >= 2) { dyv.x *= w; dyv.y *= w; dyv.z *= w; dyv.w *= w; }
      xh[i] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
      const float4 gm = src.gamma4(i, c, gamma);
      g[i] = make_float4(dyv.x * gm.x, dyv.y * gm.y, dyv.z * gm.z, dyv.w * gm.w);
      s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
      s2 += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
      dg[i].x += dyv.x * xh[i].x; dg[i].y += dyv.y * xh[i].y; dg[i].z += dyv.z * xh[i].z; dg[i].w += dyv.w * xh[i].w;
      db[i].x += dyv.x; db[i].y += dyv.y; db[i].z += dyv.z; db[i].w += dyv.w;
    }
  }
  const float m1 = wave_sum(s1) * inv_d, m2 = wave_sum(s2) * inv_d;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < nv4) {
      float4 o;
      o.x = rstd * (g[i].x - m1 - xh[i].x * m2);
      o.y = rstd * (g[i].y - m1 - xh[i].y * m2);
      o.z = rstd * (g[i].z - m1 - xh[i].z * m2);
      o.w = rstd * (g[i].w - m1 - xh[i].w * m2);
      if (has_add) {
        const float4 a = src.add(i, c);
        o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
      }
      reinterpret_cast<float4*>(dx_out + (size_t)row * d)[c] = o;
      if (dx_bf16) { u32x2 pk; pk.x = pack2bf(o.x, o.y); pk.y = pack2bf(o.z, o.w); reinterpret_cast<u32x2*>(dx_bf16 + (size_t)row * d)[c] = pk; }
    }
  }
}

// dgamma_dbeta: [2][d] laid out as dgamma then dbeta (the two may be non-adjacent: pass both pointers)
// 16 columns per block, 64 part-slices per column (1024 threads: the 2048 x 2d partial matrix is 10 MB and the kernel is bound by loads in
// flight, not bandwidth; fixed summation order => deterministic)
static __global__ void __launch_bounds__(1024) k_ln_reduce(const float* __restrict__ partial, float* __restrict__ dgamma, float* __restrict__ dbeta, int nparts, int d, int accumulate) {
  __shared__ float s_sl[64][17];
  const int c = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + c;
  float s = 0.f;
  if (j < 2 * d)
    for (int p = sl; p < nparts; p += 64) s += partial[(size_t)p * 2 * d + j];
  s_sl[sl][c] = s;
  __syncthreads();
  if (sl < 4) {                       // 4 x 16 partial sums, then 4 -> 1
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += s_sl[sl * 16 + q][c];
    s_sl[sl][c] = t;
  }
  __syncthreads();
  if (sl == 0 && j < 2 * d) {
    const float t = (s_sl[0][c] + s_sl[1][c]) + (s_sl[2][c] + s_sl[3][c]);
    float* out = j < d ? dgamma + j : dbeta + (j - d);
    *out = accumulate ? *out + t : t;
  }
}
