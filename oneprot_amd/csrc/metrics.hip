// Downstream metrics on the device (ref src/utils/downstream.py:12-59 `count_f1_max`; sklearn's roc_auc_score and scipy's spearmanr as the reference's
// saprot_fit_{cls,reg,mlp}.py call them): a stable LSD radix sort, midranks, ordered scans and sums, and F1-max built on them.
//
// Rules of the unit:
//   - no work-group waits on another (NOTEBOOK 6f): a radix pass is three launches -- histogram per tile, scan of the [256, tiles] table, ranked scatter;
//   - the same bits on every run: the order inside a tile comes from a wave ballot match and prefix counts; the only atomics are integer adds into
//     histograms, whose result does not depend on their order; every floating-point sum runs through one fixed tree whose shape depends on n alone
//     (chunks of ONEPROT_SCAN_TILE elements, eight consecutive elements per thread, a 64-lane shuffle tree, four waves left to right);
//   - nothing is read back, and every global index is 64-bit before it is scaled.
#include "common.h"
#include "../../include/oneprot_hip.h"

#define MT_THREADS 256
#define SORT_ITEMS 8
#define SORT_TILE (MT_THREADS * SORT_ITEMS)
#define SORT_WAVE_SPAN (64 * SORT_ITEMS)
#define SCAN_ITEMS 8
#define SCAN_TILE (MT_THREADS * SCAN_ITEMS)
#define MOM_ITEMS 32
#define MOM_CHUNK (MT_THREADS * MOM_ITEMS)
#define METRICS_MAX_N 0x7fffffffLL
static_assert(SORT_TILE == ONEPROT_SORT_TILE && SCAN_TILE == ONEPROT_SCAN_TILE, "the header states the tile sizes the tests import");

// ---------------------------------------------------------------------------------------------------------------- ordered scans
enum { SC_ADD = 0, SC_MAX = 1, SC_MIN = 2 };
template <typename T> struct SV { T v; int f; };      // a value and "a segment starts at or before this element, inside the span summed so far"
template <typename T, int OP> __device__ __forceinline__ T sc_op(T a, T b) {
  if (OP == SC_ADD) return a + b;
  if (OP == SC_MAX) return a > b ? a : b;
  return a < b ? a : b;
}
// the segmented-scan operator: associative, so one tree serves flat (no flag set) and segmented streams
template <typename T, int OP> __device__ __forceinline__ SV<T> sc_comb(SV<T> a, SV<T> b) {
  SV<T> r;
  r.v = b.f ? b.v : sc_op<T, OP>(a.v, b.v);
  r.f = a.f | b.f;
  return r;
}
template <typename T> __device__ __forceinline__ SV<T> sv_shfl_up(SV<T> x, int o) {
  SV<T> r;
  r.v = __shfl_up(x.v, o, 64);
  r.f = __shfl_up(x.f, o, 64);
  return r;
}

// Loads the chunk's elements (eight consecutive ones per thread), scans them and returns in e[] the inclusive scan inside the chunk; total = the chunk's
// fold.  Element i of the stream is in[REV ? n - 1 - i : i]; its flag is flags[i] when flags is given, else "i is a multiple of seg_len" (seg_len 0: none).
template <typename T, int OP, bool REV>
__device__ __forceinline__ void scan_chunk(const T* in, const int* __restrict__ flags, int64_t seg_len, int64_t n, SV<T> (&e)[SCAN_ITEMS], SV<T>& total,
                                           SV<T>* s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)tid * SCAN_ITEMS;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    const int64_t i = i0 + k;
    e[k].v = T(0);
    e[k].f = 0;
    if (i < n) {
      e[k].v = in[REV ? n - 1 - i : i];
      e[k].f = flags ? flags[i] : (seg_len > 0 && i % seg_len == 0) ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 1; k < SCAN_ITEMS; ++k) e[k] = sc_comb<T, OP>(e[k - 1], e[k]);
  SV<T> inc = e[SCAN_ITEMS - 1];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const SV<T> up = sv_shfl_up(inc, o);
    if (lane >= o) inc = sc_comb<T, OP>(up, inc);
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  SV<T> ex = sv_shfl_up(inc, 1);
  bool has = lane > 0;
  SV<T> wp = s_w[0];
  total = s_w[0];
#pragma unroll
  for (int w = 1; w < MT_THREADS / 64; ++w) {
    if (w < wave) wp = sc_comb<T, OP>(wp, s_w[w]);
    total = sc_comb<T, OP>(total, s_w[w]);
  }
  if (wave > 0) {
    ex = has ? sc_comb<T, OP>(wp, ex) : wp;
    has = true;
  }
  if (has) {
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) e[k] = sc_comb<T, OP>(ex, e[k]);
  }
}

template <typename T, int OP, bool REV>
__global__ void __launch_bounds__(MT_THREADS) k_metrics_scan_partial(const T* __restrict__ in, const int* __restrict__ flags, int64_t seg_len, int64_t n, T* __restrict__ pv,
                                                                     int* __restrict__ pf) {
  __shared__ SV<T> s_w[MT_THREADS / 64];
  SV<T> e[SCAN_ITEMS], total;
  scan_chunk<T, OP, REV>(in, flags, seg_len, n, e, total, s_w);
  if (threadIdx.x == 0) { pv[blockIdx.x] = total.v; pf[blockIdx.x] = total.f; }
}

// out may alias in: a block reads its chunk before it writes it, and the carries come from another array
template <typename T, int OP, bool REV>
__global__ void __launch_bounds__(MT_THREADS) k_metrics_scan_apply(const T* in, const int* __restrict__ flags, int64_t seg_len, int64_t n, const T* __restrict__ carry, T* out) {
  __shared__ SV<T> s_w[MT_THREADS / 64];
  SV<T> e[SCAN_ITEMS], total;
  scan_chunk<T, OP, REV>(in, flags, seg_len, n, e, total, s_w);
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  SV<T> c;
  c.f = 0;
  c.v = T(0);
  const bool has = carry != nullptr && blockIdx.x > 0;
  if (has) c.v = carry[blockIdx.x - 1];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i < n) out[REV ? n - 1 - i : i] = has ? sc_comb<T, OP>(c, e[k]).v : e[k].v;
  }
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// two levels of partials carry any n < 2^31: 2^20 chunk sums, then 512
static size_t scan_ws_bytes(int64_t n) {
  size_t b = 0;
  int64_t p = n;
  for (int lvl = 0; lvl < 2; ++lvl) {
    if (p <= SCAN_TILE) break;
    p = cdiv(p, SCAN_TILE);
    b += al256((size_t)p * 8) + al256((size_t)p * 4);
  }
  return b;
}

template <typename T, int OP, bool REV>
static void scan_run(const T* in, T* out, int64_t n, int64_t seg_len, char* ws, hipStream_t st) {
  const dim3 blk(MT_THREADS);
  const int64_t p1 = cdiv(n, SCAN_TILE);
  if (p1 <= 1) {
    hipLaunchKernelGGL((k_metrics_scan_apply<T, OP, REV>), dim3(1), blk, 0, st, in, (const int*)nullptr, seg_len, n, (const T*)nullptr, out);
    return;
  }
  T* pv1 = reinterpret_cast<T*>(ws);
  int* pf1 = reinterpret_cast<int*>(ws + al256((size_t)p1 * 8));
  ws += al256((size_t)p1 * 8) + al256((size_t)p1 * 4);
  hipLaunchKernelGGL((k_metrics_scan_partial<T, OP, REV>), dim3((unsigned)p1), blk, 0, st, in, (const int*)nullptr, seg_len, n, pv1, pf1);
  const int64_t p2 = cdiv(p1, SCAN_TILE);
  if (p2 <= 1) {
    hipLaunchKernelGGL((k_metrics_scan_apply<T, OP, false>), dim3(1), blk, 0, st, (const T*)pv1, (const int*)pf1, (int64_t)0, p1, (const T*)nullptr, pv1);
  } else {
    T* pv2 = reinterpret_cast<T*>(ws);
    int* pf2 = reinterpret_cast<int*>(ws + al256((size_t)p2 * 8));
    hipLaunchKernelGGL((k_metrics_scan_partial<T, OP, false>), dim3((unsigned)p2), blk, 0, st, (const T*)pv1, (const int*)pf1, (int64_t)0, p1, pv2, pf2);
    hipLaunchKernelGGL((k_metrics_scan_apply<T, OP, false>), dim3(1), blk, 0, st, (const T*)pv2, (const int*)pf2, (int64_t)0, p2, (const T*)nullptr, pv2);      // p2 <= 512
    hipLaunchKernelGGL((k_metrics_scan_apply<T, OP, false>), dim3((unsigned)p2), blk, 0, st, (const T*)pv1, (const int*)pf1, (int64_t)0, p1, (const T*)pv2, pv1);
  }
  hipLaunchKernelGGL((k_metrics_scan_apply<T, OP, REV>), dim3((unsigned)p1), blk, 0, st, in, (const int*)nullptr, seg_len, n, (const T*)pv1, out);
}

extern "C" size_t oneprot_scan_workspace(int64_t n) {
  if (n < 1 || n > METRICS_MAX_N) return 0;
  return scan_ws_bytes(n) + 256;      // never 0 for a valid n
}

extern "C" int oneprot_inclusive_scan(const void* x, void* y, int64_t n, int64_t seg_len, int is_f64, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !y || !workspace || n < 1 || n > METRICS_MAX_N || seg_len < 0 || (is_f64 != 0 && is_f64 != 1)) return OP_EINVAL;
  if (workspace_bytes < oneprot_scan_workspace(n) || ((uintptr_t)workspace & 7) || ((uintptr_t)x & (is_f64 ? 7 : 3)) || ((uintptr_t)y & (is_f64 ? 7 : 3))) return OP_EINVAL;
  if (is_f64) scan_run<double, SC_ADD, false>((const double*)x, (double*)y, n, seg_len, (char*)workspace, (hipStream_t)stream);
  else scan_run<int, SC_ADD, false>((const int*)x, (int*)y, n, seg_len, (char*)workspace, (hipStream_t)stream);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- moments
#define MOM_K 7
__device__ __forceinline__ void mom_block_fold(double (&s)[MOM_K], double (*s_m)[MOM_K]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < MOM_K; ++q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o, 64);      // a butterfly: every lane ends with the same bits (+ is commutative)
    if (lane == 0) s_m[wave][q] = s[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < MOM_K; ++q) s[q] = ((s_m[0][q] + s_m[1][q]) + s_m[2][q]) + s_m[3][q];
}

template <typename T>
__global__ void __launch_bounds__(MT_THREADS) k_metrics_moments_partial(const T* __restrict__ a, const T* __restrict__ b, int64_t n, double sa, double sb, double* __restrict__ part) {
  __shared__ double s_m[MT_THREADS / 64][MOM_K];
  double s[MOM_K] = {0, 0, 0, 0, 0, 0, 0};
  const int64_t base = (int64_t)blockIdx.x * MOM_CHUNK + threadIdx.x;
  for (int j = 0; j < MOM_ITEMS; ++j) {
    const int64_t i = base + (int64_t)j * MT_THREADS;
    if (i < n) {
      const T ra = a[i], rb = b[i];
      const double x = (double)ra - sa, y = (double)rb - sb, d = x - y;
      s[0] += x; s[1] += y; s[2] += x * x; s[3] += y * y; s[4] += x * y; s[5] += d * d; s[6] += (ra == rb) ? 1.0 : 0.0;
    }
  }
  mom_block_fold(s, s_m);
  if (threadIdx.x < MOM_K) part[(size_t)blockIdx.x * MOM_K + threadIdx.x] = s[threadIdx.x];
}

__global__ void __launch_bounds__(MT_THREADS) k_metrics_moments_final(const double* __restrict__ part, int64_t chunks, int64_t n, double* __restrict__ out) {
  __shared__ double s_m[MT_THREADS / 64][MOM_K];
  double s[MOM_K] = {0, 0, 0, 0, 0, 0, 0};
  for (int64_t c = threadIdx.x; c < chunks; c += MT_THREADS)
#pragma unroll
    for (int q = 0; q < MOM_K; ++q) s[q] += part[(size_t)c * MOM_K + q];
  mom_block_fold(s, s_m);
  if (threadIdx.x == 0) out[0] = (double)n;
  if (threadIdx.x < MOM_K) out[1 + threadIdx.x] = s[threadIdx.x];
}

extern "C" size_t oneprot_moments_workspace(int64_t n) {
  if (n < 1 || n > METRICS_MAX_N) return 0;
  return al256((size_t)cdiv(n, MOM_CHUNK) * MOM_K * sizeof(double));
}

extern "C" int oneprot_moments(const void* a, const void* b, int64_t n, int is_i32, float shift_a, float shift_b, void* moments_bytes, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (!a || !b || !moments_bytes || !workspace || n < 1 || n > METRICS_MAX_N || (is_i32 != 0 && is_i32 != 1)) return OP_EINVAL;
  if (workspace_bytes < oneprot_moments_workspace(n) || ((uintptr_t)workspace & 7) || ((uintptr_t)moments_bytes & 7) || (((uintptr_t)a | (uintptr_t)b) & 3)) return OP_EINVAL;
  const int64_t chunks = cdiv(n, MOM_CHUNK);
  double* part = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (is_i32) hipLaunchKernelGGL(k_metrics_moments_partial<int>, dim3((unsigned)chunks), dim3(MT_THREADS), 0, st, (const int*)a, (const int*)b, n, (double)shift_a, (double)shift_b, part);
  else hipLaunchKernelGGL(k_metrics_moments_partial<float>, dim3((unsigned)chunks), dim3(MT_THREADS), 0, st, (const float*)a, (const float*)b, n, (double)shift_a, (double)shift_b, part);
  hipLaunchKernelGGL(k_metrics_moments_final, dim3(1), dim3(MT_THREADS), 0, st, (const double*)part, chunks, n, (double*)moments_bytes);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- radix sort
// key modes of a pass's input: the stored unsigned key, or an fp32 read through the order-preserving map (descending = its complement, so that equal keys
// keep ascending index in both directions; -0 is made +0 first: the two zeros are equal keys)
enum { KM_RAW = 0, KM_F32_ASC = 1, KM_F32_DESC = 2 };
__device__ __forceinline__ unsigned f32_key(float f) {
  unsigned u = __builtin_bit_cast(unsigned, f);
  u = u == 0x80000000u ? 0u : u;      // on the bits, not `f + 0`: no arithmetic touches a denormal key
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned u) {
  u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
  return __builtin_bit_cast(float, u);
}
template <int KM> __device__ __forceinline__ unsigned load_key(const void* __restrict__ keys, int64_t i) {
  if (KM == KM_RAW) return reinterpret_cast<const unsigned*>(keys)[i];
  const unsigned u = f32_key(reinterpret_cast<const float*>(keys)[i]);
  return KM == KM_F32_DESC ? ~u : u;
}

// table[d * tiles + t] = number of keys of tile t whose digit is d (digit-major: one flat scan of the table orders digits first, tiles second)
template <int KM>
__global__ void __launch_bounds__(MT_THREADS) k_metrics_radix_hist(const void* __restrict__ keys, int64_t n, int shift, int* __restrict__ table, int64_t tiles) {
  __shared__ int hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE + threadIdx.x;
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const int64_t i = base + (int64_t)j * MT_THREADS;
    if (i < n) atomicAdd(&hist[(load_key<KM>(keys, i) >> shift) & 255u], 1);      // integer counts: any order gives the same histogram
  }
  __syncthreads();
  table[(size_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

// A wave owns SORT_WAVE_SPAN consecutive elements of the tile and walks them 64 at a time.  In a round the lanes that hold the same digit find each other
// with eight ballots; an element's place among them is the number of lower lanes in that set, and the per-wave digit counter (touched by its own wave only:
// the 64 lanes execute each LDS instruction together and in program order, so the set's first lane advances it after every lane of the set has read it, with
// no work-group barrier) carries the count from round to round.  The tile is then laid out in LDS in its sorted order and written from there, so that
// consecutive lanes store to consecutive addresses inside a digit's run.  table is the INCLUSIVE scan of the histogram table.
template <int KM>
__global__ void __launch_bounds__(MT_THREADS) k_metrics_radix_scatter(const void* __restrict__ keys, const int* __restrict__ vals, int64_t n, int shift,
                                                                      const int* __restrict__ table, int64_t tiles, unsigned* __restrict__ keys_out, int* __restrict__ vals_out) {
  __shared__ unsigned whist[MT_THREADS / 64][256];      // per wave and digit: the count so far, then the wave's start inside the digit's run
  __shared__ unsigned dstart[256];                      // where digit d begins in the sorted tile
  __shared__ unsigned gstart[256];                      // where this tile's run of digit d begins in the output
  __shared__ unsigned s_wsum[MT_THREADS / 64];
  __shared__ unsigned skey[SORT_TILE];
  __shared__ int sval[SORT_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int w = 0; w < MT_THREADS / 64; ++w) whist[w][tid] = 0u;
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * SORT_TILE;
  const int64_t first = tile0 + (int64_t)wave * SORT_WAVE_SPAN + lane;
  unsigned key[SORT_ITEMS], loc[SORT_ITEMS];
  int val[SORT_ITEMS];
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const int64_t i = first + (int64_t)j * 64;
    key[j] = 0u;
    val[j] = 0;
    if (i < n) {
      key[j] = load_key<KM>(keys, i);
      val[j] = vals ? vals[i] : (int)i;
    }
  }
  const unsigned long long lower = (1ull << lane) - 1ull;
  volatile unsigned* mine = whist[wave];
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const bool valid = first + (int64_t)j * 64 < n;
    const unsigned d = (key[j] >> shift) & 255u;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    const unsigned below = (unsigned)__popcll(same & lower), cnt = (unsigned)__popcll(same);
    const unsigned pre = valid ? mine[d] : 0u;
    __builtin_amdgcn_wave_barrier();
    if (valid && below == 0u) mine[d] = pre + cnt;
    __builtin_amdgcn_wave_barrier();
    loc[j] = pre + below;
  }
  __syncthreads();
  {
    unsigned tot = 0u;      // thread tid owns digit tid
#pragma unroll
    for (int w = 0; w < MT_THREADS / 64; ++w) {
      const unsigned c = whist[w][tid];
      whist[w][tid] = tot;
      tot += c;
    }
    unsigned inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0u;
#pragma unroll
    for (int w = 0; w < MT_THREADS / 64; ++w) before += w < wave ? s_wsum[w] : 0u;
    dstart[tid] = before + inc - tot;
    gstart[tid] = (unsigned)table[(size_t)tid * tiles + blockIdx.x] - tot;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    if (first + (int64_t)j * 64 < n) {
      const unsigned d = (key[j] >> shift) & 255u;
      const unsigned p = dstart[d] + whist[wave][d] + loc[j];
      if (p < SORT_TILE) {                                      // always true for consistent counts; an out-of-range LDS store is never issued
        skey[p] = key[j];
        sval[p] = val[j];
      }
    }
  }
  __syncthreads();
  const int64_t left = n - tile0;
  const unsigned count = left < SORT_TILE ? (unsigned)left : (unsigned)SORT_TILE;
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const unsigned p = (unsigned)j * MT_THREADS + tid;
    if (p < count) {
      const unsigned k = skey[p], d = (k >> shift) & 255u;
      const int64_t pos = (int64_t)gstart[d] + (int64_t)(p - dstart[d]);
      if (pos >= 0 && pos < n) {                                // always true for a correct table; an out-of-range store is never issued
        if (keys_out) keys_out[pos] = k;
        vals_out[pos] = sval[p];
      }
    }
  }
}

__global__ void __launch_bounds__(MT_THREADS) k_metrics_decode_keys(const unsigned* __restrict__ keys, float* __restrict__ out, int64_t n, int descending) {
  const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (i < n) out[i] = key_f32(descending ? ~keys[i] : keys[i]);
}
__global__ void __launch_bounds__(MT_THREADS) k_metrics_copy_pairs(const int* __restrict__ keys, const int* __restrict__ vals, int64_t n, int* __restrict__ keys_out,
                                                                   int* __restrict__ vals_out) {
  const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (i < n) {
    if (keys_out) keys_out[i] = keys[i];
    vals_out[i] = vals ? vals[i] : (int)i;
  }
}

struct SortWs {
  unsigned* kb[2];
  int* vb[2];
  int* table;
  char* scan_ws;
};
static size_t sort_layout(int64_t n, char* base, SortWs* w) {
  const int64_t tiles = cdiv(n, SORT_TILE);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
  char* k0 = take((size_t)n * 4); char* k1 = take((size_t)n * 4); char* v0 = take((size_t)n * 4); char* v1 = take((size_t)n * 4);
  char* tb = take((size_t)tiles * 256 * 4);
  char* sw = take(scan_ws_bytes(tiles * 256) + 256);
  if (w) { w->kb[0] = (unsigned*)k0; w->kb[1] = (unsigned*)k1; w->vb[0] = (int*)v0; w->vb[1] = (int*)v1; w->table = (int*)tb; w->scan_ws = sw; }
  return off;
}

// `passes` 8-bit passes from bit 0 up; pass 0 reads keys_in in mode km0 and vals_in (nullptr = 0 .. n-1); the last pass writes keys_out (optional, the
// unsigned keys) and vals_out.  Source and destination of a pass never alias.
static void sort_run(int km0, const void* keys_in, const int* vals_in, int64_t n, int passes, unsigned* keys_out, int* vals_out, const SortWs& w, hipStream_t st) {
  const int64_t tiles = cdiv(n, SORT_TILE);
  const dim3 grid((unsigned)tiles), blk(MT_THREADS);
  for (int p = 0; p < passes; ++p) {
    const void* ks = p == 0 ? keys_in : (const void*)w.kb[(p - 1) & 1];
    const int* vs = p == 0 ? vals_in : (const int*)w.vb[(p - 1) & 1];
    unsigned* kd = p == passes - 1 ? keys_out : w.kb[p & 1];
    int* vd = p == passes - 1 ? vals_out : w.vb[p & 1];
    const int km = p == 0 ? km0 : KM_RAW, shift = 8 * p;
    if (km == KM_RAW) hipLaunchKernelGGL(k_metrics_radix_hist<KM_RAW>, grid, blk, 0, st, ks, n, shift, w.table, tiles);
    else if (km == KM_F32_ASC) hipLaunchKernelGGL(k_metrics_radix_hist<KM_F32_ASC>, grid, blk, 0, st, ks, n, shift, w.table, tiles);
    else hipLaunchKernelGGL(k_metrics_radix_hist<KM_F32_DESC>, grid, blk, 0, st, ks, n, shift, w.table, tiles);
    scan_run<int, SC_ADD, false>((const int*)w.table, w.table, tiles * 256, 0, w.scan_ws, st);
    if (km == KM_RAW) hipLaunchKernelGGL(k_metrics_radix_scatter<KM_RAW>, grid, blk, 0, st, ks, vs, n, shift, (const int*)w.table, tiles, kd, vd);
    else if (km == KM_F32_ASC) hipLaunchKernelGGL(k_metrics_radix_scatter<KM_F32_ASC>, grid, blk, 0, st, ks, vs, n, shift, (const int*)w.table, tiles, kd, vd);
    else hipLaunchKernelGGL(k_metrics_radix_scatter<KM_F32_DESC>, grid, blk, 0, st, ks, vs, n, shift, (const int*)w.table, tiles, kd, vd);
  }
}

extern "C" size_t oneprot_sort_workspace(int64_t n) {
  if (n < 1 || n > METRICS_MAX_N) return 0;
  return sort_layout(n, nullptr, nullptr);
}

extern "C" int oneprot_sort_f32(const float* keys, int64_t n, int descending, int* perm, float* sorted_keys, void* workspace, size_t workspace_bytes, void* stream) {
  if (!keys || !perm || !workspace || n < 1 || n > METRICS_MAX_N || (descending != 0 && descending != 1)) return OP_EINVAL;
  if (workspace_bytes < oneprot_sort_workspace(n) || ((uintptr_t)workspace & 7)) return OP_EINVAL;
  SortWs w;
  sort_layout(n, (char*)workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  sort_run(descending ? KM_F32_DESC : KM_F32_ASC, keys, nullptr, n, 4, sorted_keys ? w.kb[1] : nullptr, perm, w, st);      // the last of 4 passes reads kb[0]
  if (sorted_keys) hipLaunchKernelGGL(k_metrics_decode_keys, dim3((unsigned)cdiv(n, MT_THREADS)), dim3(MT_THREADS), 0, st, (const unsigned*)w.kb[1], sorted_keys, n, descending);
  return launch_status();
}

extern "C" int oneprot_sort_i32(const int* keys, const int* values, int64_t n, int key_bits, int* keys_out, int* values_out, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (!keys || !values_out || !workspace || n < 1 || n > METRICS_MAX_N || key_bits < 1 || key_bits > 31) return OP_EINVAL;
  if (workspace_bytes < oneprot_sort_workspace(n) || ((uintptr_t)workspace & 7)) return OP_EINVAL;
  if (keys_out == keys || values_out == values) return OP_EINVAL;      // a pass never sorts in place
  SortWs w;
  sort_layout(n, (char*)workspace, &w);
  sort_run(KM_RAW, keys, values, n, (key_bits + 7) / 8, (unsigned*)keys_out, values_out, w, (hipStream_t)stream);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- midranks
// in the ascending order: lo[p] = p where a run of equal keys begins, else -1; hi[p] = p where one ends, else INT_MAX.  A forward max-scan of lo and a
// backward min-scan of hi give every position the first and the last position of its run.
__global__ void __launch_bounds__(MT_THREADS) k_metrics_run_bounds(const unsigned* __restrict__ keys, int64_t n, int* __restrict__ lo, int* __restrict__ hi) {
  const int64_t p = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (p >= n) return;
  const unsigned k = keys[p];
  lo[p] = (p == 0 || keys[p - 1] != k) ? (int)p : -1;
  hi[p] = (p == n - 1 || keys[p + 1] != k) ? (int)p : 0x7fffffff;
}
__global__ void __launch_bounds__(MT_THREADS) k_metrics_rank_scatter(const int* __restrict__ perm, const int* __restrict__ lo, const int* __restrict__ hi, int64_t n,
                                                                     int* __restrict__ rank2) {
  const int64_t p = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (p >= n) return;
  const unsigned src = (unsigned)perm[p];
  if (src < (unsigned long long)n) rank2[src] = (int)((unsigned)lo[p] + (unsigned)hi[p] + 2u);      // n = 2^31 - 1 reaches 2^32 - 2: the caller reads it unsigned
}

struct RankWs { SortWs sort; unsigned* keys; int* perm; int* lo; int* hi; char* scan_ws; };
static size_t rank_layout(int64_t n, char* base, RankWs* w) {
  size_t off = sort_layout(n, base, w ? &w->sort : nullptr);
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
  char* k = take((size_t)n * 4); char* pm = take((size_t)n * 4); char* lo = take((size_t)n * 4); char* hi = take((size_t)n * 4);
  char* sw = take(scan_ws_bytes(n) + 256);
  if (w) { w->keys = (unsigned*)k; w->perm = (int*)pm; w->lo = (int*)lo; w->hi = (int*)hi; w->scan_ws = sw; }
  return off;
}

extern "C" size_t oneprot_midranks_workspace(int64_t n) {
  if (n < 1 || n > METRICS_MAX_N) return 0;
  return rank_layout(n, nullptr, nullptr);
}

extern "C" int oneprot_midranks_f32(const float* x, int64_t n, int* rank2, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !rank2 || !workspace || n < 1 || n > METRICS_MAX_N) return OP_EINVAL;
  if (workspace_bytes < oneprot_midranks_workspace(n) || ((uintptr_t)workspace & 7)) return OP_EINVAL;
  RankWs w;
  rank_layout(n, (char*)workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(n, MT_THREADS)), blk(MT_THREADS);
  sort_run(KM_F32_ASC, x, nullptr, n, 4, w.keys, w.perm, w.sort, st);
  hipLaunchKernelGGL(k_metrics_run_bounds, grid, blk, 0, st, (const unsigned*)w.keys, n, w.lo, w.hi);
  scan_run<int, SC_MAX, false>((const int*)w.lo, w.lo, n, 0, w.scan_ws, st);
  scan_run<int, SC_MIN, true>((const int*)w.hi, w.hi, n, 0, w.scan_ws, st);
  hipLaunchKernelGGL(k_metrics_rank_scatter, grid, blk, 0, st, (const int*)w.perm, (const int*)w.lo, (const int*)w.hi, n, rank2);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- F1-max
// (ref src/utils/downstream.py:12-59.)  order[k] = flat index of the k-th score in the global descending order; a stable sort of the positions k by row
// id then lays every row out as N consecutive slots q in its own descending order, without a per-row sort or a segment table.
__global__ void __launch_bounds__(MT_THREADS) k_metrics_f1_rows(const int* __restrict__ order, int64_t n, int N, int* __restrict__ row) {
  const int64_t k = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (k < n) row[k] = order[k] / N;
}
__global__ void __launch_bounds__(MT_THREADS) k_metrics_f1_targets(const int* __restrict__ order, const int* __restrict__ slot_pos, const void* __restrict__ target, int target_is_f32,
                                                                   int64_t n, int* __restrict__ tp) {
  const int64_t q = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (q >= n) return;
  const unsigned k = (unsigned)slot_pos[q];
  int t = 0;
  if (k < (unsigned long long)n) {
    const unsigned flat = (unsigned)order[k];
    if (flat < (unsigned long long)n) t = target_is_f32 ? (reinterpret_cast<const float*>(target)[flat] != 0.f) : (reinterpret_cast<const int*>(target)[flat] != 0);
  }
  tp[q] = t;
}
// slot q = i * N + r is the (r + 1)-th element of row i: after it the row's precision is tp / (r + 1) and its recall tp / (T_i + 1e-10).  The increments over
// the row's previous element and the "row started" flag go to the element's global position.
__global__ void __launch_bounds__(MT_THREADS) k_metrics_f1_increments(const int* __restrict__ tp, const int* __restrict__ slot_pos, int64_t n, int N, double* __restrict__ dP,
                                                                      double* __restrict__ dR, int* __restrict__ started) {
  const int64_t q = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (q >= n) return;
  const int64_t i = q / N;
  const int r = (int)(q - i * N);
  const int t = tp[q], tprev = r > 0 ? tp[q - 1] : 0;
  const double T = (double)tp[i * N + N - 1] + 1e-10;
  const double prec = (double)t / (double)(r + 1), pprev = r > 0 ? (double)tprev / (double)r : 0.0;
  const double rec = (double)t / T, rprev = r > 0 ? (double)tprev / T : 0.0;
  const unsigned k = (unsigned)slot_pos[q];
  if (k < (unsigned long long)n) {
    dP[k] = prec - pprev;
    dR[k] = rec - rprev;
    started[k] = r == 0 ? 1 : 0;
  }
}

// F_k from the running sums; the largest, at equal F the earliest k.  One value per chunk, then one block over the chunks.
__device__ __forceinline__ void f1_better(double& f, long long& k, double of, long long ok) {
  if (of > f || (of == f && ok < k)) { f = of; k = ok; }
}
__device__ __forceinline__ void f1_block_best(double& f, long long& k, double* s_f, long long* s_k) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double of = __shfl_xor(f, o, 64);
    const long long ok = __shfl_xor(k, o, 64);
    f1_better(f, k, of, ok);
  }
  if (lane == 0) { s_f[wave] = f; s_k[wave] = k; }
  __syncthreads();
  f = s_f[0];
  k = s_k[0];
#pragma unroll
  for (int w = 1; w < MT_THREADS / 64; ++w) f1_better(f, k, s_f[w], s_k[w]);
}
__global__ void __launch_bounds__(MT_THREADS) k_metrics_f1_best_partial(const double* __restrict__ sP, const double* __restrict__ sR, const int* __restrict__ nstart, int64_t n, int B,
                                                                        double* __restrict__ pf, long long* __restrict__ pk) {
  __shared__ double s_f[MT_THREADS / 64];
  __shared__ long long s_k[MT_THREADS / 64];
  double f = -1.0;
  long long kb = 0x7fffffffffffffffLL;
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const int64_t k = base + (int64_t)j * MT_THREADS;
    if (k < n) {
      const double P = sP[k] / (double)nstart[k], R = sR[k] / (double)B;
      f1_better(f, kb, 2.0 * P * R / (P + R + 1e-10), k);
    }
  }
  f1_block_best(f, kb, s_f, s_k);
  if (threadIdx.x == 0) { pf[blockIdx.x] = f; pk[blockIdx.x] = kb; }
}
__global__ void __launch_bounds__(MT_THREADS) k_metrics_f1_best_final(const double* __restrict__ pf, const long long* __restrict__ pk, int64_t chunks, const float* __restrict__ pred,
                                                                      const int* __restrict__ order, int64_t n, double* __restrict__ out) {
  __shared__ double s_f[MT_THREADS / 64];
  __shared__ long long s_k[MT_THREADS / 64];
  double f = -1.0;
  long long kb = 0x7fffffffffffffffLL;
  for (int64_t c = threadIdx.x; c < chunks; c += MT_THREADS) f1_better(f, kb, pf[c], pk[c]);
  f1_block_best(f, kb, s_f, s_k);
  if (threadIdx.x == 0) {
    out[0] = f;
    double score = 0.0;
    if (kb >= 0 && kb < n) {
      const unsigned flat = (unsigned)order[kb];
      if (flat < (unsigned long long)n) score = (double)pred[flat];
    }
    out[1] = score;
  }
}

struct F1Ws { SortWs sort; int* order; int* row; int* slot_pos; int* tp; int* started; double* dP; double* dR; double* pf; long long* pk; char* scan_ws; };
static size_t f1_layout(int64_t n, char* base, F1Ws* w) {
  size_t off = sort_layout(n, base, w ? &w->sort : nullptr);
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
  const int64_t chunks = cdiv(n, SCAN_TILE);
  char* o = take((size_t)n * 4); char* rw = take((size_t)n * 4); char* sp = take((size_t)n * 4); char* tp = take((size_t)n * 4); char* stt = take((size_t)n * 4);
  char* dp = take((size_t)n * 8); char* dr = take((size_t)n * 8); char* pf = take((size_t)chunks * 8); char* pk = take((size_t)chunks * 8);
  char* sw = take(scan_ws_bytes(n) + 256);
  if (w) { w->order = (int*)o; w->row = (int*)rw; w->slot_pos = (int*)sp; w->tp = (int*)tp; w->started = (int*)stt; w->dP = (double*)dp; w->dR = (double*)dr;
           w->pf = (double*)pf; w->pk = (long long*)pk; w->scan_ws = sw; }
  return off;
}

extern "C" size_t oneprot_f1max_workspace(int B, int N) {
  if (B < 1 || N < 1 || (int64_t)B * N > METRICS_MAX_N) return 0;
  return f1_layout((int64_t)B * N, nullptr, nullptr);
}

extern "C" int oneprot_f1max(const float* pred, const void* target, int target_is_f32, int B, int N, void* f1_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (!pred || !target || !f1_bytes || !workspace || B < 1 || N < 1 || (int64_t)B * N > METRICS_MAX_N || (target_is_f32 != 0 && target_is_f32 != 1)) return OP_EINVAL;
  if (workspace_bytes < oneprot_f1max_workspace(B, N) || ((uintptr_t)workspace & 7) || ((uintptr_t)f1_bytes & 7)) return OP_EINVAL;
  const int64_t n = (int64_t)B * N;
  F1Ws w;
  f1_layout(n, (char*)workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(n, MT_THREADS)), blk(MT_THREADS);
  sort_run(KM_F32_DESC, pred, nullptr, n, 4, nullptr, w.order, w.sort, st);
  int bits = 0;
  while (((int64_t)1 << bits) < B) ++bits;
  if (bits == 0) {
    hipLaunchKernelGGL(k_metrics_copy_pairs, grid, blk, 0, st, (const int*)w.order, (const int*)nullptr, n, (int*)nullptr, w.slot_pos);      // one row: slot = position
  } else {
    hipLaunchKernelGGL(k_metrics_f1_rows, grid, blk, 0, st, (const int*)w.order, n, N, w.row);
    sort_run(KM_RAW, w.row, nullptr, n, (bits + 7) / 8, nullptr, w.slot_pos, w.sort, st);
  }
  hipLaunchKernelGGL(k_metrics_f1_targets, grid, blk, 0, st, (const int*)w.order, (const int*)w.slot_pos, target, target_is_f32, n, w.tp);
  scan_run<int, SC_ADD, false>((const int*)w.tp, w.tp, n, (int64_t)N, w.scan_ws, st);
  hipLaunchKernelGGL(k_metrics_f1_increments, grid, blk, 0, st, (const int*)w.tp, (const int*)w.slot_pos, n, N, w.dP, w.dR, w.started);
  scan_run<double, SC_ADD, false>((const double*)w.dP, w.dP, n, 0, w.scan_ws, st);
  scan_run<double, SC_ADD, false>((const double*)w.dR, w.dR, n, 0, w.scan_ws, st);
  scan_run<int, SC_ADD, false>((const int*)w.started, w.started, n, 0, w.scan_ws, st);
  const int64_t chunks = cdiv(n, SCAN_TILE);
  hipLaunchKernelGGL(k_metrics_f1_best_partial, dim3((unsigned)chunks), blk, 0, st, (const double*)w.dP, (const double*)w.dR, (const int*)w.started, n, B, w.pf, w.pk);
  hipLaunchKernelGGL(k_metrics_f1_best_final, dim3(1), blk, 0, st, (const double*)w.pf, (const long long*)w.pk, chunks, pred, (const int*)w.order, n, (double*)f1_bytes);
  return launch_status();
}
