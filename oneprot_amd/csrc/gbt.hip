// Gradient-boosted tree probes (ref src/saprot_fit_cls.py:32-38, src/saprot_fit_reg.py:26-32: xgboost.XGBClassifier / XGBRegressor with tree_method gpu_hist,
// configs/downstream_model/xgboost_{cls,reg}.yaml): the `hist` tree builder of Chen & Guestrin 2016 on fixed-point histograms.  Stages: quantile cuts, uint8
// bins, quantised gradients, per-(output, node, feature, bin) integer histograms, split search in fp64, row partition, margin update and the ensemble walk.
//
// Determinism: gradients are quantised to integers (q = rint(x 2^(GBT_FRAC - e))) before they are summed, histograms are int32 in LDS and int64 in global
// memory, and integer addition is associative -- so the integer atomics below give the same bits in every run and for every work decomposition.  There is no
// float atomic, no work-group waits on another, and nothing is read back.
//
// GBT_FRAC = 20: |g| <= 1 (logistic, softmax) or |g| < 2^e (regression), h <= 1, so |q| <= 2^20.  A work-group of the histogram kernel adds at most GBT_ROWS =
// 2047 rows into one int32 LDS counter (2047 x 2^20 < 2^31) before it flushes to global int64, where 2^24 rows x 2^20 = 2^44 is far from 2^63.
//
// LDS tile of the histogram kernel: 64 (node, feature) slots x max_bin bins x {g, h} x int32 = 128 KB at max_bin 256, of the CU's 160 KB: one work-group of
// sixteen waves per CU.  Level d has 2^d nodes, so a tile holds 64 >> d features of every node of the level; a wave's 64 lanes read 64 >> d consecutive
// feature bytes of 2^d rows, and their LDS adds land in different features' (or nodes') bins.
//
// Levels 6 .. 8 (max_depth 7 .. 9, one output: XGBRegressor) have more nodes than the tile has slots, and at 1,280 features and 256 bins more bytes than the
// histogram budget.  There the rows are put in node order once per level (k_gbt_node_keys -> the stable radix sort of metrics.hip -> k_gbt_node_seg), and
// k_gbt_hist_nodes builds a group of nodes at a time: a work-group takes a run of GBT_ROWS consecutive positions of the order and walks the consecutive
// nodes it meets, nt nodes x ft features (nt ft = 64) in the same LDS tile with the same int32 atomics, flushing whenever it leaves the tile's node span -- so
// the bound of GBT_ROWS rows per counter between two flushes holds as before, and a larger node is the sum of several work-groups' flushes.  The split search
// of a group is the two kernels of a level with a node offset (one body each, two launchers); partition, update and predict know no level limit but the
// tree's size.  The rule is the same at every depth; levels 0 .. 5 run the kernels and launches they always ran.
#include "philox.h"
#include "../../include/oneprot_hip.h"

#define GBT_FRAC 20
#define GBT_ROWS 2047
#define GBT_HIST_THREADS 1024    // the LDS tile admits one work-group per CU: sixteen waves share it, so that the CU has loads in flight while others add
#define GBT_MAX_LEVEL 5          // levels 0 .. 5 (max_depth <= 6) are histogrammed by k_gbt_hist, which keeps every node of a level in one LDS tile
#define GBT_DEEP_MAX_LEVEL 8     // levels 6 .. 8 (max_depth 7 .. 9, one output) are histogrammed by k_gbt_hist_nodes over the rows in node order, a node group at a time
#define GBT_TILE_LOG2_L6 3       // features of a k_gbt_hist_nodes tile at levels 6, 7, 8 (log2): 8 features x 8 nodes, the fastest of the seven shapes at every
#define GBT_TILE_LOG2_L7 3       // one of the three levels
#define GBT_TILE_LOG2_L8 3
typedef unsigned long long ull_t;
typedef long long ll_t;
enum { GO_LOGISTIC = 0, GO_SQUARED = 1, GO_SOFTMAX = 2 };

static inline unsigned gbt_grid(int64_t n) { return (unsigned)((n + 255) / 256 < 1048576 ? (n + 255) / 256 : 1048576); }

// ---------------------------------------------------------------------------------------------------------------------------------
// cuts: grouped [F, N] holds every feature's column in ascending order.  Candidates v[floor(k N / B)], k = 1 .. B-1, -0.0 read as +0.0; the distinct ones,
// ascending, are the cuts.  One thread per feature (B - 1 <= 255 reads).  Unused slots of cuts [F, B-1] are +inf.
__global__ void __launch_bounds__(256) k_gbt_cuts(const float* __restrict__ grouped, int64_t N, int F, int B, float* __restrict__ cuts, int* __restrict__ ncuts) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const float* v = grouped + (size_t)f * N;
  float* c = cuts + (size_t)f * (B - 1);
  int n = 0;
  float last = 0.f;
  for (int k = 1; k < B; ++k) {
    const float x = v[(int64_t)k * N / B] + 0.0f;
    if (n == 0 || x != last) { c[n++] = x; last = x; }
  }
  ncuts[f] = n;
  for (int k = n; k < B - 1; ++k) c[k] = __builtin_inff();
}

// bin(x) = number of cuts <= x (binary search over the feature's ascending cuts); lanes run along the features of a row
__global__ void __launch_bounds__(256) k_gbt_bin(const float* __restrict__ X, const float* __restrict__ cuts, const int* __restrict__ ncuts, unsigned char* __restrict__ bins,
                                                 int64_t total, int F, int B) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int f = (int)(e % F);
    const float x = X[e];
    const float* c = cuts + (size_t)f * (B - 1);
    int lo = 0, hi = ncuts[f];                                // first index with c[idx] > x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (c[mid] <= x) lo = mid + 1; else hi = mid;
    }
    bins[e] = (unsigned char)lo;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sampling: the uniform of element e is its 16-bit slice under philox.h.  Row i is kept iff its uniform slice / 65536 < rate; the features with the n_keep smallest uniforms are kept, equal uniforms to the lower index
__global__ void __launch_bounds__(256) k_gbt_row_keep(unsigned char* __restrict__ keep, int64_t N, float rate, ull_t seed, ull_t stream_id) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
    keep[i] = rate >= 1.0f ? 1 : ((float)philox_slice16((size_t)i, seed, stream_id) < rate * 65536.0f ? 1 : 0);
}
__global__ void __launch_bounds__(256) k_gbt_feat_uniform(int* __restrict__ u, int F, ull_t seed, ull_t stream_id) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f < F) u[f] = (int)philox_slice16((size_t)f, seed, stream_id);
}
__global__ void __launch_bounds__(256) k_gbt_feat_keep(const int* __restrict__ u, unsigned char* __restrict__ keep, int F, int n_keep) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int mine = u[f];
  int rank = 0;
  for (int o = 0; o < F; ++o) {
    const int v = u[o];
    rank += (v < mine || (v == mine && o < f)) ? 1 : 0;
  }
  keep[f] = rank < n_keep ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gradients in fp32 from the fp32 margin [N, K]; quantised q = rint(x 2^(GBT_FRAC - e)) into gq / hq [K, N].  e = 0 except for the g of reg:squarederror, where
// it is the smallest integer with max |g| < 2^e over the kept rows (k_gbt_gmax: the maximum of non-negative floats through an integer atomicMax of their
// bits -- order-free, so the same in every run); h is always quantised with e = 0.  Dropped rows get q = 0: they add nothing anywhere.
__global__ void __launch_bounds__(256) k_gbt_gmax(const float* __restrict__ m, const float* __restrict__ y, const unsigned char* __restrict__ keep, int* __restrict__ gmax_bits,
                                                  int64_t N) {
  float mx = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
    if (keep[i]) mx = fmaxf(mx, fabsf(m[i] - y[i]));
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) atomicMax(gmax_bits, __builtin_bit_cast(int, mx));
}
__device__ __forceinline__ int gbt_expo_of(int gmax_bits) {
  const float mx = __builtin_bit_cast(float, gmax_bits);
  if (!(mx > 0.f)) return 0;
  int ex;
  frexpf(mx, &ex);                                            // mx = m 2^ex, m in [0.5, 1): 2^(ex-1) <= mx < 2^ex
  return ex < -100 ? -100 : ex;
}
__device__ __forceinline__ int gbt_quant(float x, int shift) { return (int)rintf(ldexpf(x, shift)); }

__global__ void __launch_bounds__(256) k_gbt_grad(const float* __restrict__ m, const float* __restrict__ y, const int* __restrict__ labels,
                                                  const unsigned char* __restrict__ keep, int* __restrict__ gq, int* __restrict__ hq, int* __restrict__ expo,
                                                  const int* __restrict__ gmax_bits, int64_t N, int K, int objective) {
  if (objective == GO_SOFTMAX) {
    if (blockIdx.x == 0) for (int k = threadIdx.x; k < K; k += 256) expo[k] = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
      const float* mi = m + (size_t)i * K;
      const bool kept = keep[i] != 0;
      float mx = mi[0];
      for (int k = 1; k < K; ++k) mx = fmaxf(mx, mi[k]);
      float sum = 0.f;
      for (int k = 0; k < K; ++k) sum += expf(mi[k] - mx);
      const int lab = labels[i];
      for (int k = 0; k < K; ++k) {
        const float p = expf(mi[k] - mx) / sum;
        const float g = p - (k == lab ? 1.0f : 0.0f), h = 2.0f * p * (1.0f - p);
        gq[(size_t)k * N + i] = kept ? gbt_quant(g, GBT_FRAC) : 0;
        hq[(size_t)k * N + i] = kept ? gbt_quant(h, GBT_FRAC) : 0;
      }
    }
    return;
  }
  const int e = objective == GO_SQUARED ? gbt_expo_of(gmax_bits[0]) : 0;
  if (blockIdx.x == 0) for (int k = threadIdx.x; k < K; k += 256) expo[k] = e;
  const int64_t total = N * K;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t i = t / K;
    const int k = (int)(t - i * K);
    float g, h;
    if (objective == GO_SQUARED) {
      g = m[t] - y[t];
      h = 1.0f;
    } else {
      const float p = 1.0f / (1.0f + expf(-m[t]));
      g = p - y[t];
      h = p * (1.0f - p);
    }
    const bool kept = keep[i] != 0;
    gq[(size_t)k * N + i] = kept ? gbt_quant(g, GBT_FRAC - e) : 0;
    hq[(size_t)k * N + i] = kept ? gbt_quant(h, GBT_FRAC) : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// hist: the hot kernel.  Work-group (x, y, z) = row chunks x, x + gridDim.x, ... of GBT_ROWS rows (a chunk is flushed before the next begins), features [y ft, +ft) with ft = 64 >> level, output z of the chunk.  LDS counters
// [node 2^level][ft][B][2] int32, flushed (non-zero counters only) with int64 global atomics into hist [kc, 2^level, F, B, 2].
__global__ void __launch_bounds__(GBT_HIST_THREADS) k_gbt_hist(const unsigned char* __restrict__ bins, const int* __restrict__ gq, const int* __restrict__ hq, const int* __restrict__ pos,
                                                  ll_t* __restrict__ hist, int64_t N, int F, int B, int level) {
  extern __shared__ int lds[];
  const int tid = threadIdx.x;
  const int L = 1 << level, ft = 64 >> level, base = L - 1;
  const int entries = 128 * B;                                // L * ft * B * 2
  for (int e = tid; e < entries; e += GBT_HIST_THREADS) lds[e] = 0;
  __syncthreads();
  const int kk = blockIdx.z, f0 = blockIdx.y * ft;
  const int fi = tid & (ft - 1), rs = tid >> (6 - level), rstep = (GBT_HIST_THREADS / 64) << level;
  const int f = f0 + fi;
  const size_t ko = (size_t)kk * N;
  const int64_t nchunks = (N + GBT_ROWS - 1) / GBT_ROWS;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {      // (one chunk per work-group unless the grid was capped: the same trips for every thread)
    const int64_t r0 = chunk * GBT_ROWS, r1 = r0 + GBT_ROWS < N ? r0 + GBT_ROWS : N;
    if (f < F) {
      for (int64_t r = r0 + rs; r < r1; r += rstep) {
        const int p = pos[ko + r] - base;
        if ((unsigned)p >= (unsigned)L) continue;
        const int g = gq[ko + r], h = hq[ko + r];
        if ((g | h) == 0) continue;
        const int b = bins[(size_t)r * F + f];
        if (b >= B) continue;
        const int idx = ((p * ft + fi) * B + b) * 2;
        if (g) atomicAdd(&lds[idx], g);
        if (h) atomicAdd(&lds[idx + 1], h);
      }
    }
    __syncthreads();
    for (int e = tid; e < entries; e += GBT_HIST_THREADS) {
      const int v = lds[e];
      if (v == 0) continue;
      lds[e] = 0;                                                // ready for the next chunk
      const int c = e & 1, b = (e >> 1) % B, slot = (e >> 1) / B;
      const int ff = f0 + (slot & (ft - 1)), p = slot >> (6 - level);
      if (ff >= F) continue;
      atomicAdd((ull_t*)(hist + ((((size_t)kk * L + p) * F + ff) * B + b) * 2 + c), (ull_t)(ll_t)v);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// levels 6 .. 8 (K = 1): the rows in node order.  key = node of the level, or the sentinel 2^level for a row that stopped at a shallower leaf; the stable radix
// sort of csrc/metrics.hip orders the rows by key; seg [2^level + 1] holds each node's lower bound in the sorted keys (seg[2^level]: where the sentinels begin).
__global__ void __launch_bounds__(256) k_gbt_node_keys(const int* __restrict__ pos, int* __restrict__ keys, int64_t N, int level) {
  const int L = 1 << level;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int p = pos[i] - (L - 1);
    keys[i] = (unsigned)p < (unsigned)L ? p : L;
  }
}
__global__ void __launch_bounds__(256) k_gbt_node_seg(const int* __restrict__ skeys, int* __restrict__ seg, int64_t N, int level) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n > (1 << level)) return;
  int64_t lo = 0, hi = N;                                      // first position with skeys[position] >= n
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (skeys[mid] < n) lo = mid + 1; else hi = mid;
  }
  seg[n] = (int)lo;
}

// hist of a node group [node0, node0 + nodes) of a deep level.  Work-group (x, y) = run x of GBT_ROWS consecutive positions of `order`, feature tiles y, y + gridDim.y, ...
// of ft = 2^ftl features: the grid is a function of the shapes alone.  The LDS tile is k_gbt_hist's, [nt][ft][B][2] int32 with nt ft = 64: the work-group walks the
// spans of nt consecutive nodes that its run meets (found through seg, clipped to the run), adds the span's rows, and flushes the non-zero counters with int64
// global atomics before the next span and at the end -- so a counter never takes more than GBT_ROWS rows between two flushes, and a node larger than a run is
// the sum of several work-groups' flushes.  Rows of nodes outside the group, sentinel rows, rows with g = h = 0 and bins >= B add nothing; a run that lies
// wholly outside the group returns after reading its first and last key.  Every index read from device memory (seg, keys, order, bins) is checked before it
// addresses anything.
__global__ void __launch_bounds__(GBT_HIST_THREADS) k_gbt_hist_nodes(const unsigned char* __restrict__ bins, const int* __restrict__ gq, const int* __restrict__ hq,
                                                        const int* __restrict__ order, const int* __restrict__ skeys, const int* __restrict__ seg, ll_t* __restrict__ hist,
                                                        int64_t N, int F, int B, int level, int node0, int nodes, int ftl) {
  extern __shared__ int lds[];
  const int tid = threadIdx.x;
  const int L = 1 << level, ft = 1 << ftl, ntl = 6 - ftl, nt = 1 << ntl;
  const int64_t p0 = (int64_t)blockIdx.x * GBT_ROWS, p1 = p0 + GBT_ROWS < N ? p0 + GBT_ROWS : N;
  if (p0 >= p1) return;
  const int kfirst = skeys[p0], klast = skeys[p1 - 1];
  const int lo = kfirst > node0 ? kfirst : node0, hi = klast < node0 + nodes - 1 ? klast : node0 + nodes - 1;      // the group's nodes this run can hold (hi < L: no sentinel)
  if (lo > hi || lo < 0) return;                               // the same for every thread: before any barrier
  const int entries = 128 * B;
  for (int e = tid; e < entries; e += GBT_HIST_THREADS) lds[e] = 0;
  __syncthreads();
  const int fi = tid & (ft - 1), rs = tid >> ftl, rstep = GBT_HIST_THREADS >> ftl;
  const int tiles = (F + ft - 1) >> ftl;
  for (int tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const int f0 = tile << ftl, f = f0 + fi;
    for (int s = lo >> ntl; s <= (hi >> ntl); ++s) {
      const int n0 = s << ntl;                                 // the span's first node; n0 + nt <= L
      int64_t qs = seg[n0], qe = seg[n0 + nt];
      qs = qs > p0 ? qs : p0;
      qe = qe < p1 ? qe : p1;
      if (qs >= qe) continue;                                  // (the same for every thread: seg is read-only here)
      if (f < F) {
        for (int64_t q = qs + rs; q < qe; q += rstep) {
          const int k = skeys[q];
          if ((unsigned)(k - n0) >= (unsigned)nt || (unsigned)(k - node0) >= (unsigned)nodes) continue;
          const int r = order[q];
          if ((unsigned)r >= (unsigned)N) continue;
          const int g = gq[r], h = hq[r];
          if ((g | h) == 0) continue;
          const int b = bins[(size_t)r * F + f];
          if (b >= B) continue;
          const int idx = ((((k - n0) << ftl) + fi) * B + b) * 2;
          if (g) atomicAdd(&lds[idx], g);
          if (h) atomicAdd(&lds[idx + 1], h);
        }
      }
      __syncthreads();
      for (int e = tid; e < entries; e += GBT_HIST_THREADS) {
        const int v = lds[e];
        if (v == 0) continue;
        lds[e] = 0;                                            // ready for the next span
        const int c = e & 1, b = (e >> 1) % B, slot = (e >> 1) / B;
        const int ff = f0 + (slot & (ft - 1)), n = n0 + (slot >> ftl) - node0;          // ff < F and 0 <= n < nodes: only such rows were added
        atomicAdd((ull_t*)(hist + (((size_t)n * F + ff) * B + b) * 2 + c), (ull_t)(ll_t)v);
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// split, in two launches.  The node's totals are the sums over all bins of a feature, the left sums the running prefix.  Gains in fp64 from the int64 sums;
// best = largest gain, then lowest feature, then lowest cut.
__device__ __forceinline__ double gbt_thr(double G, double alpha) {
  const double a = fabs(G) - alpha;
  return a > 0.0 ? (G < 0.0 ? -a : a) : 0.0;
}
__device__ __forceinline__ double gbt_score(double G, double H, double alpha, double lambda) {
  const double t = gbt_thr(G, alpha);
  return t * t / (H + lambda);
}
__device__ __forceinline__ double gbt_weight(double G, double H, double alpha, double lambda) {
  const double d = H + lambda;
  return d > 0.0 ? -gbt_thr(G, alpha) / d : 0.0;
}
struct GbtBest { double gain; int f, j; ll_t GL, HL; };
__device__ __forceinline__ bool gbt_better(const GbtBest& a, const GbtBest& b) {
  if (a.f == 0x7fffffff) return false;
  if (b.f == 0x7fffffff) return true;
  return a.gain > b.gain || (a.gain == b.gain && (a.f < b.f || (a.f == b.f && a.j < b.j)));
}

// stage 1: one wave per (output, node, feature).  Lanes hold the feature's bins in up to four chunks of 64 (16-byte loads of the (g, h) pair, consecutive lanes
// consecutive bins); totals by a wave sum, left sums by a wave scan with the carry of the chunks before, every lane scores its own cuts, and an ordered
// arg-max over the lanes (gain, then lowest cut) leaves the feature's record.  Integer sums and single fp64 operations: the lane layout cannot change a bit.
struct GbtRec { double gain; ll_t GL, HL, G, H; int j, pad; };
__device__ __forceinline__ ll_t gbt_wave_sum(ll_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ ll_t gbt_wave_scan(ll_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const ll_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
// (the body is shared by the launch of a whole level, LH = 2^level nodes per output, and the launch of a node group of a deep level, LH = the group's nodes)
__device__ __forceinline__ void gbt_split_scan_body(const ll_t* __restrict__ hist, const int* __restrict__ ncuts, const unsigned char* __restrict__ feat_keep,
                                                    const int* __restrict__ expo, GbtRec* __restrict__ rec, int F, int B, int LH, double mcw, double alpha, double lambda) {
  const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6), node = blockIdx.y, kk = blockIdx.z;
  if (f >= F) return;                                          // a whole wave; the kernel has no work-group barrier
  const size_t slot = ((size_t)kk * LH + node) * F + f;
  const ll_t* Hf = hist + slot * B * 2;
  const int nc = ncuts[f];
  const double sg = ldexp(1.0, expo[kk] - GBT_FRAC), sh = ldexp(1.0, -GBT_FRAC);
  ll_t g[4], h[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int b = c * 64 + lane;
    const bool in = b <= nc && b < B;
    g[c] = in ? Hf[2 * b] : 0;
    h[c] = in ? Hf[2 * b + 1] : 0;
  }
  const ll_t G = gbt_wave_sum((g[0] + g[1]) + (g[2] + g[3])), H = gbt_wave_sum((h[0] + h[1]) + (h[2] + h[3]));
  GbtBest best = {0.0, 0x7fffffff, 0x7fffffff, 0, 0};
  if (feat_keep[f] && H > 0) {
    const double sN = gbt_score((double)G * sg, (double)H * sh, alpha, lambda);
    ll_t cg = 0, ch = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c * 64 < nc) {                                       // wave-uniform
        const ll_t GL = cg + gbt_wave_scan(g[c], lane), HL = ch + gbt_wave_scan(h[c], lane);
        cg = __shfl(GL, 63, 64);
        ch = __shfl(HL, 63, 64);
        const int j = c * 64 + lane;
        const ll_t HR = H - HL;
        if (j < nc && HL > 0 && HR > 0) {
          const double HLd = (double)HL * sh, HRd = (double)HR * sh;
          if (HLd >= mcw && HRd >= mcw) {
            const double sL = gbt_score((double)GL * sg, HLd, alpha, lambda), sR = gbt_score((double)(G - GL) * sg, HRd, alpha, lambda);
            const GbtBest cand = {(sL + sR) - sN, f, j, GL, HL};
            if (gbt_better(cand, best)) best = cand;
          }
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const GbtBest other = {__shfl_xor(best.gain, o, 64), __shfl_xor(best.f, o, 64), __shfl_xor(best.j, o, 64), __shfl_xor(best.GL, o, 64), __shfl_xor(best.HL, o, 64)};
      if (gbt_better(other, best)) best = other;
    }
  }
  if (lane == 0) {
    GbtRec r;
    r.gain = best.gain; r.GL = best.GL; r.HL = best.HL; r.G = G; r.H = H; r.j = best.f == 0x7fffffff ? -1 : best.j; r.pad = 0;
    rec[slot] = r;
  }
}
__global__ void __launch_bounds__(256) k_gbt_split_scan(const ll_t* __restrict__ hist, const int* __restrict__ ncuts, const unsigned char* __restrict__ feat_keep,
                                                        const int* __restrict__ expo, GbtRec* __restrict__ rec, int F, int B, int level, double mcw, double alpha, double lambda) {
  gbt_split_scan_body(hist, ncuts, feat_keep, expo, rec, F, B, 1 << level, mcw, alpha, lambda);
}
__global__ void __launch_bounds__(256) k_gbt_split_scan_nodes(const ll_t* __restrict__ hist, const int* __restrict__ ncuts, const unsigned char* __restrict__ feat_keep,
                                                              const int* __restrict__ expo, GbtRec* __restrict__ rec, int F, int B, int nodes, double mcw, double alpha, double lambda) {
  gbt_split_scan_body(hist, ncuts, feat_keep, expo, rec, F, B, nodes, mcw, alpha, lambda);
}

// stage 2: one work-group per (output, node): the ordered arg-max over the features' records (gain, then lowest feature, then lowest cut), and the node's entries
// (LH: the nodes per output of rec; nid0: the heap id of rec's node 0 -- 2^level - 1 for a whole level, 2^level - 1 + node0 for a node group)
__device__ __forceinline__ void gbt_split_body(const GbtRec* __restrict__ rec, const float* __restrict__ cuts, const int* __restrict__ expo, int* __restrict__ tree_feat,
                                               int* __restrict__ tree_bin, float* __restrict__ tree_thr, float* __restrict__ tree_leaf, double* __restrict__ gain_out, int F, int B,
                                               int LH, int nid0, int NN, double gamma, double alpha, double lambda, double lr) {
  __shared__ double s_gain[256];
  __shared__ int s_f[256], s_j[256];
  __shared__ ll_t s_GL[256], s_HL[256];
  const int tid = threadIdx.x, node = blockIdx.x, kk = blockIdx.y;
  const GbtRec* R = rec + ((size_t)kk * LH + node) * F;
  const double sg = ldexp(1.0, expo[kk] - GBT_FRAC), sh = ldexp(1.0, -GBT_FRAC);
  GbtBest best = {0.0, 0x7fffffff, 0x7fffffff, 0, 0};
  for (int f = tid; f < F; f += 256) {
    const GbtRec r = R[f];
    if (r.j < 0) continue;
    const GbtBest cand = {r.gain, f, r.j, r.GL, r.HL};
    if (gbt_better(cand, best)) best = cand;
  }
  s_gain[tid] = best.gain; s_f[tid] = best.f; s_j[tid] = best.j; s_GL[tid] = best.GL; s_HL[tid] = best.HL;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const GbtBest a = {s_gain[tid], s_f[tid], s_j[tid], s_GL[tid], s_HL[tid]}, b = {s_gain[tid + o], s_f[tid + o], s_j[tid + o], s_GL[tid + o], s_HL[tid + o]};
      if (gbt_better(b, a)) { s_gain[tid] = b.gain; s_f[tid] = b.f; s_j[tid] = b.j; s_GL[tid] = b.GL; s_HL[tid] = b.HL; }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  best.gain = s_gain[0]; best.f = s_f[0]; best.j = s_j[0]; best.GL = s_GL[0]; best.HL = s_HL[0];
  const bool valid = best.f != 0x7fffffff;
  const ll_t G = R[0].G, H = R[0].H;                           // the node's totals: every row is in exactly one bin of every feature
  const size_t o = (size_t)kk * NN;
  const int nid = nid0 + node, lc = 2 * nid + 1;
  const bool split = valid && best.gain > (gamma > 0.0 ? gamma : 0.0);
  if (gain_out) gain_out[o + nid] = valid ? best.gain : -__builtin_inf();
  tree_leaf[o + nid] = (float)(lr * gbt_weight((double)G * sg, (double)H * sh, alpha, lambda));
  if (split) {
    tree_feat[o + nid] = best.f; tree_bin[o + nid] = best.j; tree_thr[o + nid] = cuts[(size_t)best.f * (B - 1) + best.j];
    tree_feat[o + lc] = -1; tree_feat[o + lc + 1] = -1;
    tree_leaf[o + lc] = (float)(lr * gbt_weight((double)best.GL * sg, (double)best.HL * sh, alpha, lambda));
    tree_leaf[o + lc + 1] = (float)(lr * gbt_weight((double)(G - best.GL) * sg, (double)(H - best.HL) * sh, alpha, lambda));
  } else {
    tree_feat[o + nid] = -1; tree_bin[o + nid] = 0; tree_thr[o + nid] = 0.f;
    tree_feat[o + lc] = -1; tree_feat[o + lc + 1] = -1; tree_leaf[o + lc] = 0.f; tree_leaf[o + lc + 1] = 0.f;
  }
}
__global__ void __launch_bounds__(256) k_gbt_split(const GbtRec* __restrict__ rec, const float* __restrict__ cuts, const int* __restrict__ expo, int* __restrict__ tree_feat,
                                                   int* __restrict__ tree_bin, float* __restrict__ tree_thr, float* __restrict__ tree_leaf, double* __restrict__ gain_out, int F, int B,
                                                   int level, int NN, double gamma, double alpha, double lambda, double lr) {
  gbt_split_body(rec, cuts, expo, tree_feat, tree_bin, tree_thr, tree_leaf, gain_out, F, B, 1 << level, (1 << level) - 1, NN, gamma, alpha, lambda, lr);
}
__global__ void __launch_bounds__(256) k_gbt_split_nodes(const GbtRec* __restrict__ rec, const float* __restrict__ cuts, const int* __restrict__ expo, int* __restrict__ tree_feat,
                                                         int* __restrict__ tree_bin, float* __restrict__ tree_thr, float* __restrict__ tree_leaf, double* __restrict__ gain_out, int F, int B,
                                                         int nodes, int nid0, int NN, double gamma, double alpha, double lambda, double lr) {
  gbt_split_body(rec, cuts, expo, tree_feat, tree_bin, tree_thr, tree_leaf, gain_out, F, B, nodes, nid0, NN, gamma, alpha, lambda, lr);
}

// partition: a row in a node of this level that split moves to the left child iff bin <= cut index
__global__ void __launch_bounds__(256) k_gbt_partition(const unsigned char* __restrict__ bins, const int* __restrict__ tree_feat, const int* __restrict__ tree_bin, int* __restrict__ pos,
                                                       int64_t N, int F, int level, int NN) {
  const int kk = blockIdx.y, L = 1 << level;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int p = pos[(size_t)kk * N + i];
    if ((unsigned)(p - (L - 1)) >= (unsigned)L) continue;
    const int f = tree_feat[(size_t)kk * NN + p];
    if (f < 0 || f >= F) continue;
    pos[(size_t)kk * N + i] = 2 * p + 1 + ((int)bins[(size_t)i * F + f] <= tree_bin[(size_t)kk * NN + p] ? 0 : 1);
  }
}

// leaf: margin[i, k0 + kk] += leaf value of the node row i ended in (every row, kept or dropped)
__global__ void __launch_bounds__(256) k_gbt_update(float* __restrict__ margin, const int* __restrict__ pos, const float* __restrict__ tree_leaf, int64_t N, int K, int k0, int NN) {
  const int kk = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int p = pos[(size_t)kk * N + i];
    if ((unsigned)p < (unsigned)NN) margin[(size_t)i * K + k0 + kk] += tree_leaf[(size_t)kk * NN + p];
  }
}

// predict: the ensemble walk on raw fp32 rows, x < threshold goes left; one fp32 chain per (row, output) in round order
__global__ void __launch_bounds__(256) k_gbt_predict(const float* __restrict__ X, const int* __restrict__ tree_feat, const float* __restrict__ tree_thr,
                                                     const float* __restrict__ tree_leaf, float* __restrict__ margin, int64_t N, int F, int K, int T, int NN, float init) {
  const int64_t total = N * K;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / K;
    const int k = (int)(e - i * K);
    const float* x = X + (size_t)i * F;
    float m = init;
    for (int t = 0; t < T; ++t) {
      const size_t o = ((size_t)t * K + k) * NN;
      int p = 0;
      for (;;) {
        const int f = tree_feat[o + p];
        if (f < 0 || f >= F || 2 * p + 2 >= NN) break;
        p = 2 * p + 1 + (x[f] < tree_thr[o + p] ? 0 : 1);
      }
      m += tree_leaf[o + p];
    }
    margin[e] = m;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static bool gbt_shape(int64_t N, int F, int B) { return N >= 1 && N <= (1 << 24) && F >= 1 && F <= 65535 && B >= 2 && B <= 256; }

extern "C" int oneprot_gbt_cuts(const float* grouped, int64_t N, int F, int max_bin, float* cuts, int* ncuts, void* stream) {
  if (!grouped || !cuts || !ncuts || !gbt_shape(N, F, max_bin)) return OP_EINVAL;
  hipLaunchKernelGGL(k_gbt_cuts, dim3((F + 255) / 256), dim3(256), 0, (hipStream_t)stream, grouped, N, F, max_bin, cuts, ncuts);
  return launch_status();
}

extern "C" int oneprot_gbt_bin(const float* X, const float* cuts, const int* ncuts, void* bins, int64_t N, int F, int max_bin, void* stream) {
  if (!X || !cuts || !ncuts || !bins || !gbt_shape(N, F, max_bin)) return OP_EINVAL;
  const int64_t total = N * F;
  hipLaunchKernelGGL(k_gbt_bin, dim3(gbt_grid(total)), dim3(256), 0, (hipStream_t)stream, X, cuts, ncuts, (unsigned char*)bins, total, F, max_bin);
  return launch_status();
}

extern "C" int oneprot_gbt_sample(void* row_keep, void* feat_keep, int* feat_uniform, int64_t N, int F, float subsample, int n_keep, uint64_t seed, uint64_t row_stream,
                                  uint64_t feat_stream, void* stream) {
  if (!row_keep || !feat_keep || !feat_uniform || !gbt_shape(N, F, 2) || !(subsample > 0.f) || n_keep < 1 || n_keep > F) return OP_EINVAL;
  hipLaunchKernelGGL(k_gbt_row_keep, dim3(gbt_grid(N)), dim3(256), 0, (hipStream_t)stream, (unsigned char*)row_keep, N, subsample, (ull_t)seed, (ull_t)row_stream);
  if (n_keep == F) {
    if (hipMemsetAsync(feat_keep, 1, (size_t)F, (hipStream_t)stream) != hipSuccess) return OP_ELAUNCH;
  } else {
    hipLaunchKernelGGL(k_gbt_feat_uniform, dim3((F + 255) / 256), dim3(256), 0, (hipStream_t)stream, feat_uniform, F, (ull_t)seed, (ull_t)feat_stream);
    hipLaunchKernelGGL(k_gbt_feat_keep, dim3((F + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int*)feat_uniform, (unsigned char*)feat_keep, F, n_keep);
  }
  return launch_status();
}

extern "C" int oneprot_gbt_grad(const float* margin, const float* target, const int* labels, const void* row_keep, int* gq, int* hq, int* expo, int* gmax_bits, int64_t N,
                                int K, int objective, void* stream) {
  if (!margin || !row_keep || !gq || !hq || !expo || !gmax_bits || N < 1 || N > (1 << 24) || K < 1 || K > 65535) return OP_EINVAL;
  if (objective == GO_SOFTMAX ? !labels : !target) return OP_EINVAL;
  if (objective < 0 || objective > GO_SOFTMAX || (objective == GO_SQUARED && K != 1)) return OP_EINVAL;
  if (objective == GO_SQUARED) {
    if (hipMemsetAsync(gmax_bits, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) return OP_ELAUNCH;
    hipLaunchKernelGGL(k_gbt_gmax, dim3(gbt_grid(N) < 1024 ? gbt_grid(N) : 1024), dim3(256), 0, (hipStream_t)stream, margin, target, (const unsigned char*)row_keep, gmax_bits, N);
  }
  const int64_t work = objective == GO_SOFTMAX ? N : N * K;
  hipLaunchKernelGGL(k_gbt_grad, dim3(gbt_grid(work)), dim3(256), 0, (hipStream_t)stream, margin, target, labels, (const unsigned char*)row_keep, gq, hq, expo,
                     (const int*)gmax_bits, N, K, objective);
  return launch_status();
}

extern "C" size_t oneprot_gbt_hist_bytes(int F, int max_bin, int level) {
  if (F < 1 || F > 65535 || max_bin < 2 || max_bin > 256 || level < 0 || level > GBT_MAX_LEVEL) return 0;
  return ((size_t)1 << level) * (size_t)F * (size_t)max_bin * 2 * sizeof(int64_t);
}

extern "C" int oneprot_gbt_hist(const void* bins, const int* gq, const int* hq, const int* pos, int64_t* hist, int64_t N, int F, int max_bin, int level, int kc, void* stream) {
  if (!bins || !gq || !hq || !pos || !hist || !gbt_shape(N, F, max_bin) || level < 0 || level > GBT_MAX_LEVEL || kc < 1 || kc > 65535) return OP_EINVAL;
  const int ft = 64 >> level;
  const int64_t gy = (F + ft - 1) / ft, cap = (((int64_t)1 << 22) - 1) / (gy * kc);     // below 2^22 work-groups of 1024 threads: the launch limit of 2^32 threads
  if (cap < 1) return OP_EINVAL;                                              // (the host's chunks of outputs keep gy kc below it: oneprot_amd/gbt.py plan_chunks)
  int64_t gx = (N + GBT_ROWS - 1) / GBT_ROWS;
  if (gx > cap) gx = cap;
  const size_t lds = (size_t)128 * max_bin * sizeof(int);
  if (hipMemsetAsync(hist, 0, oneprot_gbt_hist_bytes(F, max_bin, level) * (size_t)kc, (hipStream_t)stream) != hipSuccess) return OP_ELAUNCH;
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)k_gbt_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return OP_ELAUNCH;
  hipLaunchKernelGGL(k_gbt_hist, dim3((unsigned)gx, (unsigned)gy, (unsigned)kc), dim3(GBT_HIST_THREADS), lds, (hipStream_t)stream, (const unsigned char*)bins, gq, hq, pos, (ll_t*)hist, N, F,
                     max_bin, level);
  return launch_status();
}

extern "C" size_t oneprot_gbt_split_workspace(int F, int level, int kc) {
  if (F < 1 || F > 65535 || level < 0 || level > GBT_MAX_LEVEL || kc < 1 || kc > 65535) return 0;
  return ((size_t)kc << level) * (size_t)F * sizeof(GbtRec);
}

extern "C" int oneprot_gbt_split(const int64_t* hist, const float* cuts, const int* ncuts, const void* feat_keep, const int* expo, int* tree_feat, int* tree_bin, float* tree_thr,
                                 float* tree_leaf, void* gain_bytes, void* workspace, size_t workspace_bytes, int F, int max_bin, int level, int kc, int tree_nodes,
                                 float min_child_weight, float gamma, float reg_alpha, float reg_lambda, float learning_rate, void* stream) {
  if (!hist || !cuts || !ncuts || !feat_keep || !expo || !tree_feat || !tree_bin || !tree_thr || !tree_leaf || !workspace || !gbt_shape(1, F, max_bin)) return OP_EINVAL;
  if (level < 0 || level > GBT_MAX_LEVEL || kc < 1 || kc > 65535 || tree_nodes < (4 << level) - 1 || !(reg_lambda >= 0.f) || !(reg_alpha >= 0.f)) return OP_EINVAL;
  if (workspace_bytes < oneprot_gbt_split_workspace(F, level, kc) || ((uintptr_t)workspace & 7)) return OP_EINVAL;
  hipLaunchKernelGGL(k_gbt_split_scan, dim3((F + 3) / 4, 1 << level, kc), dim3(256), 0, (hipStream_t)stream, (const ll_t*)hist, ncuts, (const unsigned char*)feat_keep, expo,
                     (GbtRec*)workspace, F, max_bin, level, (double)min_child_weight, (double)reg_alpha, (double)reg_lambda);
  hipLaunchKernelGGL(k_gbt_split, dim3(1 << level, kc), dim3(256), 0, (hipStream_t)stream, (const GbtRec*)workspace, cuts, expo, tree_feat, tree_bin, tree_thr, tree_leaf,
                     (double*)gain_bytes, F, max_bin, level, tree_nodes, (double)gamma, (double)reg_alpha, (double)reg_lambda, (double)learning_rate);
  return launch_status();
}

// ---- levels 6 .. 8: node order, histogram and split search of a node group
static bool gbt_deep_level(int level) { return level > GBT_MAX_LEVEL && level <= GBT_DEEP_MAX_LEVEL; }
static bool gbt_group(int level, int node0, int nodes) { return gbt_deep_level(level) && node0 >= 0 && nodes >= 1 && node0 + nodes <= (1 << level); }

extern "C" int oneprot_gbt_node_keys(const int* pos, int* keys, int64_t N, int level, void* stream) {
  if (!pos || !keys || N < 1 || N > (1 << 24) || !gbt_deep_level(level)) return OP_EINVAL;
  hipLaunchKernelGGL(k_gbt_node_keys, dim3(gbt_grid(N)), dim3(256), 0, (hipStream_t)stream, pos, keys, N, level);
  return launch_status();
}

extern "C" int oneprot_gbt_node_seg(const int* sorted_keys, int* seg, int64_t N, int level, void* stream) {
  if (!sorted_keys || !seg || N < 1 || N > (1 << 24) || !gbt_deep_level(level)) return OP_EINVAL;
  hipLaunchKernelGGL(k_gbt_node_seg, dim3(((1 << level) + 1 + 255) / 256), dim3(256), 0, (hipStream_t)stream, sorted_keys, seg, N, level);
  return launch_status();
}

// the tile of k_gbt_hist_nodes per level, log2 of its features (the nodes of a tile are 64 over that): DESIGN.md section 6 has the shapes tried
static int gbt_tile_log2(int level) { return level == 6 ? GBT_TILE_LOG2_L6 : level == 7 ? GBT_TILE_LOG2_L7 : GBT_TILE_LOG2_L8; }

extern "C" size_t oneprot_gbt_hist_nodes_bytes(int F, int max_bin, int nodes) {
  if (F < 1 || F > 65535 || max_bin < 2 || max_bin > 256 || nodes < 1 || nodes > (1 << GBT_DEEP_MAX_LEVEL)) return 0;
  return (size_t)nodes * (size_t)F * (size_t)max_bin * 2 * sizeof(int64_t);
}

extern "C" int oneprot_gbt_hist_nodes(const void* bins, const int* gq, const int* hq, const int* order, const int* sorted_keys, const int* seg, int64_t* hist, int64_t N, int F,
                                      int max_bin, int level, int node0, int nodes, int tile_features, void* stream) {
  if (!bins || !gq || !hq || !order || !sorted_keys || !seg || !hist || !gbt_shape(N, F, max_bin) || !gbt_group(level, node0, nodes)) return OP_EINVAL;
  int ftl = gbt_tile_log2(level);
  if (tile_features != 0) {
    if (tile_features < 1 || tile_features > 64 || (tile_features & (tile_features - 1))) return OP_EINVAL;
    ftl = __builtin_ctz((unsigned)tile_features);
  }
  const int64_t gx = (N + GBT_ROWS - 1) / GBT_ROWS, tiles = (F + (1 << ftl) - 1) >> ftl, cap = (((int64_t)1 << 22) - 1) / gx;     // below 2^22 work-groups of 1024 threads
  const int64_t gy = tiles < cap ? (tiles < 65535 ? tiles : 65535) : (cap < 65535 ? cap : 65535);      // (gx <= 8198, so cap >= 511; a work-group strides over the tiles beyond gy)
  const size_t lds = (size_t)128 * max_bin * sizeof(int);
  if (hipMemsetAsync(hist, 0, oneprot_gbt_hist_nodes_bytes(F, max_bin, nodes), (hipStream_t)stream) != hipSuccess) return OP_ELAUNCH;
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)k_gbt_hist_nodes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return OP_ELAUNCH;
  hipLaunchKernelGGL(k_gbt_hist_nodes, dim3((unsigned)gx, (unsigned)gy), dim3(GBT_HIST_THREADS), lds, (hipStream_t)stream, (const unsigned char*)bins, gq, hq, order, sorted_keys, seg,
                     (ll_t*)hist, N, F, max_bin, level, node0, nodes, ftl);
  return launch_status();
}

extern "C" size_t oneprot_gbt_split_nodes_workspace(int F, int nodes) {
  if (F < 1 || F > 65535 || nodes < 1 || nodes > (1 << GBT_DEEP_MAX_LEVEL)) return 0;
  return (size_t)nodes * (size_t)F * sizeof(GbtRec);
}

// (levels 0 .. 5 are taken too, with any group: a whole shallow level through here gives oneprot_gbt_split's bits, which the tests hold it to)
extern "C" int oneprot_gbt_split_nodes(const int64_t* hist, const float* cuts, const int* ncuts, const void* feat_keep, const int* expo, int* tree_feat, int* tree_bin, float* tree_thr,
                                       float* tree_leaf, void* gain_bytes, void* workspace, size_t workspace_bytes, int F, int max_bin, int level, int node0, int nodes,
                                       int tree_nodes, float min_child_weight, float gamma, float reg_alpha, float reg_lambda, float learning_rate, void* stream) {
  if (!hist || !cuts || !ncuts || !feat_keep || !expo || !tree_feat || !tree_bin || !tree_thr || !tree_leaf || !workspace || !gbt_shape(1, F, max_bin)) return OP_EINVAL;
  if (level < 0 || level > GBT_DEEP_MAX_LEVEL || node0 < 0 || nodes < 1 || node0 + nodes > (1 << level) || tree_nodes < (4 << level) - 1 || !(reg_lambda >= 0.f) || !(reg_alpha >= 0.f))
    return OP_EINVAL;
  if (workspace_bytes < oneprot_gbt_split_nodes_workspace(F, nodes) || ((uintptr_t)workspace & 7)) return OP_EINVAL;
  hipLaunchKernelGGL(k_gbt_split_scan_nodes, dim3((F + 3) / 4, nodes, 1), dim3(256), 0, (hipStream_t)stream, (const ll_t*)hist, ncuts, (const unsigned char*)feat_keep, expo,
                     (GbtRec*)workspace, F, max_bin, nodes, (double)min_child_weight, (double)reg_alpha, (double)reg_lambda);
  hipLaunchKernelGGL(k_gbt_split_nodes, dim3(nodes, 1), dim3(256), 0, (hipStream_t)stream, (const GbtRec*)workspace, cuts, expo, tree_feat, tree_bin, tree_thr, tree_leaf,
                     (double*)gain_bytes, F, max_bin, nodes, (1 << level) - 1 + node0, tree_nodes, (double)gamma, (double)reg_alpha, (double)reg_lambda, (double)learning_rate);
  return launch_status();
}

extern "C" int oneprot_gbt_partition(const void* bins, const int* tree_feat, const int* tree_bin, int* pos, int64_t N, int F, int level, int kc, int tree_nodes, void* stream) {
  if (!bins || !tree_feat || !tree_bin || !pos || !gbt_shape(N, F, 2) || level < 0 || level > GBT_DEEP_MAX_LEVEL || kc < 1 || kc > 65535 || tree_nodes < (4 << level) - 1) return OP_EINVAL;
  const unsigned gx = gbt_grid(N) < 65536 ? gbt_grid(N) : 65536;
  hipLaunchKernelGGL(k_gbt_partition, dim3(gx, kc), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)bins, tree_feat, tree_bin, pos, N, F, level, tree_nodes);
  return launch_status();
}

extern "C" int oneprot_gbt_update(float* margin, const int* pos, const float* tree_leaf, int64_t N, int K, int k0, int kc, int tree_nodes, void* stream) {
  if (!margin || !pos || !tree_leaf || N < 1 || N > (1 << 24) || K < 1 || k0 < 0 || kc < 1 || kc > 65535 || k0 + kc > K || tree_nodes < 1) return OP_EINVAL;
  const unsigned gx = gbt_grid(N) < 65536 ? gbt_grid(N) : 65536;
  hipLaunchKernelGGL(k_gbt_update, dim3(gx, kc), dim3(256), 0, (hipStream_t)stream, margin, pos, tree_leaf, N, K, k0, tree_nodes);
  return launch_status();
}

extern "C" int oneprot_gbt_predict(const float* X, const int* tree_feat, const float* tree_thr, const float* tree_leaf, float* margin, int64_t N, int F, int K, int n_trees,
                                   int tree_nodes, float init_margin, void* stream) {
  if (!X || !tree_feat || !tree_thr || !tree_leaf || !margin || N < 1 || F < 1 || F > 65535 || K < 1 || K > 65535 || n_trees < 0 || tree_nodes < 1) return OP_EINVAL;
  hipLaunchKernelGGL(k_gbt_predict, dim3(gbt_grid(N * K)), dim3(256), 0, (hipStream_t)stream, X, tree_feat, tree_thr, tree_leaf, margin, N, F, K, n_trees, tree_nodes, init_margin);
  return launch_status();
}
