// MSA input on the device (include/oneprot_hip.h, "MSA input"): the greedy depth selection of ref src/data/utils/msa_utils.py:21-40 as an exact integer
// rule, and the gather of the chosen rows into token ids (ref src/data/datasets/msa_dataset.py:54-56).
//
// Selection.  S_j = sum over the chosen rows i of ham(i, j), an int32 per row; every step picks the unselected j with the best S_j, the lowest j among
// equals.  One launch per step (k_select_step), every MSA of the batch in it, nothing read back in between:
//   - a work-group owns a fixed range of one MSA's rows.  It first reduces the keys the groups of that MSA left in the previous step to the row picked
//     last (every group does this for itself: a few hundred 8-byte keys out of L2), then adds ham(last, j) to S_j of its rows and leaves its own best key;
//   - a key is (score << 32) | ~index for "max" and ((2^31 - 1 - score) << 32) | ~index for "min", so that "better score, then lower index" is the
//     unsigned 64-bit maximum: associative and commutative, any reduction tree gives the same pick and no atomics are needed.  0 is "no candidate";
//   - the keys of two consecutive steps live in two buffers (a group of step s may still read step s - 1 while another one writes step s);
//   - S_j < 0 marks a chosen row.  Step 1 writes S without reading it, so the workspace needs no clearing.
// Rows are compared 16 bytes per lane.  The host pads every row to a multiple of 16 bytes with a byte all rows of the MSA share (0), so that every
// load is aligned and the padding adds no mismatch: the row stride is L_b rounded up to 16, byte0 a multiple of 16.
#include "../../include/oneprot_hip.h"
#include "common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMinRowsPerGroup = 64;
constexpr int kMaxGroupsX = 1024;          // work-groups along one MSA's rows: what one group reduces again at the start of a step
constexpr int kMaxPicks = 1024;            // k_max: S_j <= 1023 * 65535 < 2^26
constexpr int kSeqTrunc = 1022;            // get_batch_converter(truncation_seq_length=1022)

typedef unsigned long long u64;

__host__ __device__ inline int64_t round_up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// work-groups along x for a batch of n MSAs whose deepest has max_rows rows
inline int groups_x(int n, int64_t max_rows) {
  int64_t want = (max_rows + kMinRowsPerGroup - 1) / kMinRowsPerGroup;
  int64_t cap = 4096 / n;
  if (cap > kMaxGroupsX) cap = kMaxGroupsX;
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  return want < 1 ? 1 : (int)want;
}

// the workspace: row offsets int64 [n] | pick order int32 [n, k_max] | keys u64 [2, n, gx] | S int32 [total_rows]
struct WsLayout { size_t row0, order, keys, acc, bytes; };
inline WsLayout ws_layout(int n, int k_max, int gx, int64_t total_rows) {
  WsLayout w;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  w.row0 = 0;
  w.order = up((size_t)n * 8);
  w.keys = w.order + up((size_t)n * k_max * 4);
  w.acc = w.keys + up((size_t)2 * n * gx * 8);
  w.bytes = w.acc + up((size_t)total_rows * 4);
  return w;
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    v = other > v ? other : v;
  }
  return v;
}

// the maximum of every thread's v, in every thread; `sh` holds kWaves keys.  Two barriers.
__device__ __forceinline__ u64 group_max_u64(u64 v, u64* sh) {
  v = wave_max_u64(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 m = sh[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) m = sh[w] > m ? sh[w] : m;
  __syncthreads();
  return m;
}

// bytes of a ^ b that are not zero, 16 at a time: ((x & 0x7f..) + 0x7f..) | x has a byte's top bit set exactly when the byte is not zero
__device__ __forceinline__ int mismatches16(const u32x4 a, const u32x4 b) {
  int c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned x = a[i] ^ b[i];
    c += __builtin_popcount((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u);
  }
  return c;
}

__device__ __forceinline__ int64_t rows_per_group(int64_t N, int gx) {
  const int64_t r = (N + gx - 1) / gx;
  return r < kMinRowsPerGroup ? kMinRowsPerGroup : r;
}

__global__ void k_select_offsets(const int64_t* __restrict__ table, int64_t* __restrict__ row0, int n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int64_t at = 0;
    for (int b = 0; b < n; ++b) { row0[b] = at; at += table[4 * b + 1]; }
  }
}

// step s = 1 .. : makes pick number s of every MSA that still has one to make (pick 0 is row 0)
__global__ __launch_bounds__(kThreads) void k_select_step(const unsigned char* __restrict__ bytes, const int64_t* __restrict__ table,
                                                          const int64_t* __restrict__ row0, int* __restrict__ acc, const u64* __restrict__ keys_prev,
                                                          u64* __restrict__ keys_cur, int* __restrict__ order, int step, int k_max, int min_mode) {
  __shared__ u64 sh[kWaves];
  const int b = blockIdx.y, gx = gridDim.x;
  const int64_t byte0 = table[4 * b], N = table[4 * b + 1], L = table[4 * b + 2], k = table[4 * b + 3];
  const int64_t picks = k < N ? k : N;
  if (step >= picks) return;                                      // this MSA is complete: its last keys stay for k_select_finish
  const int64_t rpg = rows_per_group(N, gx), r_first = blockIdx.x * rpg;
  if (r_first >= N) return;                                       // outside the MSA's extent: leaves before any barrier
  const int64_t r_end = r_first + rpg < N ? r_first + rpg : N;
  const int groups = (int)((N + rpg - 1) / rpg);

  int last = 0;
  if (step > 1) {
    u64 best = 0;
    for (int g = threadIdx.x; g < groups; g += kThreads) { const u64 v = keys_prev[(size_t)b * gx + g]; best = v > best ? v : best; }
    best = group_max_u64(best, sh);
    last = (int)(0xffffffffu - (unsigned)best);
    if ((unsigned)last >= (u64)N) last = 0;                       // cannot happen while step < picks <= N; keeps a torn table inside its rows
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) order[(size_t)b * k_max + step - 1] = last;

  const int64_t stride = round_up16(L);
  const int chunks = (int)(stride >> 4);
  int G = 1;                                                      // lanes per row: a power of two, at most 64
  while (G < 64 && G < chunks) G <<= 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & (G - 1), rows_per_wave = 64 / G;
  const u32x4* ref = reinterpret_cast<const u32x4*>(bytes + byte0 + (int64_t)last * stride);
  const bool one_chunk = chunks <= G;
  u32x4 ref0 = {0u, 0u, 0u, 0u};
  if (one_chunk && sub < chunks) ref0 = ref[sub];
  int* S = acc + row0[b];
  u64 best = 0;
  // every lane of a wave runs the same number of iterations (the shuffles need all 64); a lane past r_end computes nothing
  for (int64_t base = r_first + (int64_t)wave * rows_per_wave; base < r_end; base += (int64_t)kWaves * rows_per_wave) {
    const int64_t j = base + lane / G;
    int d = 0;
    if (j < r_end) {
      const u32x4* row = reinterpret_cast<const u32x4*>(bytes + byte0 + j * stride);
      if (one_chunk) {
        if (sub < chunks) d = mismatches16(ref0, row[sub]);
      } else {
        for (int c = sub; c < chunks; c += G) d += mismatches16(ref[c], row[c]);
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    if (j < r_end && sub == 0) {
      if (j == last) {
        S[j] = -1;
      } else {
        const int s = step == 1 ? d : S[j];
        if (s >= 0) {
          const int t = step == 1 ? d : s + d;
          S[j] = t;
          const u64 key = ((u64)(unsigned)(min_mode ? 0x7fffffff - t : t) << 32) | (0xffffffffu - (unsigned)j);
          best = key > best ? key : best;
        }
      }
    }
  }
  best = group_max_u64(best, sh);
  if (threadIdx.x == 0) keys_cur[(size_t)b * gx + blockIdx.x] = best;
}

// the last pick of every MSA, then its picks in ascending order
__global__ __launch_bounds__(kThreads) void k_select_finish(const int64_t* __restrict__ table, const u64* __restrict__ keys, int* __restrict__ order_ws,
                                                            int* __restrict__ indices, int* __restrict__ order_out, int gx, int n, int k_max) {
  __shared__ u64 sh[kWaves];
  __shared__ int picks_sh[kMaxPicks];
  const int b = blockIdx.x;
  const int64_t N = table[4 * b + 1], k = table[4 * b + 3];
  const int picks = (int)(k < N ? k : N);
  int* order = order_ws + (size_t)b * k_max;
  if (picks >= 2) {
    const int64_t rpg = rows_per_group(N, gx);
    const int groups = (int)((N + rpg - 1) / rpg);
    const u64* kb = keys + ((size_t)((picks - 1) & 1) * n + b) * gx;
    u64 best = 0;
    for (int g = threadIdx.x; g < groups; g += kThreads) { const u64 v = kb[g]; best = v > best ? v : best; }
    best = group_max_u64(best, sh);
    if (threadIdx.x == 0) order[picks - 1] = (int)(0xffffffffu - (unsigned)best);
  } else if (threadIdx.x == 0) {
    order[0] = 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < picks; i += kThreads) picks_sh[i] = order[i];
  __syncthreads();
  for (int i = threadIdx.x; i < k_max; i += kThreads) {
    if (i < picks) {
      const int v = picks_sh[i];
      int rank = 0;
      for (int q = 0; q < picks; ++q) rank += picks_sh[q] < v;       // the picks are distinct
      indices[(size_t)b * k_max + rank] = v;
      if (order_out) order_out[(size_t)b * k_max + i] = v;
    } else {
      indices[(size_t)b * k_max + i] = -1;
      if (order_out) order_out[(size_t)b * k_max + i] = -1;
    }
  }
}

// what the host mirror of the table says about the batch; false = refuse
struct BatchShape { int64_t total_rows, max_rows, max_picks; };
bool read_table(const int64_t* th, int n, int k_max, int64_t n_bytes, BatchShape& s) {
  s = BatchShape{0, 0, 0};
  for (int b = 0; b < n; ++b) {
    const int64_t byte0 = th[4 * b], N = th[4 * b + 1], L = th[4 * b + 2], k = th[4 * b + 3];
    if (N < 1 || N > 0x7fffffff || L < 1 || L > 65535 || k < 1 || k > k_max) return false;
    if (byte0 < 0 || (byte0 & 15) || byte0 > n_bytes || N * round_up16(L) > n_bytes - byte0) return false;
    s.total_rows += N;
    if (N > s.max_rows) s.max_rows = N;
    const int64_t picks = k < N ? k : N;
    if (picks > s.max_picks) s.max_picks = picks;
  }
  return true;
}

__device__ __forceinline__ int tokens_per_row(int64_t L, int max_length) {
  const int t = 1 + (int)(L < kSeqTrunc ? L : kSeqTrunc);
  return t < max_length ? t : max_length;
}

// grid (x over the tokens of a row, y = row of the output: 0 .. R_max - 1 the MSA rows, R_max the sequence side, z = MSA)
__global__ __launch_bounds__(kThreads) void k_tokenize(const unsigned char* __restrict__ bytes, const int64_t* __restrict__ table, const int* __restrict__ indices,
                                                       const int* __restrict__ byte_map, int64_t* __restrict__ tokens, const int* __restrict__ cu_tokens,
                                                       int64_t* __restrict__ seq_tokens, int n, int k_max, int R_max, int Lt_max, int Ls_max, int max_length,
                                                       int64_t T_tokens, int64_t T_pad, int cls_id, int pad_id, int eos_id) {
  const int b = blockIdx.z, r = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
  const int64_t byte0 = table[4 * b], N = table[4 * b + 1], L = table[4 * b + 2], k = table[4 * b + 3];
  const int picks = (int)(k < N ? k : N), Lt = tokens_per_row(L, max_length);
  const int64_t stride = round_up16(L);
  if (cu_tokens && b == 0 && r == 0 && blockIdx.x == 0)              // the stream's tail
    for (int64_t i = T_tokens + threadIdx.x; i < T_pad; i += kThreads) tokens[i] = pad_id;
  if (r == R_max) {                                                  // <cls> letters <eos>, truncated with <eos> kept (the HF ESM-2 tokenizer)
    if (!seq_tokens || t >= Ls_max) return;
    const int Ls = (int)(L + 2 < max_length ? L + 2 : max_length);
    int64_t id = pad_id;
    if (t == 0) id = cls_id;
    else if (t == Ls - 1) id = eos_id;
    else if (t < Ls) id = byte_map[bytes[byte0 + (t - 1)]];
    seq_tokens[(size_t)b * Ls_max + t] = id;
    return;
  }
  if (cu_tokens) {
    if (r >= picks || t >= Lt) return;
  } else if (t >= Lt_max) {
    return;
  }
  int64_t id = pad_id;
  if (r < picks && t < Lt) {
    int64_t row = indices[(size_t)b * k_max + r];
    row = row < 0 ? 0 : row < N ? row : N - 1;                       // the caller's indices are not validated: stay inside the MSA
    id = t == 0 ? cls_id : byte_map[bytes[byte0 + row * stride + (t - 1)]];
  }
  if (cu_tokens) tokens[(int64_t)cu_tokens[b] + (int64_t)r * Lt + t] = id;
  else tokens[((size_t)b * R_max + r) * Lt_max + t] = id;
}

}  // namespace

extern "C" size_t oneprot_msa_select_workspace(int n, int k_max, int64_t total_rows, int64_t max_rows) {
  if (n < 1 || n > 65535 || k_max < 1 || k_max > kMaxPicks || total_rows < n || max_rows < 1 || max_rows > total_rows) return 0;
  return ws_layout(n, k_max, groups_x(n, max_rows), total_rows).bytes;
}

extern "C" int oneprot_msa_select(const void* msa_bytes, const int64_t* table, void* workspace, int* indices, int* order, const int64_t* table_host,
                                  size_t workspace_bytes, int64_t n_bytes, int n, int k_max, int min_mode, void* stream) {
  if (!msa_bytes || !table || !workspace || !indices || !table_host) return OP_EINVAL;
  if (n < 1 || n > 65535 || k_max < 1 || k_max > kMaxPicks || n_bytes < 16 || (min_mode != 0 && min_mode != 1)) return OP_EINVAL;
  if (((uintptr_t)msa_bytes & 15) || ((uintptr_t)table & 7) || ((uintptr_t)workspace & 15)) return OP_EINVAL;
  BatchShape s;
  if (!read_table(table_host, n, k_max, n_bytes, s)) return OP_EINVAL;
  const int gx = groups_x(n, s.max_rows);
  const WsLayout w = ws_layout(n, k_max, gx, s.total_rows);
  if (workspace_bytes < w.bytes) return OP_EINVAL;
  char* ws = static_cast<char*>(workspace);
  int64_t* row0 = reinterpret_cast<int64_t*>(ws + w.row0);
  int* order_ws = reinterpret_cast<int*>(ws + w.order);
  u64* keys = reinterpret_cast<u64*>(ws + w.keys);
  int* acc = reinterpret_cast<int*>(ws + w.acc);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned char* bytes = static_cast<const unsigned char*>(msa_bytes);
  k_select_offsets<<<1, 64, 0, st>>>(table, row0, n);
  for (int step = 1; step < (int)s.max_picks; ++step) {
    const u64* prev = keys + (size_t)((step - 1) & 1) * n * gx;
    u64* cur = keys + (size_t)(step & 1) * n * gx;
    k_select_step<<<dim3(gx, n), kThreads, 0, st>>>(bytes, table, row0, acc, prev, cur, order_ws, step, k_max, min_mode);
  }
  k_select_finish<<<n, kThreads, 0, st>>>(table, keys, order_ws, indices, order, gx, n, k_max);
  return launch_status();
}

extern "C" int oneprot_msa_tokenize(const void* msa_bytes, const int64_t* table, const int* indices, const int* byte_map, int64_t* tokens, const int* cu_tokens,
                                    int64_t* seq_tokens, const int64_t* table_host, int64_t n_bytes, int n, int k_max, int R_max, int Lt_max, int Ls_max,
                                    int max_length, int64_t T_pad, int cls_id, int pad_id, int eos_id, void* stream) {
  if (!msa_bytes || !table || !indices || !byte_map || !tokens || !table_host) return OP_EINVAL;
  if (n < 1 || n > 65535 || k_max < 1 || k_max > kMaxPicks || max_length < 2 || R_max < 1 || R_max > kMaxPicks || Lt_max < 1 || n_bytes < 16) return OP_EINVAL;
  if (((uintptr_t)msa_bytes & 15) || ((uintptr_t)table & 7) || ((uintptr_t)tokens & 7)) return OP_EINVAL;
  if (seq_tokens && Ls_max < 2) return OP_EINVAL;
  BatchShape s;
  if (!read_table(table_host, n, k_max, n_bytes, s)) return OP_EINVAL;
  int64_t T_tokens = 0;
  for (int b = 0; b < n; ++b) {
    const int64_t N = table_host[4 * b + 1], L = table_host[4 * b + 2], k = table_host[4 * b + 3];
    const int64_t picks = k < N ? k : N;
    int64_t Lt = 1 + (L < kSeqTrunc ? L : kSeqTrunc), Ls = L + 2;
    if (Lt > max_length) Lt = max_length;
    if (Ls > max_length) Ls = max_length;
    if (picks > R_max || Lt > Lt_max || (seq_tokens && Ls > Ls_max)) return OP_EINVAL;
    T_tokens += picks * Lt;
  }
  if (cu_tokens && (T_pad < T_tokens || T_pad > 0x7fffffff)) return OP_EINVAL;
  const int width = seq_tokens && Ls_max > Lt_max ? Ls_max : Lt_max;
  const dim3 grid((width + kThreads - 1) / kThreads, R_max + (seq_tokens ? 1 : 0), n);
  k_tokenize<<<grid, kThreads, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const unsigned char*>(msa_bytes), table, indices, byte_map, tokens, cu_tokens,
                                                                     seq_tokens, n, k_max, R_max, Lt_max, Ls_max, max_length, T_tokens, T_pad, cls_id, pad_id,
                                                                     eos_id);
  return launch_status();
}
