// Retrieval at database scale (ref retrieval_metric.py:83-102, eval.py:158-184): the similarity tile S . M^T is formed on the matrix pipe and consumed
// in registers -- compared against the diagonal and counted (oneprot_sim_rank; oneprot_sim_rank_ties also counts equality), or offered to a running k-best list (oneprot_sim_topk) -- so the N x N
// matrix is never written.  The contraction is the fp32-input MFMA v_mfma_f32_32x32x2_f32: fp32 operands, and per output element the k-ordered fmaf chain
// acc = fmaf(a_k, b_k, acc) from k = 0 upwards, which is the chain k_sgemm (sgemm.hip) computes with alpha = 1.  Ranks therefore equal those of
// oneprot_sgemm + oneprot_diag_rank bit for bit (tests/test_retrieval_gpu.py demands torch.equal), and so do top-k scores.
//
// One tile body serves all three kernels: a block of 256 threads (2 x 2 waves) forms a (64 * MT) x 128 tile, 32-deep K slices staged through LDS.
// The MFMA takes k = 2 s + h from lane half h at step s, so a slice is stored [row][h][s]: a lane reads four consecutive steps of its half with one
// 16-byte LDS read and issues them in ascending order.  Rows past the end of either operand and k past D are zero-filled: fmaf(0, 0, acc) is exact.
#include "common.h"
#include "../../include/oneprot_hip.h"

#define SIM_BK 32
#define SIM_LD 36      // floats per LDS row: 32 + 4, rows 144 bytes apart (16-byte aligned, eight consecutive rows cover all 64 banks with their 16-byte reads)
#define SIM_TN 128

// acc[mt][ct][reg]: row (wr * 32 * MT + mt * 32 + sim_reg_row(reg, h)), column (wc * 64 + ct * 32 + (lane & 31)) of the tile; wr = wave & 1, wc = wave >> 1
__device__ __forceinline__ int sim_reg_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// A rows [a0, a0 + 64 MT) clipped to aend, B rows [b0, b0 + 128) clipped to bend; VEC = rows are 16-byte aligned (D % 4 == 0 and aligned bases).
// Ends with a __syncthreads(): the LDS buffers are free when it returns.
template <int MT, bool VEC>
__device__ __forceinline__ void sim_tile(const float* __restrict__ A, int a0, int aend, const float* __restrict__ B, int b0, int bend, int D, float* sA, float* sB,
                                         f32x16 (&acc)[MT][2]) {
  constexpr int NA = MT * 2, NB = 4;      // float4 per thread and slice
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][ct][i] = 0.f;
  f32x4 ra[NA], rb[NB];
  unsigned oka[NA], okb[NB];      // which of the four elements exist; the others are zeroed when the slice is stored
  // Every load reads a valid (clamped) address and nothing depends on its result before the slice is stored, so the loads of the next slice stay in flight
  // during the multiply.  Both operands have at least one row in range (a0 < aend, b0 < bend) and D >= 1 (VEC: D >= 4).
  auto load4 = [&](const float* __restrict__ P, int row, int rend, int gk, unsigned& ok) -> f32x4 {
    const float* p = P + (size_t)min(row, rend - 1) * D;
    f32x4 v;
    if (VEC) {
      ok = (row < rend && gk < D) ? 15u : 0u;
      v = *reinterpret_cast<const f32x4*>(p + min(gk, D - 4));
    } else {
      ok = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ok |= (row < rend && gk + e < D) ? 1u << e : 0u;
        v[e] = p[min(gk + e, D - 1)];
      }
    }
    return v;
  };
  auto fetch = [&](int k0) {
#pragma unroll
    for (int it = 0; it < NA; ++it) { const int idx = tid + it * 256; ra[it] = load4(A, a0 + (idx >> 3), aend, k0 + 4 * (idx & 7), oka[it]); }
#pragma unroll
    for (int it = 0; it < NB; ++it) { const int idx = tid + it * 256; rb[it] = load4(B, b0 + (idx >> 3), bend, k0 + 4 * (idx & 7), okb[it]); }
  };
  // k = 4q .. 4q+3 of a row are (h, s) = (0, 2q), (1, 2q), (0, 2q+1), (1, 2q+1)
  auto put = [&](float* s, int idx, f32x4 v, unsigned ok) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (ok >> e & 1u) ? v[e] : 0.f;
    float* p = s + (idx >> 3) * SIM_LD + 2 * (idx & 7);
    *reinterpret_cast<f32x2_t*>(p) = f32x2_t{v[0], v[2]};
    *reinterpret_cast<f32x2_t*>(p + 16) = f32x2_t{v[1], v[3]};
  };
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += SIM_BK) {
#pragma unroll
    for (int it = 0; it < NA; ++it) put(sA, tid + it * 256, ra[it], oka[it]);
#pragma unroll
    for (int it = 0; it < NB; ++it) put(sB, tid + it * 256, rb[it], okb[it]);
    __syncthreads();
    if (k0 + SIM_BK < D) fetch(k0 + SIM_BK);      // in flight during the multiply
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 a[MT], b[2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(sA + (wr * 32 * MT + mt * 32 + r) * SIM_LD + h * 16 + 4 * t);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) b[ct] = *reinterpret_cast<const f32x4*>(sB + (wc * 64 + ct * 32 + r) * SIM_LD + h * 16 + 4 * t);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) acc[mt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][e], b[ct][e], acc[mt][ct], 0, 0, 0);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- diagonal
// diag[i] = S_i . M_i from the diagonal 128 x 128 tiles, by the tile body: the same chain as element (i, i) of any tile of k_sim_rank
template <bool VEC>
__global__ void __launch_bounds__(256) k_sim_pair_dot(const float* __restrict__ S, const float* __restrict__ M, float* __restrict__ diag, int N, int D) {
  __shared__ __attribute__((aligned(16))) float sA[128 * SIM_LD];
  __shared__ __attribute__((aligned(16))) float sB[SIM_TN * SIM_LD];
  const int t0 = blockIdx.x * 128;
  f32x16 acc[2][2];
  sim_tile<2, VEC>(S, t0, N, M, t0, N, D, sA, sB, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave & 1, wc = wave >> 1, h = lane >> 5;
  if (wr != wc) return;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = wr * 64 + mt * 32 + sim_reg_row(reg, h), col = wc * 64 + mt * 32 + (lane & 31);
      if (row == col && t0 + row < N) diag[t0 + row] = acc[mt][mt][reg];
    }
}

// ---------------------------------------------------------------------------------------------------------------- ranks
// One 128 x 128 tile per block.  Blocks are numbered so that 16 row tiles x all column tiles form a group with the row tile running fastest: the blocks
// in flight together share a few megabytes of S and M rows.
// TIES (oneprot_sim_rank_ties): next to every `v > diag` count the same tile value is compared `v == diag` and counted the same way into tie_row / tie_col,
// the matching pair (global row == global column) left out by its index.  Without TIES the added lines do not exist: the kernel is oneprot_sim_rank's as before.
template <bool VEC, bool TIES>
__global__ void __launch_bounds__(256) k_sim_rank(const float* __restrict__ S, const float* __restrict__ M, const float* __restrict__ diag, int N, int D, int row0, int rows,
                                                  int nrt, int nct, int* __restrict__ rank_row, int* __restrict__ rank_col, int* __restrict__ tie_row,
                                                  int* __restrict__ tie_col) {
  __shared__ __attribute__((aligned(16))) float sA[128 * SIM_LD];
  __shared__ __attribute__((aligned(16))) float sB[SIM_TN * SIM_LD];
  __shared__ float sDr[128];
  __shared__ int sCr[128], sCc[128];
  __shared__ int sTr[TIES ? 128 : 1], sTc[TIES ? 128 : 1];
  constexpr int GR = 16;
  const int per_group = GR * nct, group = blockIdx.x / per_group, rem = blockIdx.x % per_group;
  const int gr_rows = min(GR, nrt - group * GR);
  const int rt = group * GR + rem % gr_rows, ct_ = rem / gr_rows;
  if (ct_ >= nct) return;                         // the last group has fewer than GR row tiles: its spare block numbers (whole block, before any barrier)
  const int rend = row0 + rows, r0 = row0 + rt * 128, c0 = ct_ * SIM_TN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1, h = lane >> 5;
  if (tid < 128) { sDr[tid] = r0 + tid < rend ? diag[r0 + tid] : 0.f; sCr[tid] = 0; sCc[tid] = 0; }
  if (TIES && tid < 128) { sTr[tid] = 0; sTc[tid] = 0; }
  f32x16 acc[2][2];
  sim_tile<2, VEC>(S, r0, rend, M, c0, N, D, sA, sB, acc);      // its barriers also publish sDr / sCr / sCc (and sTr / sTc)
  int ccol[2] = {0, 0};
  int tcol[2] = {0, 0};
  float dcol[2];
  bool vcol[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int j = c0 + wc * 64 + ct * 32 + (lane & 31);
    vcol[ct] = j < N;
    dcol[ct] = vcol[ct] ? diag[j] : 0.f;
  }
  const int jrel = c0 + wc * 64 + (lane & 31) - r0;      // TIES: column j of ct is the matching pair of tile row `row` when row == jrel + 32 ct
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = wr * 64 + mt * 32 + sim_reg_row(reg, h);
      const bool vrow = r0 + row < rend;
      const float drow = sDr[row];
      int lo = 0, hi = 0;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float v = acc[mt][ct][reg];
        const unsigned long long m = __ballot(vrow && vcol[ct] && v > drow);
        lo += __popc((unsigned)m);
        hi += __popc((unsigned)(m >> 32));
        ccol[ct] += (vrow && vcol[ct] && v > dcol[ct]) ? 1 : 0;
      }
      if (lane == 0 && lo) atomicAdd(&sCr[wr * 64 + mt * 32 + sim_reg_row(reg, 0)], lo);
      if (lane == 32 && hi) atomicAdd(&sCr[wr * 64 + mt * 32 + sim_reg_row(reg, 1)], hi);
      if constexpr (TIES) {
        int tlo = 0, thi = 0;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const float v = acc[mt][ct][reg];
          const bool other = vrow && vcol[ct] && row != jrel + 32 * ct;      // in range on both sides (the zero padding past N / the slab is no tie of a zero diagonal) and not the pair itself
          const unsigned long long m = __ballot(other && v == drow);
          tlo += __popc((unsigned)m);
          thi += __popc((unsigned)(m >> 32));
          tcol[ct] += (other && v == dcol[ct]) ? 1 : 0;
        }
        if (lane == 0 && tlo) atomicAdd(&sTr[wr * 64 + mt * 32 + sim_reg_row(reg, 0)], tlo);
        if (lane == 32 && thi) atomicAdd(&sTr[wr * 64 + mt * 32 + sim_reg_row(reg, 1)], thi);
      }
    }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
    if (ccol[ct]) atomicAdd(&sCc[wc * 64 + ct * 32 + (lane & 31)], ccol[ct]);
  if constexpr (TIES) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
      if (tcol[ct]) atomicAdd(&sTc[wc * 64 + ct * 32 + (lane & 31)], tcol[ct]);
  }
  __syncthreads();
  if (tid < 128) {
    if (sCr[tid] && r0 + tid < rend) atomicAdd(&rank_row[r0 + tid], sCr[tid]);
    if constexpr (TIES) { if (sTr[tid] && r0 + tid < rend) atomicAdd(&tie_row[r0 + tid], sTr[tid]); }
  } else {
    const int c = tid - 128;
    if (sCc[c] && c0 + c < N) atomicAdd(&rank_col[c0 + c], sCc[c]);
    if constexpr (TIES) { if (sTc[c] && c0 + c < N) atomicAdd(&tie_col[c0 + c], sTc[c]); }
  }
}

// ---------------------------------------------------------------------------------------------------------------- top-k
// An entry is one 64-bit key: the score's bits made monotone (high word) and ~index (low word), so that a larger key is a larger score or, at equal
// scores, a smaller database index.  0 is below every key of a non-NaN score and marks an empty slot.
__device__ __forceinline__ unsigned long long sim_key(float s, int j) {
  unsigned u = __builtin_bit_cast(unsigned, s + 0.f);      // + 0: -0 becomes +0, the two compare equal as scores
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ((unsigned long long)u << 32) | (unsigned)~j;
}
__device__ __forceinline__ float sim_key_score(unsigned long long key) {
  unsigned u = (unsigned)(key >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
  return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ int sim_key_index(unsigned long long key) { return (int)~(unsigned)key; }

#define TOPK_TQ 64
// dynamic LDS: lists [64][k] keys, worst key [64], sA [64][36], sB [128][36], worst position [64]
static inline size_t topk_lds(int k) { return (size_t)TOPK_TQ * k * 8 + TOPK_TQ * 8 + (TOPK_TQ + SIM_TN) * SIM_LD * 4 + TOPK_TQ * 4; }

// A block owns 64 queries and the database tiles [blockIdx.y * tps, (blockIdx.y + 1) * tps).  Per query the k best keys so far sit unordered in LDS together
// with the worst of them and its slot; a tile's score is admitted when it beats that worst key (it then replaces it and the list is rescanned for the new
// worst), so after the first tiles almost every score is dropped by one comparison.  Two waves hold the same 32 queries (different columns) and take turns.
template <bool VEC>
__global__ void __launch_bounds__(256) k_sim_topk(const float* __restrict__ Q, const float* __restrict__ Db, int nq, int N, int D, int k, int tps, int ntiles,
                                                  unsigned long long* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(smem);
  unsigned long long* worst = lists + (size_t)TOPK_TQ * k;
  float* sA = reinterpret_cast<float*>(worst + TOPK_TQ);
  float* sB = sA + TOPK_TQ * SIM_LD;
  int* wpos = reinterpret_cast<int*>(sB + SIM_TN * SIM_LD);
  const int q0 = blockIdx.x * TOPK_TQ, split = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1, h = lane >> 5;
  for (int e = tid; e < TOPK_TQ * k; e += 256) lists[e] = 0ull;
  if (tid < TOPK_TQ) { worst[tid] = 0ull; wpos[tid] = 0; }
  const int t_end = min((split + 1) * tps, ntiles);
  for (int t = split * tps; t < t_end; ++t) {
    const int c0 = t * SIM_TN;
    f32x16 acc[1][2];
    sim_tile<1, VEC>(Q, q0, nq, Db, c0, N, D, sA, sB, acc);      // (its first barrier also publishes the cleared lists)
    for (int ph = 0; ph < 2; ++ph) {
      if (wc == ph) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            const int row = wr * 32 + sim_reg_row(reg, h), j = c0 + wc * 64 + ct * 32 + (lane & 31);
            const unsigned long long key = sim_key(acc[0][ct][reg], j);
            unsigned long long m = __ballot(q0 + row < nq && j < N && key > worst[row]);
            while (m) {                                              // uniform over the wave
              const int src = __ffsll(m) - 1;
              m &= m - 1;
              const unsigned long long ck = __shfl(key, src, 64);
              const int crow = wr * 32 + sim_reg_row(reg, src >> 5);
              if (ck > worst[crow]) {                                // the threshold may have risen since the ballot
                unsigned long long* L = lists + (size_t)crow * k;
                L[wpos[crow]] = ck;                                  // every lane stores the same value: each lane's later reads follow its own store
                unsigned long long mn = ~0ull;
                int mp = 0;
                for (int p = lane; p < k; p += 64) { const unsigned long long kv = L[p]; if (kv < mn) { mn = kv; mp = p; } }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                  const unsigned long long on = __shfl_xor(mn, o, 64);
                  const int op = __shfl_xor(mp, o, 64);
                  if (on < mn || (on == mn && op < mp)) { mn = on; mp = op; }
                }
                worst[crow] = mn;
                wpos[crow] = mp;
              }
            }
          }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  // descending order by counting: slot = number of keys ahead of this one (empty slots keep their relative order behind the real keys)
  for (int e = tid; e < TOPK_TQ * k; e += 256) {
    const int q = e / k, p = e - q * k;
    if (q0 + q >= nq) break;
    const unsigned long long* L = lists + (size_t)q * k;
    const unsigned long long key = L[p];
    int ahead = 0;
    for (int t = 0; t < k; ++t) { const unsigned long long o = L[t]; ahead += (o > key || (o == key && t < p)) ? 1 : 0; }
    ws[((size_t)split * nq + q0 + q) * k + ahead] = key;
  }
}

// One block per query: the final slot of a key is its slot in its own (descending) list plus, by binary search, the number of larger keys in every other list.
__global__ void __launch_bounds__(256) k_sim_topk_merge(const unsigned long long* __restrict__ ws, int nq, int k, int splits, float* __restrict__ scores,
                                                        long long* __restrict__ indices) {
  const int q = blockIdx.x;
  for (int e = threadIdx.x; e < splits * k; e += 256) {
    const int s = e / k, p = e - s * k;
    const unsigned long long key = ws[((size_t)s * nq + q) * k + p];
    if (key == 0ull) continue;
    int slot = p;
    for (int s2 = 0; s2 < splits && slot < k; ++s2) {
      if (s2 == s) continue;
      const unsigned long long* L = ws + ((size_t)s2 * nq + q) * k;
      int lo = 0, hi = k;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (L[mid] > key) lo = mid + 1; else hi = mid; }
      slot += lo;
    }
    if (slot < k) { scores[(size_t)q * k + slot] = sim_key_score(key); indices[(size_t)q * k + slot] = sim_key_index(key); }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline bool sim_vec_ok(const void* a, const void* b, int D) { return (D & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

extern "C" int oneprot_sim_pair_dot(const float* S, const float* M, float* diag, int N, int D, void* stream) {
  if (!S || !M || !diag || N <= 0 || D <= 0) return OP_EINVAL;
  const dim3 grid((N + 127) / 128);
  if (sim_vec_ok(S, M, D)) hipLaunchKernelGGL(k_sim_pair_dot<true>, grid, dim3(256), 0, (hipStream_t)stream, S, M, diag, N, D);
  else hipLaunchKernelGGL(k_sim_pair_dot<false>, grid, dim3(256), 0, (hipStream_t)stream, S, M, diag, N, D);
  return launch_status();
}

static int sim_rank_launch(const float* S, const float* M, const float* diag, int N, int D, int row0, int rows, int* rank_row, int* rank_col, int* tie_row, int* tie_col,
                           void* stream) {
  if (!S || !M || !diag || !rank_row || !rank_col || N <= 0 || D <= 0 || row0 < 0 || rows <= 0 || row0 > N - rows) return OP_EINVAL;
  const int nrt = (rows + 127) / 128, nct = (N + SIM_TN - 1) / SIM_TN, groups = (nrt + 15) / 16;
  const int64_t blocks = (int64_t)groups * 16 * nct;        // (the last group's spare numbers return at once)
  if (blocks > 0x7fffffff) return OP_EINVAL;                // a slab this large: the caller passes fewer rows per call
  const dim3 grid((unsigned)blocks), block(256);
  const bool vec = sim_vec_ok(S, M, D);
#define SIM_RANK_GO(V, T) hipLaunchKernelGGL((k_sim_rank<V, T>), grid, block, 0, (hipStream_t)stream, S, M, diag, N, D, row0, rows, nrt, nct, rank_row, rank_col, tie_row, tie_col)
  if (tie_row) { if (vec) SIM_RANK_GO(true, true); else SIM_RANK_GO(false, true); }
  else { if (vec) SIM_RANK_GO(true, false); else SIM_RANK_GO(false, false); }
#undef SIM_RANK_GO
  return launch_status();
}

extern "C" int oneprot_sim_rank(const float* S, const float* M, const float* diag, int N, int D, int row0, int rows, int* rank_row, int* rank_col, void* stream) {
  return sim_rank_launch(S, M, diag, N, D, row0, rows, rank_row, rank_col, nullptr, nullptr, stream);
}

extern "C" int oneprot_sim_rank_ties(const float* S, const float* M, const float* diag, int N, int D, int row0, int rows, int* rank_row, int* rank_col, int* tie_row,
                                     int* tie_col, void* stream) {
  if (!tie_row || !tie_col) return OP_EINVAL;
  return sim_rank_launch(S, M, diag, N, D, row0, rows, rank_row, rank_col, tie_row, tie_col, stream);
}

// query tiles x database splits: enough blocks to fill the chip twice over when there are few queries, at most 64 lists to merge per query
static void topk_plan(int nq, int N, int& qtiles, int& splits, int& tps, int& ntiles) {
  qtiles = (nq + TOPK_TQ - 1) / TOPK_TQ;
  ntiles = (N + SIM_TN - 1) / SIM_TN;
  int want = (512 + qtiles - 1) / qtiles;
  want = want > 64 ? 64 : want;
  want = want > ntiles ? ntiles : want;
  tps = (ntiles + want - 1) / want;
  splits = (ntiles + tps - 1) / tps;
}

extern "C" size_t oneprot_sim_topk_workspace(int nq, int N, int k) {
  if (nq <= 0 || N <= 0 || k < 1 || k > 256 || k > N) return 0;
  int qtiles, splits, tps, ntiles;
  topk_plan(nq, N, qtiles, splits, tps, ntiles);
  return (size_t)splits * nq * k * sizeof(unsigned long long);
}

extern "C" int oneprot_sim_topk(const float* Q, const float* Db, int nq, int N, int D, int k, float* scores, int64_t* indices, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (!Q || !Db || !scores || !indices || !workspace || nq <= 0 || N <= 0 || D <= 0 || k < 1 || k > 256 || k > N) return OP_EINVAL;
  if (workspace_bytes < oneprot_sim_topk_workspace(nq, N, k) || ((uintptr_t)workspace & 7)) return OP_EINVAL;
  int qtiles, splits, tps, ntiles;
  topk_plan(nq, N, qtiles, splits, tps, ntiles);
  const size_t lds = topk_lds(k);
  const bool vec = sim_vec_ok(Q, Db, D);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(vec ? (const void*)k_sim_topk<true> : (const void*)k_sim_topk<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return OP_ELAUNCH;
  unsigned long long* ws = reinterpret_cast<unsigned long long*>(workspace);
  if (vec) hipLaunchKernelGGL(k_sim_topk<true>, dim3(qtiles, splits), dim3(256), lds, (hipStream_t)stream, Q, Db, nq, N, D, k, tps, ntiles, ws);
  else hipLaunchKernelGGL(k_sim_topk<false>, dim3(qtiles, splits), dim3(256), lds, (hipStream_t)stream, Q, Db, nq, N, D, k, tps, ntiles, ws);
  hipLaunchKernelGGL(k_sim_topk_merge, dim3(nq), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)ws, nq, k, splits, scores, reinterpret_cast<long long*>(indices));
  return launch_status();
}
