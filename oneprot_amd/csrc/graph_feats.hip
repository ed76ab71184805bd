// Pocket / struct_graph input on the device (include/oneprot_hip.h, "graph input"): the atom records of a whole batch to the tensors of a GraphBatch,
// the rule of ref src/data/utils/struct_graph_utils.py:31-144 (get_atom_pos, compute_diherals, calc_side_chain_embs, calc_bb_embs) as
// oneprot_amd/graph_data.py states it on the host.  DESIGN.md section 7 states the rule once.
//
// Two launches, one thread per residue, no atomics, no shared memory:
//   1. k_select: the thread walks its residue's run of atoms once, front to back, and keeps for each of the nine places (N, CA, C, CB, G, D, E, Z,
//      NH1) the last atom whose name stands in the place's set -- numpy's fancy assignment lets the last write win.  No such atom: NaN.  A NaN
//      component of N or C takes CA's.  It writes x, batch, the three coordinate rows and the four side-chain torsions (sines, then cosines), which
//      need the residue's own atoms only; the first threads copy graph_ptr to ptr.
//   2. k_backbone: the thread reads the N, CA, C rows of its residue and of its two neighbours INSIDE its graph (launch 1 wrote them) and writes
//      phi, psi, omega (cosines, then sines); phi of a graph's first residue and psi, omega of its last are angle 0.
// The arithmetic is the host's, operation by operation, in fp32 without contraction: torch's cross (a1 b2 - a2 b1, ...), sums of three that start
// from +0 (torch's reduction does: a sum of three -0 is +0, which decides atan2(0, 0) = 0 against atan2(0, -0) = pi), nan_to_num after the division
// and after atan2.  So every degenerate case -- a NaN operand, a zero vector -- falls out of the same formula as on the host, and a residue's result
// depends on nothing but its own atoms and its neighbours' rows: the same bits alone or in any batch.
#include "../../include/oneprot_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPlaces = 9;
constexpr float kFltMax = 3.402823466e+38f;

struct V3 { float x, y, z; };

constexpr unsigned code(char a, char b = 0, char c = 0) { return (unsigned)(unsigned char)a | ((unsigned)(unsigned char)b << 8) | ((unsigned)(unsigned char)c << 16); }

// the place of an atom name (its first four bytes, zero padded, little endian), -1 for a name of no set (ref struct_graph_utils.py:33-41)
__device__ __forceinline__ int place_of(unsigned name) {
  switch (name) {
    case code('N'): return 0;
    case code('C', 'A'): return 1;
    case code('C'): return 2;
    case code('C', 'B'): return 3;
    case code('C', 'G'): case code('S', 'G'): case code('O', 'G'): case code('C', 'G', '1'): case code('O', 'G', '1'): return 4;
    case code('C', 'D'): case code('S', 'D'): case code('C', 'D', '1'): case code('O', 'D', '1'): case code('N', 'D', '1'): return 5;
    case code('C', 'E'): case code('N', 'E'): case code('O', 'E', '1'): return 6;
    case code('C', 'Z'): case code('N', 'Z'): return 7;
    case code('N', 'H', '1'): return 8;
    default: return -1;
  }
}

__device__ __forceinline__ float nan_to_num(float v) {
  if (v != v) return 0.0f;
  if (v > kFltMax) return kFltMax;
  if (v < -kFltMax) return -kFltMax;
  return v;
}

__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float sum3(float a, float b, float c) { return ((0.0f + a) + b) + c; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return sum3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ float norm(V3 a) { return sqrtf(dot(a, a)); }

// compute_diherals
__device__ __forceinline__ float dihedral(V3 v1, V3 v2, V3 v3) {
  const V3 n1 = cross(v1, v2), n2 = cross(v2, v3);
  const float a = dot(n1, n2);
  const float b = nan_to_num(dot(cross(n1, n2), v2) / norm(v2));
  return nan_to_num(atan2f(b, a));
}

// _normalize of calc_bb_embs
__device__ __forceinline__ V3 unit(V3 v) {
  const float n = norm(v);
  return {nan_to_num(v.x / n), nan_to_num(v.y / n), nan_to_num(v.z / n)};
}

__device__ __forceinline__ V3 load3(const float* p, int64_t r) { return {p[3 * r], p[3 * r + 1], p[3 * r + 2]}; }
__device__ __forceinline__ void store3(float* p, int64_t r, V3 v) { p[3 * r] = v.x; p[3 * r + 1] = v.y; p[3 * r + 2] = v.z; }

struct GfArgs {
  const float* atom_pos;
  const unsigned* atom_name4;
  const int64_t* res_atom_ptr;
  const unsigned char* res_type;
  const int64_t* graph_ptr;
  int64_t* x;
  float *ca, *cn, *cc, *bb, *sc;
  int64_t *batch, *ptr;
  int64_t A, N;
  int G;
};

__global__ __launch_bounds__(kThreads) void k_select(const GfArgs a) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r <= a.G) a.ptr[r] = a.graph_ptr[r];             // N >= 1 and G <= N: the grid holds at least G + 1 threads (checked by the entry point)
  if (r >= a.N) return;
  int64_t at[kPlaces];
#pragma unroll
  for (int k = 0; k < kPlaces; ++k) at[k] = -1;
  int64_t a0 = a.res_atom_ptr[r], a1 = a.res_atom_ptr[r + 1];
  if (a0 < 0) a0 = 0;                                   // the entry point has validated the host copy of the table; the device copy is bounded all the same
  if (a1 > a.A) a1 = a.A;
  for (int64_t i = a0; i < a1; ++i) {
    const int p = place_of(a.atom_name4[i]);
#pragma unroll
    for (int k = 0; k < kPlaces; ++k)
      if (p == k) at[k] = i;
  }
  const float nan = __builtin_nanf("");
  V3 pos[kPlaces];
#pragma unroll
  for (int k = 0; k < kPlaces; ++k) pos[k] = at[k] >= 0 ? load3(a.atom_pos, at[k]) : V3{nan, nan, nan};
  const V3 ca = pos[1];
#pragma unroll
  for (int k = 0; k < 3; k += 2) {                      // N and C: a NaN component takes CA's
    if (pos[k].x != pos[k].x) pos[k].x = ca.x;
    if (pos[k].y != pos[k].y) pos[k].y = ca.y;
    if (pos[k].z != pos[k].z) pos[k].z = ca.z;
  }
  store3(a.cn, r, pos[0]);
  store3(a.ca, r, ca);
  store3(a.cc, r, pos[2]);
  a.x[r] = a.res_type[r];
  int lo = 0, hi = a.G;                                 // the last graph g with graph_ptr[g] <= r
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.graph_ptr[mid] <= r) lo = mid; else hi = mid;
  }
  a.batch[r] = lo;
  // the chain N, CA, CB, G, D, E, Z and its four torsions
  const V3 chain[7] = {pos[0], pos[1], pos[3], pos[4], pos[5], pos[6], pos[7]};
  V3 v[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = sub(chain[k + 1], chain[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float ang = dihedral(v[k], v[k + 1], v[k + 2]);
    a.sc[8 * r + k] = sinf(ang);
    a.sc[8 * r + 4 + k] = cosf(ang);
  }
}

__global__ __launch_bounds__(kThreads) void k_backbone(const GfArgs a) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.N) return;
  int64_t g = a.batch[r];
  if (g < 0) g = 0;
  if (g >= a.G) g = a.G - 1;
  const bool has_prev = r > 0 && r > a.graph_ptr[g], has_next = r + 1 < a.graph_ptr[g + 1] && r + 1 < a.N;
  const V3 n = load3(a.cn, r), ca = load3(a.ca, r), c = load3(a.cc, r);
  const V3 u1 = unit(sub(ca, n)), u2 = unit(sub(c, ca));      // U[3 r], U[3 r + 1] of the flattened chain
  float phi = 0.0f, psi = 0.0f, omega = 0.0f;
  if (has_prev) {
    const V3 u0 = unit(sub(n, load3(a.cc, r - 1)));           // U[3 r - 1]
    phi = dihedral(u0, u1, u2);
  }
  if (has_next) {
    const V3 nn = load3(a.cn, r + 1);
    const V3 u3 = unit(sub(nn, c)), u4 = unit(sub(load3(a.ca, r + 1), nn));      // U[3 r + 2], U[3 r + 3]
    psi = dihedral(u1, u2, u3);
    omega = dihedral(u2, u3, u4);
  }
  float* o = a.bb + 6 * r;
  o[0] = cosf(phi); o[1] = cosf(psi); o[2] = cosf(omega);
  o[3] = sinf(phi); o[4] = sinf(psi); o[5] = sinf(omega);
}

}  // namespace

extern "C" int oneprot_graph_featurize(const float* atom_pos, const int* atom_name4, const int64_t* res_atom_ptr, const void* res_type_bytes,
                                       const int64_t* graph_ptr, int64_t* x, float* coords_ca, float* coords_n, float* coords_c, float* bb_embs,
                                       float* side_chain_embs, int64_t* batch, int64_t* ptr, const int64_t* res_atom_ptr_host, const int64_t* graph_ptr_host,
                                       int64_t A, int64_t N, int G, void* stream) {
  if (!atom_pos || !atom_name4 || !res_atom_ptr || !res_type_bytes || !graph_ptr || !x || !coords_ca || !coords_n || !coords_c || !bb_embs || !side_chain_embs ||
      !batch || !ptr || !res_atom_ptr_host || !graph_ptr_host) return OP_EINVAL;
  if (N < 1 || G < 1 || A < 0 || N > ONEPROT_GRAPH_MAX_NODES || G > N) return OP_EINVAL;
  if (graph_ptr_host[0] != 0 || graph_ptr_host[G] != N || res_atom_ptr_host[0] != 0 || res_atom_ptr_host[N] != A) return OP_EINVAL;
  for (int g = 0; g < G; ++g)
    if (graph_ptr_host[g + 1] < graph_ptr_host[g]) return OP_EINVAL;
  for (int64_t r = 0; r < N; ++r)
    if (res_atom_ptr_host[r + 1] < res_atom_ptr_host[r]) return OP_EINVAL;
  GfArgs a;
  a.atom_pos = atom_pos;
  a.atom_name4 = reinterpret_cast<const unsigned*>(atom_name4);
  a.res_atom_ptr = res_atom_ptr;
  a.res_type = static_cast<const unsigned char*>(res_type_bytes);
  a.graph_ptr = graph_ptr;
  a.x = x; a.ca = coords_ca; a.cn = coords_n; a.cc = coords_c; a.bb = bb_embs; a.sc = side_chain_embs; a.batch = batch; a.ptr = ptr;
  a.A = A; a.N = N; a.G = G;
  const unsigned blocks = (unsigned)((N + 1 + kThreads - 1) / kThreads);      // N + 1 threads: ptr has G + 1 <= N + 1 entries
  hipStream_t s = static_cast<hipStream_t>(stream);
  k_select<<<blocks, kThreads, 0, s>>>(a);
  k_backbone<<<blocks, kThreads, 0, s>>>(a);
  return launch_status();
}
