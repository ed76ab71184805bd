// The one place that draws from Philox4x32-10 (common.h) and the one statement of the ELEMENT RULE of this library's stored-nowhere masks:
//   element e reads the 16-bit slice e & 7 of block(counter = e >> 3, stream id, seed): slice j is the low (j even) or high (j odd) half of word j >> 1;
//   a dropout keeps e iff that slice >= thr = round(p * 65536), and scales kept values by 65536 / (65536 - thr), the inverse of the keep probability used.
// Forward and backward kernels of every file regenerate the same mask because they all come through here.  tests/philox_ref.py restates the rule on the
// host and tests/test_dropout_rule_gpu.py pins every consumer to it.  (The attention-probability dropouts use the per-element hash of attn_drop.h.)
#pragma once
#include "common.h"

// the four words of one block: counter = (counter, stream id), key = seed, each split into its 32-bit halves
__device__ __forceinline__ void philox_block(uint64_t counter, uint64_t seed, uint64_t stream_id, unsigned (&w)[4]) {
  philox4x32_10((unsigned)counter, (unsigned)(counter >> 32), (unsigned)stream_id, (unsigned)(stream_id >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
}
// the slice of one element, for kernels whose lanes do not own whole blocks
__device__ __forceinline__ unsigned philox_slice16(size_t e, uint64_t seed, uint64_t stream_id) {
  unsigned w[4];
  philox_block(e >> 3, seed, stream_id, w);
  const unsigned j = (unsigned)e & 7u, q = j >> 1;
  const unsigned v = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
  return (j & 1u) ? (v >> 16) : (v & 0xffffu);
}
// the keep decisions of the eight elements 8 * block .. 8 * block + 7, for kernels whose lanes own whole blocks
__device__ __forceinline__ void philox_keep8(uint64_t block, unsigned thr, uint64_t seed, uint64_t stream_id, bool (&keep)[8]) {
  unsigned w[4];
  philox_block(block, seed, stream_id, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    keep[2 * j] = (w[j] & 0xffffu) >= thr;
    keep[2 * j + 1] = (w[j] >> 16) >= thr;
  }
}
// p -> (thr, scale); false for p < 0, NaN, p >= 1 and a p that rounds to thr = 65536 (nothing kept).  The fp32 expressions are part of the rule.
static inline bool dropout_thr_scale(float p, unsigned& thr, float& scale) {
  if (!(p >= 0.f) || !(p < 1.f)) return false;
  thr = (unsigned)(p * 65536.f + 0.5f);
  if (thr >= 65536u) return false;
  scale = 65536.f / (float)(65536u - thr);
  return true;
}
