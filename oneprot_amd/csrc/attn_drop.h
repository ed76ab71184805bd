// The mask rule of the attention-probability dropouts, shared by attention.hip (BERT tower: hf BertSelfAttention) and msa.hip (MSA tower: fair-esm
// RowSelfAttention / ColumnSelfAttention).  keep(bh, q, k) is a pure function of (seed, stream, bh, q, k): one 32-bit integer hash per ELEMENT (lowbias32
// finaliser over a multiplicative mix of the indices), so that every kernel regenerates the same mask from its own layout; kept iff the upper 16 bits
// >= thr16 = round(p * 65536), kept probabilities scaled by 65536 / (65536 - thr16).  p < 2^-17 gives thr16 = 0: no dropout at all.
// tests/philox_ref.py restates the rule on the host and tests/test_attention_dropout_gpu.py pins it: change no constant here.
#pragma once
#include "philox.h"      // dropout_thr_scale: p -> (thr16, scale) as for the Philox masks

struct AttnDrop { unsigned thr16, s0, s1; float scale; };
__device__ __forceinline__ bool attn_keep(unsigned qi, unsigned ki, unsigned bh, const AttnDrop& dr) {
  unsigned x = (qi * 0x9E3779B1u) ^ (ki * 0x85EBCA77u + dr.s0) ^ (bh * 0xC2B2AE3Du + dr.s1);
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return (x >> 16) >= dr.thr16;
}
static int attn_drop_make(float p, uint64_t seed, uint64_t stream_id, AttnDrop& dr) {
  if (!dropout_thr_scale(p, dr.thr16, dr.scale)) return OP_EINVAL;
  const uint64_t m = (seed ^ (stream_id * 0x9E3779B97F4A7C15ull)) * 0xD6E8FEB86659FD93ull;
  dr.s0 = (unsigned)m; dr.s1 = (unsigned)(m >> 32) ^ (unsigned)(stream_id * 0x2545F491u);
  return OP_OK;
}
