// Text input on the device (include/oneprot_hip.h, "text input"): BERT normalisation, pre-tokenisation and WordPiece of a whole batch in one launch,
// the rule of ref src/data/datasets/text_dataset.py:25,51 (HF's fast BERT tokenizer) restated over tables the host builds (oneprot_amd/text_data.py).
//
// One work-group per text.  It walks the text's UTF-8 bytes kChunk at a time, everything in LDS, nothing but the ids written to memory:
//   1. decode: the thread of a lead byte reads the character's bytes (they may lie in the next chunk: the read goes to memory, bounded by the text's
//      end), looks the code point up in the two-level normalisation table and gets 0 .. 3 normalised characters, each with a kind (other / a word of
//      its own: punctuation, CJK / space).  A wave scan of the counts places them behind the characters carried from the previous chunk;
//   2. words: two ballots per 64 positions give the bit masks "a word ends here" and "a word starts here"; a start finds its word's number by
//      popcount and its end by find-first-set.  The last word of a chunk that is not the text's last may go on in the next chunk: its first 101
//      characters are carried (a word of more than 100 characters is [UNK] whatever follows, so 101 decide);
//   3. matching: threads take words.  The prefix hashes h_k of a word (h = h * P + c + 1 mod 2^32) give the hash of any substring as
//      h_e - h_s * P^(e - s), so one greedy step costs one table probe per candidate end and a string compare only on a hit of the full 32-bit key;
//      the probe verifies length, keyspace ("##" pieces are a keyspace of their own) and every character, so a collision never yields an id;
//   4. output: a scan of the words' piece counts gives every piece its place; the first max_length - 2 are written between [CLS] and [SEP].
// The walk stops once max_length - 2 pieces exist.  Integer arithmetic only, no atomics: two runs write the same bytes.
#include "../../include/oneprot_hip.h"
#include "common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kChunk = kThreads;                     // bytes per step, one per thread
constexpr int kMaxExpand = 3;                        // normalised characters per input character (the host asserts it when it builds the table)
constexpr int kMaxWord = 100;                        // WordPiece(max_input_chars_per_word=100)
constexpr int kTailKeep = kMaxWord + 1;
constexpr int kBuf = 1024;                           // >= kTailKeep + kChunk * kMaxExpand = 869, a multiple of 4 * kThreads / 4 and of 64
constexpr int kPerThread = kBuf / kThreads;
constexpr unsigned kP = 0x01000193u;
constexpr unsigned kCpMask = 0x1fffffu;
enum { KIND_OTHER = 0, KIND_SOLO = 1, KIND_SPACE = 2 };
static_assert(kTailKeep + kChunk * kMaxExpand <= kBuf - 1, "position n must exist in the masks");
static_assert(kTailKeep <= kThreads, "the carried characters are moved one per thread");

typedef unsigned long long u64;

struct WpArgs {
  const unsigned char* bytes;
  const int64_t* offsets;
  const int *nidx, *nent, *npool, *slots, *vchars;
  int *ids, *lengths;
  int n_blocks, n_pool, cap_mask, n_vchars, max_piece, max_length, cls, sep, unk, pad;
};

__device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// the id of the piece s[0 .. L) in keyspace `cont`, -1 when the vocabulary does not hold it
__device__ __forceinline__ int lookup(const WpArgs& a, const unsigned* s, int L, int cont, unsigned hsub) {
  const unsigned key = fmix32(hsub ^ ((unsigned)L * 0x9e3779b1u) ^ (cont ? 0x85ebca6bu : 0u));
  const int meta = L | (cont << 16);
  unsigned slot = key & (unsigned)a.cap_mask;
  for (int probe = 0; probe <= a.cap_mask; ++probe, slot = (slot + 1) & (unsigned)a.cap_mask) {
    const int4 e = reinterpret_cast<const int4*>(a.slots)[slot];       // {key, first character in vchars, length | keyspace << 16, id}
    if (e.w < 0) return -1;
    if ((unsigned)e.x == key && e.z == meta && e.y >= 0 && e.y <= a.n_vchars - L) {
      bool same = true;
      for (int k = 0; k < L; ++k) same &= a.vchars[e.y + k] == (int)(s[k] & kCpMask);
      if (same) return e.w;
    }
  }
  return -1;
}

// the pieces of the word buf[p0 .. p0 + len) into pb[p0 ..]; returns their number (1 .. len)
__device__ int match_word(const WpArgs& a, const unsigned* buf, unsigned* hb, int* pb, const unsigned* powp, int p0, int len) {
  if (len > kMaxWord) { pb[p0] = a.unk; return 1; }
  unsigned h = 0;
  for (int k = 0; k < len; ++k) { h = h * kP + (buf[p0 + k] & kCpMask) + 1u; hb[p0 + k] = h; }       // hb[p0 + k] = the hash of the first k + 1 characters
  int start = 0, np = 0;
  while (start < len) {
    const unsigned hs = start ? hb[p0 + start - 1] : 0u;
    int end = start + a.max_piece < len ? start + a.max_piece : len;     // no piece of the vocabulary is longer
    int id = -1;
    for (; end > start; --end) {
      id = lookup(a, buf + p0 + start, end - start, start > 0, hb[p0 + end - 1] - hs * powp[end - start]);
      if (id >= 0) break;
    }
    if (id < 0) { pb[p0] = a.unk; return 1; }                            // one position without a match: the whole word is [UNK]
    pb[p0 + np++] = id;
    start = end;
  }
  return np;
}

__global__ __launch_bounds__(kThreads) void k_wordpiece(const WpArgs a) {
  __shared__ unsigned buf[kBuf];                     // normalised characters: code point | kind << 21
  __shared__ unsigned hbuf[kBuf];
  __shared__ int pbuf[kBuf];
  __shared__ unsigned short wstart[kBuf], wlen[kBuf], wcnt[kBuf], woff[kBuf];
  __shared__ u64 brk[kBuf / 64], stt[kBuf / 64];
  __shared__ unsigned powp[kMaxWord + 1];
  __shared__ int csum[kWaves], psum[kWaves];
  __shared__ int tail_start, tail_len;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int64_t o0 = a.offsets[b], o1 = a.offsets[b + 1];
  const int budget = a.max_length - 2;
  int* out = a.ids + (size_t)b * a.max_length;
  if (tid == 0) {
    unsigned p = 1;
    for (int k = 0; k <= kMaxWord; ++k) { powp[k] = p; p *= kP; }
  }
  int tail = 0, produced = 0;
  __syncthreads();
  for (int64_t pos = o0; produced < budget; pos += kChunk) {
    const bool final = pos + kChunk >= o1;
    // ---- 1. decode and normalise
    int cnt = 0;
    unsigned e = 0;
    const int64_t i = pos + tid;
    if (i < o1) {
      const unsigned c0 = a.bytes[i];
      if ((c0 & 0xc0u) != 0x80u) {
        unsigned cp;
        int nb;
        if (c0 < 0x80u) { cp = c0; nb = 1; }
        else if ((c0 & 0xe0u) == 0xc0u) { cp = c0 & 0x1fu; nb = 2; }
        else if ((c0 & 0xf0u) == 0xe0u) { cp = c0 & 0x0fu; nb = 3; }
        else if ((c0 & 0xf8u) == 0xf0u) { cp = c0 & 0x07u; nb = 4; }
        else { cp = 0xfffdu; nb = 1; }
        bool bad = false;
        for (int k = 1; k < nb; ++k) {
          const unsigned c = i + k < o1 ? a.bytes[i + k] : 0u;
          bad |= (c & 0xc0u) != 0x80u;
          cp = (cp << 6) | (c & 0x3fu);
        }
        if (bad || cp > 0x10ffffu) cp = 0xfffdu;                        // dropped by the rule; the host refuses what does not decode
        const int blk = a.nidx[cp >> 8];
        if (blk >= 0 && blk < a.n_blocks) e = (unsigned)a.nent[blk * 256 + (int)(cp & 255u)];
        cnt = (int)((e >> 23) & 3u);
      }
    }
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) csum[wave] = incl;
    if (tid == 0) tail_start = -1;
    __syncthreads();
    int at = tail + incl - cnt, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) at += csum[w];
      total += csum[w];
    }
    const int n = tail + total;                                         // <= 869
    if (cnt == 1) {
      buf[at] = e & 0x7fffffu;
    } else if (cnt > 1) {
      const int pidx = (int)(e & kCpMask);
      for (int k = 0; k < cnt; ++k) buf[at + k] = pidx + k < a.n_pool ? ((unsigned)a.npool[pidx + k] & 0x7fffffu) : (0x20u | (KIND_SPACE << 21));
    }
    __syncthreads();
    // ---- 2. words: position p = k * kThreads + tid, so that a wave's ballot is the mask of 64 consecutive positions
    unsigned mine = 0;                                                  // bit k: position k * kThreads + tid starts a word; bit 4 + k: that word is a single character
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int p = k * kThreads + tid;
      const unsigned kind = p < n ? buf[p] >> 21 : (unsigned)KIND_SPACE;
      const unsigned prev = p > 0 && p <= n ? buf[p - 1] >> 21 : (unsigned)KIND_SPACE;
      const bool is_brk = kind != KIND_OTHER;
      const bool is_start = p < n && kind != KIND_SPACE && (kind != KIND_OTHER || prev != KIND_OTHER);
      const u64 mb = __ballot(is_brk), ms = __ballot(is_start);
      if (lane == 0) { brk[k * kWaves + wave] = mb; stt[k * kWaves + wave] = ms; }
      if (is_start) mine |= (1u << k) | (kind != KIND_OTHER ? 16u << k : 0u);
    }
    __syncthreads();
    int n_starts = 0;
#pragma unroll
    for (int w = 0; w < kBuf / 64; ++w) n_starts += __builtin_popcountll(stt[w]);
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      if (!(mine & (1u << k))) continue;
      const int p = k * kThreads + tid, wd = p >> 6;
      int widx = __builtin_popcountll(stt[wd] & ((1ull << (p & 63)) - 1ull));
      for (int w = 0; w < wd; ++w) widx += __builtin_popcountll(stt[w]);
      int end = p + 1;
      if (!(mine & (16u << k))) {                                       // the first position behind p that is no word character; position n is one
        int w2 = end >> 6;
        u64 m = brk[w2] >> (end & 63);
        if (m) {
          end += __builtin_ctzll(m);
        } else {
          end = kBuf;
          for (++w2; w2 < kBuf / 64; ++w2)
            if (brk[w2]) { end = w2 * 64 + __builtin_ctzll(brk[w2]); break; }
        }
        if (end > n) end = n;
      }
      const int len = end - p < kTailKeep ? end - p : kTailKeep;
      if (!final && end == n && !(mine & (16u << k))) { tail_start = p; tail_len = len; }       // may go on in the next chunk; the last word, so at most one
      else { wstart[widx] = (unsigned short)p; wlen[widx] = (unsigned short)len; }
    }
    __syncthreads();
    const int ts = tail_start;
    const int n_words = n_starts - (ts >= 0 ? 1 : 0);
    // ---- 3. matching
    for (int w = tid; w < n_words; w += kThreads) wcnt[w] = (unsigned short)match_word(a, buf, hbuf, pbuf, powp, wstart[w], wlen[w]);
    __syncthreads();
    // ---- 4. places of the pieces
    int c[kPerThread], s = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) { const int w = tid * kPerThread + k; c[k] = w < n_words ? wcnt[w] : 0; s += c[k]; }
    int pin = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(pin, o, 64);
      if (lane >= o) pin += v;
    }
    if (lane == 63) psum[wave] = pin;
    __syncthreads();
    int off = pin - s, pieces = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) off += psum[w];
      pieces += psum[w];
    }
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) { const int w = tid * kPerThread + k; if (w < n_words) woff[w] = (unsigned short)off; off += c[k]; }
    __syncthreads();
    for (int w = tid; w < n_words; w += kThreads) {
      const int o = produced + woff[w], m = wcnt[w], p0 = wstart[w];
      for (int k = 0; k < m && o + k < budget; ++k) out[1 + o + k] = pbuf[p0 + k];
    }
    produced += pieces;
    // ---- the carried word moves to the front
    const int tl = ts >= 0 ? tail_len : 0;
    const unsigned v = tid < tl ? buf[ts + tid] : 0u;
    __syncthreads();
    if (tid < tl) buf[tid] = v;
    tail = tl;
    if (final) break;
  }
  if (produced > budget) produced = budget;
  if (tid == 0) { out[0] = a.cls; out[1 + produced] = a.sep; a.lengths[b] = produced + 2; }
  for (int j = produced + 2 + tid; j < a.max_length; j += kThreads) out[j] = a.pad;
}

}  // namespace

extern "C" int oneprot_wordpiece_encode(const void* text_bytes, const int64_t* offsets, const int* norm_index, const int* norm_entries, const int* norm_pool,
                                        const int* vocab_slots, const int* vocab_chars, int* ids, int* lengths, const int64_t* offsets_host, int64_t n_bytes,
                                        int n_texts, int n_blocks, int n_pool, int n_slots, int n_vocab_chars, int max_piece_chars, int max_length, int cls_id,
                                        int sep_id, int unk_id, int pad_id, void* stream) {
  if (!text_bytes || !offsets || !norm_index || !norm_entries || !norm_pool || !vocab_slots || !vocab_chars || !ids || !lengths || !offsets_host) return OP_EINVAL;
  if (n_texts < 1 || n_texts > ONEPROT_WORDPIECE_MAX_TEXTS || max_length < 2 || max_length > ONEPROT_WORDPIECE_MAX_LENGTH || n_bytes < 0) return OP_EINVAL;
  if (n_blocks < 1 || n_blocks > 0x1100 || n_pool < 1 || n_vocab_chars < 1 || max_piece_chars < 1 || max_piece_chars > kMaxWord) return OP_EINVAL;
  if (n_slots < 2 || n_slots > (1 << 26) || (n_slots & (n_slots - 1))) return OP_EINVAL;
  if (cls_id < 0 || sep_id < 0 || unk_id < 0 || pad_id < 0) return OP_EINVAL;
  if (((uintptr_t)vocab_slots & 15) || ((uintptr_t)offsets & 7) || ((uintptr_t)ids & 3) || ((uintptr_t)lengths & 3)) return OP_EINVAL;
  if (offsets_host[0] < 0 || offsets_host[n_texts] > n_bytes) return OP_EINVAL;
  for (int b = 0; b < n_texts; ++b)
    if (offsets_host[b + 1] < offsets_host[b]) return OP_EINVAL;
  WpArgs a;
  a.bytes = static_cast<const unsigned char*>(text_bytes);
  a.offsets = offsets;
  a.nidx = norm_index; a.nent = norm_entries; a.npool = norm_pool; a.slots = vocab_slots; a.vchars = vocab_chars;
  a.ids = ids; a.lengths = lengths;
  a.n_blocks = n_blocks; a.n_pool = n_pool; a.cap_mask = n_slots - 1; a.n_vchars = n_vocab_chars; a.max_piece = max_piece_chars; a.max_length = max_length;
  a.cls = cls_id; a.sep = sep_id; a.unk = unk_id; a.pad = pad_id;
  k_wordpiece<<<n_texts, kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
  return launch_status();
}
