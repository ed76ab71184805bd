"""Host reference of the library's dropout masks, written from the generators' definitions and not from the kernels: Philox4x32-10
(Salmon et al., SC'11; the Random123 round function and Weyl key schedule) in numpy uint64 arithmetic, and the per-element hash of the
attention-probability dropout.  Vectorised over counters so that a mask of a few million elements takes a fraction of a second.

Mask rules (oneprot_amd/csrc/featops.hip, the oneprot_dropout_* kernels; attention.hip, attn_keep / attn_drop_make):
  hidden-state / LoRA dropout   element e keeps iff the 16-bit slice e & 7 of Philox4x32-10(counter = (e >> 3, stream), key = seed) is >= thr,
                                slice j = bits 16 * (j & 1) .. + 15 of output word j >> 1; thr = round(p * 65536)
  attention-probability dropout keep(bh, q, k) iff the upper 16 bits of lowbias32(mix(q, k, bh, seed, stream)) are >= thr
"""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0, c1, c2, c3) under key (k0, k1): Python ints or numpy arrays (broadcast); returns four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & M32), np.uint64(k1 & M32)
    m0, m1, mask = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1), np.uint64(M32)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]            # 32 x 32 -> 64-bit products (exact in uint64)
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & mask, (p0 >> sh) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & mask, (k1 + np.uint64(PHILOX_W1)) & mask
    return [v.astype(np.uint32) for v in c]


def dropout_threshold(p):
    """thr = round(p * 65536) and the scale 65536 / (65536 - thr) of kept values, as the launchers compute them in fp32"""
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    return thr, np.float32(65536.0) / np.float32(65536 - thr)


def philox_keep(n, p, seed, stream):
    """bool [n]: the keep mask of the Philox dropout kernels for elements 0 .. n-1 (n a multiple of 8)"""
    assert n % 8 == 0
    thr, _ = dropout_threshold(p)
    e8 = np.arange(n // 8, dtype=np.uint64)
    words = philox4x32_10(e8 & np.uint64(M32), e8 >> np.uint64(32), stream & M32, (stream >> 32) & M32, seed & M32, (seed >> 32) & M32)
    w = np.stack(words, axis=1)                                   # [n/8, 4]
    halves = np.stack([w & 0xFFFF, w >> 16], axis=2).reshape(-1)  # element 8 * i + 2 * j + h  <-  word j, half h
    return halves >= thr


def attn_keep(B, H, L, p, seed, stream):
    """bool [B, H, L(q), L(k)]: the keep mask of the attention-probability dropout"""
    thr, _ = dropout_threshold(p)
    m = ((seed ^ ((stream * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)) * 0xD6E8FEB86659FD93) & 0xFFFFFFFFFFFFFFFF
    s0 = m & M32
    s1 = ((m >> 32) ^ (stream * 0x2545F491)) & M32
    u = np.uint64
    q = np.arange(L, dtype=np.uint64)[:, None]
    k = np.arange(L, dtype=np.uint64)[None, :]
    out = np.empty((B * H, L, L), dtype=bool)
    mask = u(M32)
    qk = ((q * u(0x9E3779B1)) & mask) ^ ((k * u(0x85EBCA77) + u(s0)) & mask)
    for bh in range(B * H):
        x = qk ^ ((u(bh) * u(0xC2B2AE3D) + u(s1)) & mask)
        x ^= x >> u(16)
        x = (x * u(0x7FEB352D)) & mask
        x ^= x >> u(15)
        x = (x * u(0x846CA68B)) & mask
        x ^= x >> u(16)
        out[bh] = (x >> u(16)) >= thr
    return out.reshape(B, H, L, L)
