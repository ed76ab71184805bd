"""The host reference of the dropout generators (tests/philox_ref.py) pinned on published values, so that the GPU tests that compare every kernel's mask
with it (tests/test_production_sizes_gpu.py) compare with Philox4x32-10 itself."""
import numpy as np

from tests import philox_ref as R


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox4x32_10_known_answers():
    """Random123's known-answer vectors for philox4x32 with 10 rounds (kat_vectors)"""
    assert _hex(R.philox4x32_10(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _hex(R.philox4x32_10(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_vectorised_equals_scalar_calls():
    """the array form (counters broadcast against scalar stream words) gives what one call per counter gives, also past 2^32 elements"""
    ctr = np.array([0, 1, 7, 0xFFFFFFFF, 0x1_0000_0000 + 5], dtype=np.uint64)
    lo, hi = ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32)
    vec = np.stack(R.philox4x32_10(lo, hi, 0x89ABCDEF, 0x1234567, 0xDEADBEEF, 0x5EED), axis=1)
    for i, c in enumerate(ctr.tolist()):
        one = R.philox4x32_10(c & 0xFFFFFFFF, c >> 32, 0x89ABCDEF, 0x1234567, 0xDEADBEEF, 0x5EED)
        assert [int(w) for w in one] == [int(w) for w in vec[i]]


def test_philox_keep_slices_and_rate():
    """element 8 i + 2 j + h reads half h of word j of counter i; keep rate 1 - thr / 65536"""
    seed, stream, p = (0x1234 << 32) | 0xABCD, (0x77 << 32) | 5, 0.1
    keep = R.philox_keep(64 * 1024, p, seed, stream)
    words = R.philox4x32_10(3, 0, stream & 0xFFFFFFFF, stream >> 32, seed & 0xFFFFFFFF, seed >> 32)
    thr, scale = R.dropout_threshold(p)
    assert thr == 6554 and abs(float(scale) - 65536 / (65536 - 6554)) < 1e-6
    for j in range(4):
        assert keep[24 + 2 * j] == (int(words[j]) & 0xFFFF >= thr)
        assert keep[24 + 2 * j + 1] == (int(words[j]) >> 16 >= thr)
    assert abs(keep.mean() - (1 - thr / 65536)) < 4 * (0.1 * 0.9 / keep.size) ** 0.5


def test_attention_keep_rate_and_independence():
    keep = R.attn_keep(2, 3, 67, 0.1, (5 << 40) | 9, (1 << 61) | 3)
    assert keep.shape == (2, 3, 67, 67)
    assert abs(keep.mean() - (1 - 6554 / 65536)) < 0.01
    other = R.attn_keep(2, 3, 67, 0.1, (5 << 40) | 9, (1 << 61) | 4)
    assert abs(float((keep == other).mean()) - (0.9 * 0.9 + 0.1 * 0.1)) < 0.02
