"""The end-to-end fixtures of the gradient-boosted tree tests and the host rebuild of a fit's sampling masks.  A helper module like tests/gbt_ref.py, not a
test.  Every fixture is N = 300, F = 8, max_bin 16, depth 3, 5 rounds on Gaussian features of numpy's default_rng; tests/test_gbt_cpu.py asserts that the
restatement's decision gap on each of them is at least 1e-4, so that no fixture asks the device to reproduce a coin toss."""
import functools

import numpy as np

from tests import gbt_ref as R
from tests import philox_ref as PR

N, F, B, DEPTH, ROUNDS = 300, 8, 16, 3, 5
RNG_DOMAIN_GBT = 6
SAMPLE_SEED, SAMPLE_RATE = 1234, 0.8
PARAMS = dict(n_estimators=ROUNDS, max_depth=DEPTH, max_bin=B, learning_rate=0.3)

# name -> (objective, seed of default_rng).  Seeds were picked by the gap alone (seeds 0 and 3 have exact cross-partition ties and are not used); the gaps
# the restatement reports are recorded in GAPS and re-checked by test_gbt_cpu.py::test_fixture_gaps.
FIXTURES = {"logistic": (R.LOGISTIC, 1), "squared": (R.SQUARED, 2), "softmax": (R.SOFTMAX, 5), "multilabel": (R.LOGISTIC, 5), "sampled": (R.LOGISTIC, 4)}
GAPS = {"logistic": 3.35e-3, "squared": 2.58e-3, "softmax": 2.48e-3, "multilabel": 1.17e-3, "sampled": 2.53e-3}       # as the restatement reported them (3 digits)


def slices16(n, seed, stream):
    """uint16-valued int64 [n]: the 16-bit slice of elements 0 .. n-1 under oneprot_dropout_f32's element rule (tests/philox_ref.py philox_keep's layout)"""
    n8 = (n + 7) // 8
    e8 = np.arange(n8, dtype=np.uint64)
    words = PR.philox4x32_10(e8 & np.uint64(PR.M32), e8 >> np.uint64(32), stream & PR.M32, (stream >> 32) & PR.M32, seed & PR.M32, (seed >> 32) & PR.M32)
    w = np.stack(words, axis=1).astype(np.int64)
    return np.stack([w & 0xFFFF, w >> 16], axis=2).reshape(-1)[:n]


def stream_of(local):
    return (RNG_DOMAIN_GBT << 60) | int(local)


def sampling_masks(n_rows, n_feat, rounds, seed, subsample, colsample):
    """(row masks, feature masks) of every round of a fit with random_state = seed: rows of round t from stream t, features from stream rounds + t"""
    rows = [R.row_mask_from_slices(slices16(n_rows, seed, stream_of(t)), subsample) for t in range(rounds)]
    feats = [R.feat_mask_from_slices(slices16(n_feat, seed, stream_of(rounds + t)), colsample) if colsample < 1.0 else np.ones(n_feat, dtype=bool)
             for t in range(rounds)]
    return rows, feats


def data(name):
    """(X fp32 [N, F], y) of a fixture"""
    objective, seed = FIXTURES[name]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, F)).astype(np.float32)
    if name in ("logistic", "sampled"):
        y = ((X @ rng.standard_normal(F) + 0.5 * rng.standard_normal(N)) > 0).astype(np.float32)
    elif name == "squared":
        y = (np.sin(X[:, 0]) + X[:, 1] * X[:, 2]).astype(np.float32)
    elif name == "softmax":
        y = np.argmax(X @ rng.standard_normal((F, 3)) + 0.5 * rng.standard_normal((N, 3)), axis=1).astype(np.int64)
    else:
        y = ((X @ rng.standard_normal((F, 5)) + 0.5 * rng.standard_normal((N, 5))) > 0).astype(np.float32)
    return X, y


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's fit of a fixture, computed once and shared (callers must not change it)"""
    X, y = data(name)
    kw = {}
    if name == "sampled":
        kw["row_masks"], kw["feat_masks"] = sampling_masks(N, F, ROUNDS, SAMPLE_SEED, SAMPLE_RATE, SAMPLE_RATE)
    return R.fit(X, y, FIXTURES[name][0], **PARAMS, **kw)
