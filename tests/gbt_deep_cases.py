"""The fixtures of the deep tree levels (max_depth 7 .. 9 of XGBRegressor: tests/test_gbt_deep_cpu.py, tests/test_gbt_deep_gpu.py).  A helper module like
tests/gbt_cases.py, not a test.  End-to-end fits are reg:squarederror on gbt_cases._recipe("squared", seed, N, F) at learning rate 0.3; the seeds were picked
by the restatement's decision gap alone (other seeds of the same recipes have gaps down to 1e-6: do not swap one without re-checking), and
test_gbt_deep_cpu.py re-checks every gap.  Below them: the node layouts and hand-written segments of the kernel-level cases with their numpy references."""
import functools

import numpy as np

from tests import gbt_cases as C
from tests import gbt_ref as R

LR, SAMPLE_SEED, SAMPLE_RATE = 0.3, 1234, 0.8
# name -> (N, F, max_bin, depth, min_child_weight, rounds, sampled, recipe seed)
FITS = {"d7": (6000, 12, 16, 7, 24.0, 3, False, 1), "d8s": (6000, 12, 32, 8, 16.0, 2, True, 3), "d9": (9000, 12, 32, 9, 12.0, 3, False, 1),
        "d9s": (9000, 12, 32, 9, 12.0, 2, True, 4), "d9w": (9000, 130, 16, 9, 12.0, 1, False, 2)}
GAPS = {"d7": 9.03e-4, "d8s": 9.13e-4, "d9": 2.68e-4, "d9s": 6.31e-4, "d9w": 6.90e-4}          # as the restatement reported them (3 digits)
DEEP_SPLITS = {"d7": 74, "d8s": 91, "d9": 378, "d9s": 289, "d9w": 181}                          # nodes at levels >= 6 that split, over all rounds
GBT_ROWS = 2047                                                                                 # positions of a run of the node-ordered histogram kernel


def fit_data(name):
    N, F, B, depth, mcw, rounds, sampled, seed = FITS[name]
    return C._recipe("squared", seed, N, F)


def fit_params(name):
    """the constructor keywords of a fixture, as both sides take them"""
    N, F, B, depth, mcw, rounds, sampled, seed = FITS[name]
    return dict(n_estimators=rounds, max_depth=depth, max_bin=B, learning_rate=LR, min_child_weight=mcw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's fit of a fixture, computed once and shared (callers must not change it)"""
    N, F, B, depth, mcw, rounds, sampled, seed = FITS[name]
    X, y = fit_data(name)
    kw = {}
    if sampled:
        kw["row_masks"], kw["feat_masks"] = C.sampling_masks(N, F, rounds, SAMPLE_SEED, SAMPLE_RATE, SAMPLE_RATE)
    return R.fit(X, y, R.SQUARED, **fit_params(name), **kw)


def deep_splits(ref):
    return sum(int((tr["feat"][63:] >= 0).sum()) for rnd in ref["trees"] for tr in rnd)


# ================================================================================================================== node order
def level_pos(rng, N, level):
    """pos int32 [N] over the heap: every node of the level that N rows can fill, node 1 of the level left empty, a tenth of the rows at shallower heap ids
    (they stopped at a leaf above)"""
    L, base = 1 << level, (1 << level) - 1
    n = rng.integers(0, L, N)
    if N >= L:
        n[:L] = np.arange(L)
    n[n == 1] = 0
    pos = (base + n).astype(np.int32)
    stopped = rng.random(N) < 0.1
    pos[stopped] = rng.integers(0, base, int(stopped.sum()))
    return pos


def order_reference(pos, level):
    """(order, sorted keys, seg [L + 1]) by numpy: the stable argsort of the keys and searchsorted"""
    L, base = 1 << level, (1 << level) - 1
    key = np.where((pos >= base) & (pos < base + L), pos - base, L).astype(np.int64)
    order = np.argsort(key, kind="stable")
    return order.astype(np.int32), key[order].astype(np.int32), np.searchsorted(key[order], np.arange(L + 1), side="left").astype(np.int32)


# ================================================================================================================== histograms of a node group
def random_rows(rng, N, F, B):
    """(bins uint8 [N, F], gq, hq int32 [N]) with a tenth of the rows carrying g = h = 0 (dropped by subsampling) and |q| <= 2^20"""
    bins = rng.integers(0, B, (N, F)).astype(np.uint8)
    gq = rng.integers(-(1 << R.FRAC), (1 << R.FRAC) + 1, N).astype(np.int32)
    hq = rng.integers(1, (1 << R.FRAC) + 1, N).astype(np.int32)
    dropped = rng.random(N) < 0.1
    gq[dropped], hq[dropped] = 0, 0
    return bins, gq, hq


HAND_LEVEL = 8
HAND_ONE, HAND_RUN, HAND_RUN1, HAND_THREE = 3, 40, 41, 100        # level-8 nodes holding 1, exactly 2047, 2048 and 4100 rows


@functools.lru_cache(maxsize=None)
def hand_case(F, B):
    """dict(bins, gq, hq, pos, counts) of the hand-written level-8 segments: the first and last node of the level empty, node 3 one row, node 40 exactly 2047
    rows and node 41 exactly 2048 rows -- every row of both in bin 0 (or B - 1) of feature 0 with gq = hq = 2^20, so that the node's counter is 2047 x 2^20
    (fits int32) resp. 2048 x 2^20 = 2^31 (does not: a run that is not flushed where it ends wraps, and shows; node 41 begins at position 4096 of the node order, so a run length of 2048 in place of
    2047 would hold it whole) --, node 100 holds 4100 rows (three runs), the
    other nodes share 3700 rows, and 150 rows sit at shallower heap ids.  The rows are shuffled: node order is the kernel's business.  Computed once and shared
    (callers must not change it)."""
    rng = np.random.default_rng(8000 + 10 * F + B)
    L, base = 1 << HAND_LEVEL, (1 << HAND_LEVEL) - 1
    counts = np.zeros(L, dtype=np.int64)
    counts[HAND_ONE], counts[HAND_RUN], counts[HAND_RUN1], counts[HAND_THREE] = 1, GBT_ROWS, GBT_ROWS + 1, 4100
    free = np.array([n for n in range(1, L - 1) if counts[n] == 0 and n != 7])                 # node 7 stays empty too, in the middle of a run
    below, above = free[free < HAND_RUN], free[free > HAND_RUN1]
    counts += np.bincount(below[rng.integers(0, len(below), 2048)], minlength=L)                # 2048 + 1 + 2047 rows before node 41: it begins at position 4096
    counts += np.bincount(above[rng.integers(0, len(above), 1652)], minlength=L)
    node = np.repeat(np.arange(L), counts)
    pos = np.concatenate([base + node, rng.integers(0, base, 150)]).astype(np.int32)
    N = len(pos)
    bins, gq, hq = random_rows(rng, N, F, B)
    for n, b in ((HAND_RUN, 0), (HAND_RUN1, B - 1)):
        rows = np.nonzero(pos == base + n)[0]
        bins[rows, 0], gq[rows], hq[rows] = b, 1 << R.FRAC, 1 << R.FRAC
    perm = rng.permutation(N)
    return dict(bins=bins[perm], gq=gq[perm], hq=hq[perm], pos=pos[perm], counts=counts)


def hist_bincount(bins, gq, hq, pos, level, B):
    """int64 [L, F, B, 2] of one output, written apart from gbt_cases.hist_reference (np.add.at over (row, feature) pairs): one np.bincount per feature and
    component over node x B + bin"""
    N, F = bins.shape
    L, base = 1 << level, (1 << level) - 1
    rows = np.nonzero((pos >= base) & (pos < base + L))[0]
    out = np.zeros((L, F, B, 2), dtype=np.int64)
    for f in range(F):
        at = (pos[rows].astype(np.int64) - base) * B + bins[rows, f]
        for c, q in enumerate((gq, hq)):
            plus = np.bincount(at, weights=np.maximum(q[rows], 0).astype(np.float64), minlength=L * B)        # exact: sums below 2^53
            minus = np.bincount(at, weights=np.maximum(-q[rows].astype(np.int64), 0).astype(np.float64), minlength=L * B)
            out[:, f, :, c] = (plus.astype(np.int64) - minus.astype(np.int64)).reshape(L, B)
    return out


@functools.lru_cache(maxsize=None)
def hand_reference(F, B):
    """gbt_cases.hist_reference of hand_case(F, B): int64 [256, F, B, 2], computed once and shared (callers must not change it)"""
    d = hand_case(F, B)
    return C.hist_reference(d["bins"], d["gq"][None].astype(np.int64), d["hq"][None].astype(np.int64), d["pos"][None], HAND_LEVEL, B)[0]
