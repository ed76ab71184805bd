"""The end-to-end fixtures of the gradient-boosted tree tests and the host rebuild of a fit's sampling masks.  A helper module like tests/gbt_ref.py, not a
test.  Every fixture is N = 300, F = 8, max_bin 16, depth 3, 5 rounds on Gaussian features of numpy's default_rng; tests/test_gbt_cpu.py asserts that the
restatement's decision gap on each of them is at least 1e-4, so that no fixture asks the device to reproduce a coin toss.  Below them: the same recipes at
4500 rows, and the inputs and numpy references of tests/test_gbt_edges_gpu.py (hand-written trees and rows for the ensemble walk, held-out rows, gradient
cases with their fp64 values), each checked without a GPU in tests/test_gbt_cpu.py."""
import functools

import numpy as np
import torch

from oneprot_amd import gbt, hip
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


def _recipe(name, seed, n, f):
    """the data recipe of a fixture name at any size"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f)).astype(np.float32)
    if name in ("logistic", "sampled"):
        y = ((X @ rng.standard_normal(f) + 0.5 * rng.standard_normal(n)) > 0).astype(np.float32)
    elif name == "squared":
        y = (np.sin(X[:, 0]) + X[:, 1] * X[:, 2]).astype(np.float32)
    elif name == "softmax":
        y = np.argmax(X @ rng.standard_normal((f, 3)) + 0.5 * rng.standard_normal((n, 3)), axis=1).astype(np.int64)
    else:
        y = ((X @ rng.standard_normal((f, 5)) + 0.5 * rng.standard_normal((n, 5))) > 0).astype(np.float32)
    return X, y


def data(name):
    """(X fp32 [N, F], y) of a fixture"""
    return _recipe(name, FIXTURES[name][1], N, F)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's fit of a fixture, computed once and shared (callers must not change it)"""
    X, y = data(name)
    kw = {}
    if name == "sampled":
        kw["row_masks"], kw["feat_masks"] = sampling_masks(N, F, ROUNDS, SAMPLE_SEED, SAMPLE_RATE, SAMPLE_RATE)
    return R.fit(X, y, FIXTURES[name][0], **PARAMS, **kw)


# ================================================================================================================== fixtures past one row chunk
# N = 4500 is three row chunks of the histogram kernel (2047 + 2047 + 406): a histogram there is the sum of several work-groups' int64 atomics.  The data
# recipes are those of the small fixtures.  Depth 6 at this size has exact cross-partition ties on every seed tried and is not asked for.
BIG_N, BIG_F, BIG_B, BIG_DEPTH, BIG_ROUNDS = 4500, 12, 32, 4, 3
BIG_PARAMS = dict(n_estimators=BIG_ROUNDS, max_depth=BIG_DEPTH, max_bin=BIG_B, learning_rate=0.3)
BIG_FIXTURES = {"logistic": (R.LOGISTIC, 1), "squared": (R.SQUARED, 1), "softmax": (R.SOFTMAX, 4), "multilabel": (R.LOGISTIC, 6), "sampled": (R.LOGISTIC, 3)}
BIG_GAPS = {"logistic": 7.56e-4, "squared": 2.28e-3, "softmax": 4.23e-4, "multilabel": 6.08e-4, "sampled": 2.32e-3}        # as the restatement reported them (3 digits)


def big_data(name):
    return _recipe(name, BIG_FIXTURES[name][1], BIG_N, BIG_F)


@functools.lru_cache(maxsize=None)
def big_reference(name):
    """the restatement's fit of a 4500-row fixture, computed once and shared (callers must not change it)"""
    X, y = big_data(name)
    kw = {}
    if name == "sampled":
        kw["row_masks"], kw["feat_masks"] = sampling_masks(BIG_N, BIG_F, BIG_ROUNDS, SAMPLE_SEED, SAMPLE_RATE, SAMPLE_RATE)
    return R.fit(X, y, BIG_FIXTURES[name][0], **BIG_PARAMS, **kw)


# ================================================================================================================== the ensemble walk on rows not seen in fit
def walk(X, feat, thr, leaf, init, n_trees=None, le=False):
    """fp32 [N, K]: the level-synchronous walk of heap trees feat / thr / leaf [T, K, NN] over raw rows: a node with feat < 0 is where a row stays, x < thr goes
    left, and one fp32 add per tree in round order.  Written apart from gbt_ref.predict_margin (a loop per row), which it must equal bit for bit.  le=True is the
    WRONG rule x <= thr, kept so that a test can show that its inputs tell the two apart."""
    X = np.asarray(X, dtype=np.float32)
    T, K, NN = feat.shape
    depth = (NN + 1).bit_length() - 2
    n = X.shape[0]
    rows = np.arange(n)
    m = np.full((n, K), np.float32(init), dtype=np.float32)
    for t in range(T if n_trees is None else n_trees):
        for k in range(K):
            p = np.zeros(n, dtype=np.int64)
            for _ in range(depth):
                f = feat[t, k, p]
                live = f >= 0
                x = X[rows, np.where(live, f, 0)]
                left = (x <= thr[t, k, p]) if le else (x < thr[t, k, p])
                p = np.where(live, 2 * p + 2 - left, p)
            m[:, k] = m[:, k] + leaf[t, k, p]
    return m


def pack_trees(model):
    """(feat int32, thr fp32, leaf fp32) [T, K, NN] of a gbt_ref.fit result"""
    return tuple(np.stack([np.stack([tr[key] for tr in rnd]) for rnd in model["trees"]]) for key in ("feat", "thr", "leaf"))


# (depth, K, stored T, n_trees, F, N, init_margin): every depth in {1, 3, 6}, K in {1, 3, 5}, T in {0, 1, 7} (no tree is walked with n_trees = 0: an empty
# tensor has no address to hand over, so the arrays hold one tree), a prefix of the stored trees once, F in {1, 8, 1280}, N in {1, 255, 256, 257, 70 001}
PREDICT_CASES = ((1, 1, 1, 1, 1, 1, 0.0), (3, 3, 7, 7, 8, 255, 0.5), (6, 5, 7, 7, 1280, 257, -1.25), (6, 1, 7, 4, 8, 70001, 0.3), (3, 5, 1, 1, 8, 256, 0.0),
                 (1, 3, 7, 7, 1, 257, 2.0), (6, 3, 1, 0, 8, 255, 0.7), (6, 5, 7, 7, 8, 70001, -0.5), (1, 5, 7, 7, 1280, 1, 0.25), (6, 3, 7, 7, 1, 256, 0.0),
                 (3, 1, 1, 1, 1280, 257, 1.5))


def synthetic_trees(rng, T, K, depth, F):
    """(feat, feat_full, thr, leaf) [T, K, NN] written by hand: random features, N(0, 1) thresholds of which some are +0.0, non-zero leaves at EVERY node; about a
    fifth of the nodes above the last level stop (feat = -1) and whatever lies below them is left as it was drawn -- garbage that must never be read.  Tree (0, 0)
    stops nowhere, so some paths run to the last level; the root of the last tree stops when there is more than one tree.  feat_full is feat without the
    stops: walking it reads below stopped nodes, the mistake a test must be able to see."""
    NN, inner = (2 << depth) - 1, (1 << depth) - 1
    feat_full = rng.integers(0, F, (T, K, NN)).astype(np.int32)
    thr = rng.standard_normal((T, K, NN)).astype(np.float32)
    thr[rng.random(thr.shape) < 0.15] = 0.0
    leaf = (rng.uniform(0.05, 1.0, (T, K, NN)) * rng.choice((-1.0, 1.0), (T, K, NN))).astype(np.float32)
    stopped = rng.random((T, K, NN)) < 0.2
    stopped[..., inner:] = True
    stopped[0, 0, :inner] = False
    if T * K > 1:
        stopped[-1, -1, 0] = True
    return np.where(stopped, -1, feat_full).astype(np.int32), feat_full, thr, leaf


@functools.lru_cache(maxsize=None)
def predict_case(index):
    """dict(X, feat, feat_full, thr, leaf, n_trees, init, want) of PREDICT_CASES[index], computed once and shared (callers must not change it).  X is N(0, 1)
    overwritten by row number modulo 8: 0 a value equal, bit for bit, to the threshold of a node of a walked tree (half of them roots, which every row reaches) in that
    node's feature; 1 and 2 a -0.0 and a +0.0 in the feature of a node whose threshold is +0.0; 3 and 4 +inf and -inf; 5 a row of 3 x the largest |threshold|, with
    either sign; 6 and 7 stay Gaussian."""
    depth, K, T, n_trees, F, n, init = PREDICT_CASES[index]
    rng = np.random.default_rng(500 + index)
    feat, feat_full, thr, leaf = synthetic_trees(rng, T, K, depth, F)
    X = rng.standard_normal((n, F)).astype(np.float32)
    kind = np.arange(n) % 8
    lt, lk, ln = np.nonzero(feat[:max(n_trees, 1)] >= 0)
    if len(lt):
        r0 = np.nonzero(kind == 0)[0]
        roots = np.nonzero(ln == 0)[0]
        j = rng.integers(0, len(lt), len(r0))
        j[::2] = roots[rng.integers(0, len(roots), len(j[::2]))]
        X[r0, feat[lt[j], lk[j], ln[j]]] = thr[lt[j], lk[j], ln[j]]
        zeros = np.nonzero(thr[lt, lk, ln] == 0.0)[0]
        for which, value in ((1, -0.0), (2, 0.0)):
            r = np.nonzero(kind == which)[0]
            j = zeros[rng.integers(0, len(zeros), len(r))] if len(zeros) else rng.integers(0, len(lt), len(r))
            X[r, feat[lt[j], lk[j], ln[j]]] = np.float32(value)
    for which, value in ((3, np.inf), (4, -np.inf)):
        r = np.nonzero(kind == which)[0]
        X[r, rng.integers(0, F, len(r))] = np.float32(value)
    r = np.nonzero(kind == 5)[0]
    X[r] = np.float32(3.0) * np.abs(thr).max() * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), (len(r), F))
    return dict(X=X, feat=feat, feat_full=feat_full, thr=thr, leaf=leaf, n_trees=n_trees, init=init, want=walk(X, feat, thr, leaf, init, n_trees))


def heldout(name):
    """400 fresh rows of a small fixture: default_rng(1000 + seed), the second half scaled by 3, and in each of the first 20 rows one column set to one of that
    feature's cuts (the restatement's, which the device's are asserted equal to)"""
    rng = np.random.default_rng(1000 + FIXTURES[name][1])
    X = rng.standard_normal((400, F)).astype(np.float32)
    X[200:] *= np.float32(3.0)
    cuts = reference(name)["cuts"]
    for i in range(20):
        f = int(rng.integers(0, F))
        X[i, f] = cuts[f][int(rng.integers(0, len(cuts[f])))]
    return X


# ================================================================================================================== gradients per objective against fp64
GRAD_CASES = ((R.SOFTMAX, 2), (R.SOFTMAX, 3), (R.SOFTMAX, 10), (R.LOGISTIC, 1), (R.LOGISTIC, 5), (R.LOGISTIC, 585))
GRAD_NS = (1, 255, 256, 257, 5000)
GRAD_FACTOR = 4.0              # the suite's yardstick for an fp32 evaluation in another order (tests/test_probe_gpu.py FACTOR)


def gradients64(m, y, objective):
    """gbt_ref.gradients' formulas evaluated in fp64 from the fp32 margin"""
    m = np.asarray(m, dtype=np.float64)
    if objective == R.SQUARED:
        return m - np.asarray(y, dtype=np.float64), np.ones_like(m)
    if objective == R.LOGISTIC:
        p = 1.0 / (1.0 + np.exp(-m))
        return p - np.asarray(y, dtype=np.float64), p * (1.0 - p)
    ex = np.exp(m - m.max(axis=1, keepdims=True))
    p = ex / ex.sum(axis=1, keepdims=True)
    onehot = (np.arange(m.shape[1])[None, :] == np.asarray(y).reshape(-1, 1)).astype(np.float64)
    return p - onehot, 2.0 * p * (1.0 - p)


def grad_cases(objective, K):
    """yields (label, margin fp32 [N, K], y, keep bool [N]): every N of GRAD_NS x three kinds of margin (N(0, 2); a saturated mix of +-100, +-30 and +-0.5; all
    equal) under a keep mask of rate 0.7, then N = 257 with every row kept and with every row dropped.  Softmax labels hold class 0 and class K - 1."""
    todo = [(n, kind, 0.7) for n in GRAD_NS for kind in ("normal", "saturated", "equal")] + [(257, "normal", 1.0), (257, "normal", 0.0)]
    for c, (n, kind, rate) in enumerate(todo):
        rng = np.random.default_rng(7000 + 100 * K + c)
        if kind == "normal":
            m = (2.0 * rng.standard_normal((n, K))).astype(np.float32)
        elif kind == "saturated":
            m = rng.choice(np.array([100.0, -100.0, 30.0, -30.0, 0.5, -0.5], dtype=np.float32), (n, K))
        else:
            m = np.full((n, K), 0.75, dtype=np.float32)
        if objective == R.SOFTMAX:
            y = rng.integers(0, K, n).astype(np.int64)
            y[0], y[-1] = 0, (K - 1 if n > 1 or c % 2 else 0)
        else:
            y = (rng.random((n, K)) < 0.5).astype(np.float32)
        yield f"{objective} K {K} N {n} {kind} keep {rate}", m, y, rng.random(n) < rate


def grad_reference(m, y, objective):
    """(g64, h64, E32, bound in quanta): the fp64 gradients [N, K], the largest |fp32 restatement - fp64| of the case floored at 2^-24, and the bound
    0.5 + 2^20 x 4 x E32 on |q - 2^20 x fp64| (half a quantum of rint plus the fp32 evaluation's own error at the suite's factor)"""
    g32, h32 = R.gradients(m, y, objective)
    g64, h64 = gradients64(m, y, objective)
    e32 = max(float(np.abs(g32 - g64).max()), float(np.abs(h32 - h64).max()), 2.0 ** -24)
    return g64, h64, e32, 0.5 + 2.0 ** R.FRAC * GRAD_FACTOR * e32


# ================================================================================================================== launches and gates the GPU files share
DEV = "cuda:0"
# largest |device margin - restatement margin| over the rounds of every end-to-end fixture, measured on an MI355X (printed by the tests with -s); the
# regression fixture has no exp in its chain and every operation of it is a single IEEE fp32 operation on both sides: it is exact
MEASURED = {"logistic": 1.192e-7, "squared": 0.0, "softmax": 2.384e-7, "multilabel": 2.384e-7, "sampled": 3.576e-7}       # 1, 0, 2, 2 and 3 x 2^-23
FACTOR = 16.0


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return t.to(DEV, dtype).contiguous() if dtype is not None else t.to(DEV).contiguous()


def cuts_of(cuts, ncuts):
    cuts, ncuts = cuts.cpu().numpy(), ncuts.cpu().numpy()
    return [cuts[f, :ncuts[f]] for f in range(len(ncuts))]


def run_grad(m, y, objective, keep=None):
    N, K = m.shape
    md = dev(m, torch.float32)
    keep = np.ones(N, dtype=np.uint8) if keep is None else keep.astype(np.uint8)
    gq, hq = (torch.empty(K, N, dtype=torch.int32, device=DEV) for _ in range(2))
    expo, gmax = torch.empty(K, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    if objective == R.SOFTMAX:
        hip.call("oneprot_gbt_grad", md, None, dev(y, torch.int32), dev(keep), gq, hq, expo, gmax, N, K, 2)
    else:
        hip.call("oneprot_gbt_grad", md, dev(y.reshape(N, K), torch.float32), None, dev(keep), gq, hq, expo, gmax, N, K, gbt.OBJECTIVES[objective])
    return gq, hq, expo


def hist_reference(bins, gq, hq, pos, level, B):
    """int64 [K, L, F, B, 2]: every (row, feature) adds its row's integers at (node, feature, bin) -- one np.add.at per output and component"""
    K, (N, F) = gq.shape[0], bins.shape
    L, base = 1 << level, (1 << level) - 1
    out = np.zeros((K, L, F, B, 2), dtype=np.int64)
    for k in range(K):
        rows = np.nonzero((pos[k] >= base) & (pos[k] < base + L))[0]
        flat = ((pos[k][rows, None].astype(np.int64) - base) * F + np.arange(F)[None, :]) * B + bins[rows].astype(np.int64)
        for c, q in enumerate((gq[k], hq[k])):
            acc = np.zeros(L * F * B, dtype=np.int64)
            np.add.at(acc, flat.reshape(-1), np.repeat(q[rows], F))
            out[k, ..., c] = acc.reshape(L, F, B)
    return out


def run_hist(bins, gq, hq, pos, level, B):
    K, N = gq.shape
    F = bins.shape[1]
    hist = torch.full((K, 1 << level, F, B, 2), -7, dtype=torch.int64, device=DEV)       # overwritten, not accumulated
    assert hip.query("oneprot_gbt_hist_bytes", F, B, level) * K == hist.numel() * 8
    hip.call("oneprot_gbt_hist", bins, gq, hq, pos, hist, N, F, B, level, K)
    return hist


def fit_device(name, **over):
    X, y = data(name)
    objective = FIXTURES[name][0]
    kw = dict(PARAMS, objective=objective)
    if name == "sampled":
        kw.update(subsample=SAMPLE_RATE, colsample_bytree=SAMPLE_RATE, random_state=SAMPLE_SEED)
    kw.update(over)
    cls = gbt.XGBRegressor if objective == R.SQUARED else gbt.XGBClassifier
    return cls(**kw).fit(X, y), X, y


def assert_same_trees(model, ref, label):
    s = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    for t, rnd in enumerate(ref["trees"]):
        for k, tr in enumerate(rnd):
            assert np.array_equal(s["tree_feat"][t, k], tr["feat"]), (label, t, k, s["tree_feat"][t, k], tr["feat"])
            split = tr["feat"] >= 0
            assert np.array_equal(s["tree_bin"][t, k][split], tr["bin"][split]) and np.array_equal(s["tree_thr"][t, k][split], tr["thr"][split]), (label, t, k)
    got = cuts_of(model._state["cuts"], model._state["ncuts"])
    assert all(np.array_equal(a, b) for a, b in zip(got, ref["cuts"]))
