"""The gradient-boosted tree probes on the device (csrc/gbt.hip, oneprot_amd/gbt.py) against the independent restatement tests/gbt_ref.py.

Cuts, bins, quantised gradients, histograms, node ids, tree structure and leaf values are integers or decisions on integers and are compared EXACTLY.  Gains
are fp64 on both sides and agree to 1e-12 relative.  Margins differ by the fp32 `exp` of the device against numpy's and the fp32 chain on top of it; their bound
is 16 x the largest |device - restatement| measured once on an MI355X per objective (MEASURED below): a few ulp per round, with room for
another exp implementation and none for a wrong leaf (a leaf value here is ~0.1).  The end-to-end fixtures decide every split by a relative gain gap of at
least 1e-4 (tests/test_gbt_cpu.py::test_fixture_gaps), so equal structure is a fair demand."""
import json
import math

import numpy as np
import pytest
import torch

from oneprot_amd import gbt, hip
from tests import gbt_cases as C
from tests import gbt_ref as R
from tests.gbt_cases import DEV, FACTOR, MEASURED, assert_same_trees, cuts_of, dev, fit_device, hist_reference, run_grad, run_hist

pytestmark = pytest.mark.gpu
# ================================================================================================================== cuts / bins
def special_columns(X, rng):
    """a constant column, a column of 3 distinct values, a column of +-0.0 and values around them -- wherever the matrix is wide enough"""
    N, F = X.shape
    if F >= 7:
        X[:, 1] = 2.5
        X[:, 3] = rng.choice(np.array([-1.0, 0.25, 7.0], dtype=np.float32), N)
        X[:, 5] = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0], dtype=np.float32), N)
    elif N >= 2:
        X[::2, 0] = -0.0
        X[1::2, 0] = 0.0
    return X


@pytest.mark.parametrize("B", [2, 16, 256])
def test_cuts_and_bins_exact(B):
    rng = np.random.default_rng(11)
    for N in (1, 2, 255, 256, 257, 2049):
        for F in (1, 7, 33):
            X = special_columns(rng.standard_normal((N, F)).astype(np.float32), rng)
            want_cuts, want_bins = R.make_cuts(X, B)
            cuts, ncuts, bins = gbt.build_cuts(dev(X), B)
            got = cuts_of(cuts, ncuts)
            for f in range(F):
                assert np.array_equal(got[f].view(np.int32), want_cuts[f].view(np.int32)), (N, F, B, f)      # bits: a cut at zero is +0.0
                assert np.isinf(cuts[f, int(ncuts[f]):].cpu().numpy()).all()
            assert np.array_equal(bins.cpu().numpy(), want_bins), (N, F, B)
            if F >= 7:
                assert int(ncuts[1]) == 1 and int(ncuts[3]) <= 3


# ================================================================================================================== gradients
def test_gradients_at_the_extremes():
    """|g| = 1 with h = 0 (a saturated logistic), a regression round whose max |g| is 3e4 and another at 1e-6; dropped rows are 0; exact integers"""
    rng = np.random.default_rng(5)
    N = 777
    keep = rng.random(N) < 0.7
    m = np.where(rng.random((N, 1)) < 0.5, 100.0, -100.0).astype(np.float32)
    y = (m[:, 0] < 0).astype(np.float32)
    gq, hq, expo = run_grad(m, y, R.LOGISTIC, keep)
    g, h = R.gradients(m, y.reshape(N, 1), R.LOGISTIC)
    wg, wh = R.quantise(g[:, 0], h[:, 0], keep, 0)
    assert np.array_equal(gq[0].cpu().numpy(), wg) and np.array_equal(hq[0].cpu().numpy(), wh) and int(expo[0]) == 0
    assert set(np.abs(wg[keep])) == {1 << R.FRAC} and not wh.any() and not gq[0].cpu().numpy()[~keep].any()
    for scale in (3e4, 1e-6):
        y = rng.standard_normal(N).astype(np.float32)
        m = np.zeros((N, 1), dtype=np.float32)
        y *= np.float32(scale) / np.abs(y[keep]).max()
        y[~keep] *= 10                                                        # a dropped row does not set the exponent
        gq, hq, expo = run_grad(m, y, R.SQUARED, keep)
        g, h = R.gradients(m, y.reshape(N, 1), R.SQUARED)
        e = R.exponent(g[:, 0], keep, R.SQUARED)
        wg, wh = R.quantise(g[:, 0], h[:, 0], keep, e)
        assert int(expo[0]) == e and 2.0 ** (e - 1) <= np.abs(g[keep, 0]).max() < 2.0 ** e
        assert np.array_equal(gq[0].cpu().numpy(), wg) and np.array_equal(hq[0].cpu().numpy(), wh)
        assert np.abs(wg).max() >= 1 << (R.FRAC - 1) and set(wh[keep]) == {1 << R.FRAC}


# ================================================================================================================== histograms
def node_layout(N, level, rng):
    """pos [N] over the nodes of a level (and a few rows parked at nodes of other levels): node 1 of the level empty and node 2 holding a single row when the
    level has them and there are rows enough"""
    L, base = 1 << level, (1 << level) - 1
    pos = rng.integers(0, L, N)
    if L >= 4:
        pos[pos == 1] = 0
        pos[pos == 2] = 3
        if N >= 8:
            pos[N // 2] = 2
    pos = pos + base
    if N >= 16:
        pos[rng.random(N) < 0.1] = max(base - 1, 0) if level else 5          # rows that stopped at a leaf above (or sit elsewhere): not of this level
    return pos


@pytest.mark.parametrize("level", [0, 2, 5])
def test_histograms_exact(level):
    """1, 4 and 32 nodes; every row count around the wave, the work-group's row quota (2047) and beyond; feature counts around the 64-wide tile; K in {1, 3};
    gradients up to the fixed point's extremes (|q| = 2^20); two runs equal; one output per launch equals all outputs in one"""
    rng = np.random.default_rng(100 + level)
    for N in (1, 63, 64, 65, 2047, 2049, 5000):
        for F in (1, 7, 33, 130):
            for K, B in ((1, 256), (3, 16)):
                bins = rng.integers(0, B, (N, F)).astype(np.uint8)
                gq = rng.integers(-(1 << R.FRAC), (1 << R.FRAC) + 1, (K, N)).astype(np.int32)
                hq = rng.integers(0, (1 << R.FRAC) + 1, (K, N)).astype(np.int32)
                gq[:, ::5] = np.where(rng.random(gq[:, ::5].shape) < 0.5, 1 << R.FRAC, -(1 << R.FRAC))          # |g| = 1 ...
                hq[:, ::5] = 0                                                                             # ... with h = 0
                pos = np.stack([node_layout(N, level, rng) for _ in range(K)]).astype(np.int32)
                want = hist_reference(bins, gq.astype(np.int64), hq.astype(np.int64), pos, level, B)
                d = [dev(a) for a in (bins, gq, hq, pos)]
                got = run_hist(*d, level, B)
                assert np.array_equal(got.cpu().numpy(), want), (N, F, K, B)
                assert torch.equal(run_hist(*d, level, B), got)
                if K > 1:
                    one = torch.stack([run_hist(d[0], d[1][k:k + 1], d[2][k:k + 1], d[3][k:k + 1], level, B)[0] for k in range(K)])
                    assert torch.equal(one, got)


def test_histogram_all_rows_at_full_scale_do_not_overflow():
    """2047 rows (a work-group's whole quota) of |q| = 2^20 in ONE bin: the int32 LDS counter holds 2047 x 2^20 < 2^31; 5000 such rows take three work-groups"""
    for N in (2047, 5000):
        bins = np.zeros((N, 3), dtype=np.uint8)
        gq = np.full((1, N), -(1 << R.FRAC), dtype=np.int32)
        hq = np.full((1, N), 1 << R.FRAC, dtype=np.int32)
        got = run_hist(dev(bins), dev(gq), dev(hq), dev(np.zeros((1, N), dtype=np.int32)), 0, 4).cpu().numpy()
        assert (got[0, 0, :, 0, 0] == -N * (1 << R.FRAC)).all() and (got[0, 0, :, 0, 1] == N * (1 << R.FRAC)).all() and not got[0, 0, :, 1:].any()


def test_histogram_at_the_largest_row_count():
    """N = 2^24, the contract's limit: 8,197 row chunks, row offsets past 2^24 F bytes; sums by integer masks"""
    N, F, B = 1 << 24, 2, 4
    g = torch.Generator(device=DEV).manual_seed(4)
    bins = torch.randint(0, B, (N, F), dtype=torch.uint8, device=DEV, generator=g)
    gq = torch.randint(-(1 << R.FRAC), (1 << R.FRAC) + 1, (1, N), dtype=torch.int32, device=DEV, generator=g)
    hq = torch.randint(0, (1 << R.FRAC) + 1, (1, N), dtype=torch.int32, device=DEV, generator=g)
    pos = torch.randint(1, 3, (1, N), dtype=torch.int32, device=DEV, generator=g)
    got = run_hist(bins, gq, hq, pos, 1, B).cpu().numpy()
    bn, gn, hn, pn = bins.cpu().numpy(), gq[0].cpu().numpy().astype(np.int64), hq[0].cpu().numpy().astype(np.int64), pos[0].cpu().numpy()
    for n in range(2):
        for f in range(F):
            for b in range(B):
                m = (pn == 1 + n) & (bn[:, f] == b)
                assert got[0, n, f, b, 0] == gn[m].sum() and got[0, n, f, b, 1] == hn[m].sum(), (n, f, b)


# ================================================================================================================== split search
def run_split(H, ncuts, keep, expo, level, B, D, **params):
    """H int64 [K, L, F, B, 2] -> (feat, bin, thr, leaf, gain) numpy arrays [K, NN]"""
    K, L, F = H.shape[:3]
    NN = (2 << D) - 1
    cuts = torch.arange(F * (B - 1), dtype=torch.float32, device=DEV).view(F, B - 1).contiguous()
    tf = torch.full((K, NN), -5, dtype=torch.int32, device=DEV)
    tb, tt, tl = torch.zeros_like(tf), torch.zeros(K, NN, device=DEV), torch.zeros(K, NN, device=DEV)
    gain = torch.zeros(K * NN * 8, dtype=torch.uint8, device=DEV)
    p = dict(min_child_weight=1.0, gamma=0.0, reg_alpha=0.0, reg_lambda=1.0, learning_rate=0.3)
    p.update(params)
    ws = torch.empty(hip.query("oneprot_gbt_split_workspace", F, level, K), dtype=torch.uint8, device=DEV)
    assert ws.numel() == K * L * F * 48
    hip.call("oneprot_gbt_split", dev(H), cuts, dev(np.asarray(ncuts, dtype=np.int32)), dev(np.asarray(keep, dtype=np.uint8)), dev(np.asarray(expo, dtype=np.int32)), tf, tb, tt,
             tl, gain, ws, ws.numel(), F, B, level, K, NN, p["min_child_weight"], p["gamma"], p["reg_alpha"], p["reg_lambda"], p["learning_rate"])
    return tf.cpu().numpy(), tb.cpu().numpy(), tt.cpu().numpy(), tl.cpu().numpy(), gain.view(torch.float64).view(K, NN).cpu().numpy(), cuts.cpu().numpy()


def random_hist(rng, K, level, F, B, N, e=0):
    """integer histograms of a random binned data set, nodes of the level filled unevenly (node 1 empty when there is one)"""
    L = 1 << level
    ncuts = rng.integers(1, B, F)
    bins = np.stack([rng.integers(0, ncuts[f] + 1, N) for f in range(F)], axis=1).astype(np.uint8)
    H = np.zeros((K, L, F, B, 2), dtype=np.int64)
    for k in range(K):
        g = rng.standard_normal(N).astype(np.float32) * np.float32(0.3 * 2.0 ** e)
        h = rng.uniform(0.05, 0.25, N).astype(np.float32)
        gq, hq = R.quantise(g, h, np.ones(N, dtype=bool), e)
        pos = rng.integers(0, L, N)
        if L > 1:
            pos[pos == 1] = 0
        for n in range(L):
            H[k, n] = R.histogram(bins, gq, hq, np.nonzero(pos == n)[0], B)
    return H, ncuts


def check_split(H, ncuts, keep, expo, level, B, D, label, **params):
    """every node against the restatement; returns (nodes compared, nodes skipped below the gap)"""
    tf, tb, tt, tl, gain, cuts = run_split(H, ncuts, keep, expo, level, B, D, **params)
    rp = {k: v for k, v in params.items() if k != "learning_rate"}
    lr = float(np.float32(params.get("learning_rate", 0.3)))
    alpha, lam = float(np.float32(params.get("reg_alpha", 0.0))), float(np.float32(params.get("reg_lambda", 1.0)))
    K, L = H.shape[:2]
    seen = skipped = 0
    for k in range(K):
        sg, sh = math.ldexp(1.0, int(expo[k]) - R.FRAC), math.ldexp(1.0, -R.FRAC)
        for n in range(L):
            nid = L - 1 + n
            d = R.best_split(H[k, n], ncuts, keep, int(expo[k]), **rp)
            seen += 1
            assert tl[k, nid] == np.float32(lr * R.weight(d["G"] * sg, d["H"] * sh, alpha, lam)), (label, k, n)
            if not d["valid"]:
                assert tf[k, nid] == -1 and gain[k, nid] == -math.inf, (label, k, n)
                continue
            assert abs(gain[k, nid] - d["gain"]) <= 1e-12 * abs(d["gain"]), (label, k, n, gain[k, nid], d["gain"])
            if d["gap"] < 1e-9:
                skipped += 1
                continue
            if d["split"]:
                assert (tf[k, nid], tb[k, nid]) == (d["f"], d["j"]), (label, k, n)
                assert tt[k, nid] == cuts[d["f"], d["j"]]
                assert tl[k, 2 * nid + 1] == np.float32(lr * R.weight(d["GL"] * sg, d["HL"] * sh, alpha, lam))
                assert tl[k, 2 * nid + 2] == np.float32(lr * R.weight((d["G"] - d["GL"]) * sg, (d["H"] - d["HL"]) * sh, alpha, lam))
            else:
                assert tf[k, nid] == -1 and tl[k, 2 * nid + 1] == 0 and tl[k, 2 * nid + 2] == 0, (label, k, n)
            assert tf[k, 2 * nid + 1] == -1 and tf[k, 2 * nid + 2] == -1
    return seen, skipped


def test_split_search_against_the_restatement():
    """from integer histograms handed in, so both sides see the same input: the chosen (feature, cut) wherever the restatement's gap is >= 1e-9, gains to 1e-12
    relative, leaf values to the fp32 rounding of the fp64 value; at most 5 % of the nodes may fall below the gap"""
    rng = np.random.default_rng(21)
    seen = skipped = 0
    for level, F, B, K, e, params in ((0, 1, 2, 1, 0, {}), (0, 300, 16, 2, 0, {}), (2, 33, 256, 3, 0, dict(reg_lambda=10.0, learning_rate=0.1)), (5, 7, 16, 1, 0, {}),
                                      (3, 20, 32, 2, 15, dict(reg_alpha=0.1, gamma=0.1)), (1, 9, 8, 1, -19, dict(min_child_weight=5.0)), (4, 130, 64, 1, 0, dict(reg_lambda=0.0)), (5, 40, 16, 1, 0, dict(reg_lambda=10.0, min_child_weight=3.0))):
        H, ncuts = random_hist(rng, K, level, F, B, 400 << level, e)
        keep = rng.random(F) < 0.8
        keep[rng.integers(0, F)] = True
        a, b = check_split(H, ncuts, keep, [e] * K, level, B, max(level + 1, 3), f"level {level} F {F} B {B}", **params)
        seen, skipped = seen + a, skipped + b
    print(f"split: {seen} nodes, {skipped} below the 1e-9 gap")
    assert seen >= 100 and skipped <= 0.05 * seen


def test_split_corner_cases():
    one = 1 << R.FRAC
    H = np.zeros((1, 2, 3, 4, 2), dtype=np.int64)                              # level 1: node 0 filled, node 1 without rows
    H[0, 0, :, 0] = (-3 * one, 3 * one)
    H[0, 0, :, 2] = (2 * one, 2 * one)
    H[0, 0, 0] = 0
    H[0, 0, 0, 1] = (-one, 5 * one)                                            # feature 0 holds every row in one bin: no valid cut; features 1 and 2 are identical
    ncuts, keep = [3, 3, 3], [True, True, True]
    for label, params in (("ties", {}), ("min_child_weight", dict(min_child_weight=2.5)), ("gamma", dict(gamma=10.0)), ("alpha", dict(reg_alpha=2.5)),
                          ("lambda 0", dict(reg_lambda=0.0))):
        seen, skipped = check_split(H, ncuts, keep, [0], 1, 4, 2, label, **params)
        assert (seen, skipped) == (2, 0)
    tf, tb, tt, tl, gain, _ = run_split(H, ncuts, keep, [0], 1, 4, 2)
    assert (tf[0, 1], tb[0, 1]) == (1, 0) and tf[0, 2] == -1 and gain[0, 2] == -math.inf and tl[0, 2] == 0       # the lower of two identical features; the empty node
    assert run_split(H, ncuts, [True, False, True], [0], 1, 4, 2)[0][0, 1] == 2
    assert run_split(H, ncuts, keep, [0], 1, 4, 2, min_child_weight=2.5)[0][0, 1] == -1
    assert run_split(H, ncuts, keep, [0], 1, 4, 2, gamma=10.0)[0][0, 1] == -1
    g = run_split(H, ncuts, keep, [0], 1, 4, 2, reg_alpha=2.5)[4][0, 1]
    assert abs(g - 0.0625) <= 1e-15


# ================================================================================================================== partition / leaf / predict, end to end
@pytest.mark.parametrize("name", ["logistic", "squared", "softmax", "multilabel", "sampled"])
def test_end_to_end_against_the_restatement(name):
    """tree structure exactly the restatement's; the final margin within 16 x the measured rounding difference; predict_margin of the training rows bit-equal to
    the margin fit ended with; a state_dict round trip and a second seeded fit give the same bits"""
    ref = C.reference(name)
    model, X, y = fit_device(name)
    assert_same_trees(model, ref, name)
    diff = float(np.abs(model.train_margin_.cpu().numpy().astype(np.float64) - ref["margin"].astype(np.float64)).max())
    print(f"{name}: max |device margin - restatement margin| = {diff:.3e} (measured {MEASURED[name]:.1e}, bound {FACTOR * MEASURED[name]:.1e})")
    assert diff <= FACTOR * MEASURED[name]
    pm = model.predict_margin(X)
    assert torch.equal(pm, model.train_margin_)
    again, _, _ = fit_device(name)
    assert torch.equal(again.train_margin_, model.train_margin_) and all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), model.state_dict().values()))
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    other = type(model)().load_state_dict(sd)
    assert torch.equal(other.predict_margin(X), pm)
    if name == "logistic":
        proba = model.predict_proba(X)
        assert proba.shape == (C.N, 2) and torch.equal(model.predict(X), (proba[:, 1] > 0.5).long())
        one = type(model)(**dict(C.PARAMS, objective=R.LOGISTIC, subsample=1.0, colsample_bytree=1.0, random_state=99)).fit(X, y)
        assert torch.equal(one.train_margin_, model.train_margin_)            # rates of 1.0 draw nothing: the bits of a fit without sampling, whatever the seed
    if name == "softmax":
        assert model.predict_proba(X).shape == (C.N, 3) and torch.equal(model.predict(X), pm.argmax(1))
    if name == "multilabel":
        assert model.predict(X).shape == (C.N, 5) and model.predict_proba(X).shape == (C.N, 5)
    if name == "squared":
        assert torch.equal(model.predict(X), pm[:, 0])


def test_histogram_budget_does_not_change_a_bit(monkeypatch):
    """one output per chunk (the smallest budget that admits one) against all outputs in one chunk"""
    whole, X, y = fit_device("multilabel")
    monkeypatch.setenv("ONEPROT_GBT_HIST_BYTES", str((1 << (C.DEPTH - 1)) * C.F * C.B * 16))
    assert len(gbt.plan_chunks(5, C.F, C.B, C.DEPTH)) == 5
    chunked, _, _ = fit_device("multilabel")
    assert torch.equal(chunked.train_margin_, whole.train_margin_) and all(torch.equal(a, b) for a, b in zip(chunked.state_dict().values(), whole.state_dict().values()))
    monkeypatch.setenv("ONEPROT_GBT_HIST_BYTES", "1000")
    with pytest.raises(ValueError):
        fit_device("multilabel")


@pytest.mark.parametrize("depth", [1, 6])
def test_node_ids_leaves_and_prediction(depth):
    """one round by hand through the entry points: node ids of every row exact after every level, leaf values the fp32 rounding of the restatement's fp64 value,
    and the fitted model's prediction of its training rows bit-equal to its final margin"""
    X, y = C.data("logistic")
    ref = R.fit(X, y, R.LOGISTIC, n_estimators=2, max_depth=depth, max_bin=C.B, learning_rate=0.3)
    model = gbt.XGBClassifier(n_estimators=2, max_depth=depth, max_bin=C.B, learning_rate=0.3).fit(X, y)
    assert_same_trees(model, ref, f"depth {depth}")
    leaf = model.state_dict()["tree_leaf"].cpu().numpy()
    for t in range(2):
        tr = ref["trees"][t][0]
        reached = np.unique(tr["pos"])
        assert np.array_equal(leaf[t, 0][reached], tr["leaf"][reached])
    assert torch.equal(model.predict_margin(X), model.train_margin_)
    # the first round's node ids, level by level
    xd = dev(X)
    cuts, ncuts, bins = gbt.build_cuts(xd, C.B)
    N, F, NN = C.N, C.F, (2 << depth) - 1
    keep_r, keep_f = torch.ones(N, dtype=torch.uint8, device=DEV), torch.ones(F, dtype=torch.uint8, device=DEV)
    gq, hq, expo = run_grad(np.zeros((N, 1), dtype=np.float32), y, R.LOGISTIC)
    pos = torch.zeros(1, N, dtype=torch.int32, device=DEV)
    tf = torch.full((1, NN), -1, dtype=torch.int32, device=DEV)
    tb, tt, tl = torch.zeros_like(tf), torch.zeros(1, NN, device=DEV), torch.zeros(1, NN, device=DEV)
    hist = torch.empty(hip.query("oneprot_gbt_hist_bytes", F, C.B, depth - 1) // 8, dtype=torch.int64, device=DEV)
    ws = torch.empty(hip.query("oneprot_gbt_split_workspace", F, depth - 1, 1), dtype=torch.uint8, device=DEV)
    want = np.zeros(N, dtype=np.int64)
    tr = ref["trees"][0][0]
    for level in range(depth):
        hip.call("oneprot_gbt_hist", bins, gq, hq, pos, hist, N, F, C.B, level, 1)
        hip.call("oneprot_gbt_split", hist, cuts, ncuts, keep_f, expo, tf, tb, tt, tl, None, ws, ws.numel(), F, C.B, level, 1, NN, 1.0, 0.0, 0.0, 1.0, 0.3)
        hip.call("oneprot_gbt_partition", bins, tf, tb, pos, N, F, level, 1, NN)
        at = (want >= (1 << level) - 1) & (tr["feat"][want] >= 0)
        want[at] = 2 * want[at] + 1 + (ref["bins"][at, tr["feat"][want[at]]] > tr["bin"][want[at]])
        assert np.array_equal(pos[0].cpu().numpy(), want), level
    assert np.array_equal(want, tr["pos"])
    margin = torch.zeros(N, 1, device=DEV)
    hip.call("oneprot_gbt_update", margin, pos, tl, N, 1, 0, 1, NN)
    assert np.array_equal(margin[:, 0].cpu().numpy(), tr["leaf"][tr["pos"]])


def test_sampling_masks_equal_the_host_rebuild():
    """the row and feature masks of a round against tests/philox_ref.py; keep frequencies at N = 20 000 within 5 sigma of the rate"""
    N, F, seed = 20000, 1280, C.SAMPLE_SEED
    rows, feats = C.sampling_masks(N, F, 3, seed, 0.8, 0.8)
    for t in range(3):
        rk, fk, fu = torch.empty(N, dtype=torch.uint8, device=DEV), torch.empty(F, dtype=torch.uint8, device=DEV), torch.empty(F, dtype=torch.int32, device=DEV)
        hip.call("oneprot_gbt_sample", rk, fk, fu, N, F, 0.8, R.n_keep_features(F, 0.8), seed, gbt.stream_of(t), gbt.stream_of(3 + t))
        assert np.array_equal(rk.cpu().numpy().astype(bool), rows[t]) and np.array_equal(fk.cpu().numpy().astype(bool), feats[t])
        assert abs(rows[t].mean() - 0.8) < 5 * math.sqrt(0.8 * 0.2 / N) and int(fk.sum()) == 1024
    hip.call("oneprot_gbt_sample", rk, fk, fu, N, F, 1.0, F, seed, gbt.stream_of(0), gbt.stream_of(3))
    assert bool(rk.all()) and bool(fk.all())


# ================================================================================================================== one realistic shape; the task groups
def test_realistic_shape_log_loss_falls_every_round():
    N, F, T = 4096, 1280, 10
    g = torch.Generator().manual_seed(3)
    X = torch.randn(N, F, generator=g)
    w = torch.randn(F, generator=g)
    y = ((X @ w) / math.sqrt(F) + 0.3 * torch.randn(N, generator=g) > 0).float()
    model = gbt.XGBClassifier(n_estimators=T, max_depth=5, learning_rate=0.3, max_bin=256).fit(X.to(DEV), y)
    s, yd = model._state, y.to(DEV).double()
    losses = []
    for t in range(T + 1):
        m = torch.empty(N, 1, device=DEV)
        hip.call("oneprot_gbt_predict", X.to(DEV), s["tree_feat"], s["tree_thr"], s["tree_leaf"], m, N, F, 1, t, model.tree_nodes, 0.0)
        m = m[:, 0].double()
        losses.append(float((torch.nn.functional.softplus(m) - yd * m).mean()))
    print("log-loss per round:", " ".join(f"{v:.4f}" for v in losses))
    assert abs(losses[0] - math.log(2)) < 1e-12 and all(b < a for a, b in zip(losses, losses[1:]))
    assert torch.equal(m.float(), model.train_margin_[:, 0])
    assert float(((model.predict(X) == y.long().to(DEV)).float().mean())) > 0.7


def write_embeddings(root, task, target_of, rng, F=24):
    """synthetic embeddings of one task in load_data's file layout: <root>/esm2/<task>/<partition>/<task>_<partition>_embeddings_labels.pt"""
    for part, n in (("train", 240), ("valid", 80), ("test", 80)):
        X = rng.standard_normal((n, F)).astype(np.float32)
        d = root / "esm2" / task / part
        d.mkdir(parents=True)
        torch.save({"embeddings": torch.from_numpy(X), "labels_fitness": torch.from_numpy(target_of(X))}, d / f"{task}_{part}_embeddings_labels.pt")


def test_evaluate_returns_the_reference_keys_for_every_task_group(tmp_path):
    """synthetic embeddings in load_data's file layout; one task of each of the four groups, through evaluate (labels, as the reference) and scores="proba\""""
    rng = np.random.default_rng(9)
    F = 24
    W = rng.standard_normal((F, 6))
    write = lambda task, target_of: write_embeddings(tmp_path, task, target_of, rng, F)
    write("HumanPPI", lambda X: (X @ W[:, 0] > 0).astype(np.int64))
    write("EC", lambda X: (X @ W > 0).astype(np.float32))
    write("ThermoStability", lambda X: (X @ W[:, 1]).astype(np.float32))
    write("DeepLoc10", lambda X: np.argmax(X @ W[:, :4], axis=1).astype(np.int64))
    keys = {"HumanPPI": ("accuracy", "f1_micro", "auc"), "EC": ("f1_max",), "ThermoStability": ("mse", "r2", "spearman_rho"), "DeepLoc10": ("accuracy", "f1_micro")}
    for task, ks in keys.items():
        reg = task == "ThermoStability"
        cfg = {"task_name": task, "model_type": "esm2", "emb_dir": str(tmp_path), "evaluate_on": ["train", "valid", "test"], "threshold": math.inf,
               "downstream_model": {"_target_": "xgboost.XGBRegressor" if reg else "xgboost.XGBClassifier", "name": "x", "n_estimators": 20, "max_depth": 3,
                                    "learning_rate": 0.3, "objective": "reg:squarederror" if reg else "binary:logistic", "booster": "gbtree", "tree_method": "gpu_hist",
                                    "n_jobs": -1, "max_bin": 32}}
        data = gbt.load_data(cfg)
        res = gbt.evaluate(cfg, data)
        assert set(res) == {f"{p}_{k}" for p in ("valid", "test") for k in ks}, task
        assert all(isinstance(v, float) and math.isfinite(v) for v in res.values()), (task, res)
        assert gbt.evaluate.last.objective == gbt.objective_of(task)
        print(task, json.dumps(res))
        if task == "HumanPPI":
            assert res["test_accuracy"] > 0.6 and res["test_auc"] > 0.6
            soft = gbt.evaluate(cfg, data, scores="proba")
            assert soft["test_accuracy"] == res["test_accuracy"] and 0.6 < soft["test_auc"] <= 1.0            # (labels make a three-point ROC curve)
        if task == "ThermoStability":
            assert res["test_r2"] > 0.0
        if task == "DeepLoc10":
            assert res["test_accuracy"] > 0.4                                   # four classes
        if task == "EC":
            assert 0.0 < res["test_f1_max"] <= 1.0 and set(gbt.evaluate(cfg, data, scores="proba")) == set(res)


def test_command_line_prints_one_json_row(tmp_path, capsys):
    """python src/saprot_fit_cls.py --one task_name=HumanPPI emb_dir=... (and the regressor's twin), in process: one JSON row with the reference's keys"""
    from src import saprot_fit_cls, saprot_fit_reg
    rng = np.random.default_rng(10)
    w = rng.standard_normal(24)
    write_embeddings(tmp_path, "HumanPPI", lambda X: (X @ w > 0).astype(np.int64), rng)
    write_embeddings(tmp_path, "ThermoStability", lambda X: (X @ w).astype(np.float32), rng)
    saprot_fit_cls.main(["--one", "task_name=HumanPPI", f"emb_dir={tmp_path}", "downstream_model.n_estimators=10"])
    row = json.loads(capsys.readouterr().out.strip())
    assert set(row) == {"task_name", "model_type"} | {f"{p}_{k}" for p in ("valid", "test") for k in ("accuracy", "f1_micro", "auc")} and row["task_name"] == "HumanPPI"
    saprot_fit_reg.main(["--one", f"emb_dir={tmp_path}", "downstream_model.n_estimators=10", "downstream_model.subsample=0.8"])
    row = json.loads(capsys.readouterr().out.strip())
    assert set(row) == {"task_name", "model_type"} | {f"{p}_{k}" for p in ("valid", "test") for k in ("mse", "r2", "spearman_rho")} and row["task_name"] == "ThermoStability"


def test_host_refusals():
    with pytest.raises(ValueError):
        gbt.XGBRegressor(n_estimators=1, max_depth=1).fit(np.array([[1.0, float("nan")]], dtype=np.float32), np.array([0.0], dtype=np.float32))
    with pytest.raises(ValueError):
        gbt.XGBRegressor(n_estimators=1, max_depth=1).fit(np.array([[1.0, float("inf")]], dtype=np.float32), np.array([0.0], dtype=np.float32))
    with pytest.raises(hip.HipKernelError):                                    # CPU tensors at the kernel boundary
        hip.call("oneprot_gbt_cuts", torch.zeros(4), 4, 1, 2, torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    one = gbt.XGBRegressor(n_estimators=2, max_depth=2).fit(np.array([[3.0]], dtype=np.float32), np.array([1.5], dtype=np.float32))      # N = 1, F = 1
    assert one.predict(np.array([[3.0]], dtype=np.float32)).shape == (1,)
