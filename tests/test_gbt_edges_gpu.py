"""A second pass over the gradient-boosted tree kernels (csrc/gbt.hip, oneprot_amd/gbt.py), at the places tests/test_gbt_gpu.py does not reach: the ensemble walk
on rows the model has not seen and on hand-written trees, the gradients of every objective against fp64, partition and update with several outputs, fits whose
histograms are the sum of several work-groups, the histogram kernel with its grid capped, and cuts at 70 000 rows.

References are numpy: tests/gbt_ref.py and the fixtures of tests/gbt_cases.py, whose own checks (the walk against gbt_ref.predict_margin, the gradient bound
against the fp32 restatement, the fixtures' decision gaps, and that the inputs tell a wrong walk from the right one) run in tests/test_gbt_cpu.py.  Everything
made of integers, of decisions on them, or of the same IEEE fp32 additions on both sides is compared EXACTLY.  The bounds that are not zero:
  gradients   |q - 2^20 x fp64| <= 0.5 + 2^20 x 4 x E32 quanta, E32 the fp32 restatement's own distance from fp64 in that case (about one quantum in all)
  fit margins T x 2^-22 past one row chunk: equal structure, one fp32 leaf added per round on both sides, margins below 2, so the two roundings of a round
              differ by at most one ulp of [1, 2) = 2^-23; the bound doubles that
  held-out    the small fixtures' own 16 x MEASURED of tests/test_gbt_gpu.py
  probabilities 2^-19: sigmoid and softmax are at most eight fp32 operations on values <= 1 (subtract, exp, the sums, divide, 1 - p), each within 2^-24 of
              its exact result, at the suite's factor 4 for an fp32 evaluation in another order
Observed values are printed (-s) and recorded in DESIGN.md next to the MEASURED table."""
import numpy as np
import pytest
import torch

from oneprot_amd import gbt, hip
from tests import gbt_cases as C
from tests import gbt_ref as R
from tests.gbt_cases import DEV, FACTOR, MEASURED, assert_same_trees, cuts_of, dev, fit_device, hist_reference, run_grad, run_hist

pytestmark = pytest.mark.gpu
ONE = 1 << R.FRAC
PROBA_TOL = 2.0 ** -19
NAMES = ["logistic", "squared", "softmax", "multilabel", "sampled"]


# ================================================================================================================== 1. prediction on rows not seen in fit
def run_predict(X, feat, thr, leaf, n_trees, init):
    (N, F), (T, K, NN) = X.shape, feat.shape
    out = torch.full((N, K), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("oneprot_gbt_predict", dev(X), dev(feat), dev(thr), dev(leaf), out, N, F, K, n_trees, NN, float(init))
    return out.cpu().numpy()


@pytest.mark.parametrize("index", range(len(C.PREDICT_CASES)))
def test_predict_on_hand_written_trees(index):
    """oneprot_gbt_predict on heap trees written with numpy (nodes that stop early above garbage entries, paths to the last level) over rows that sit on a
    threshold bit for bit, +-0.0 against a threshold of +0.0, +-inf and values 3 x outside the thresholds: the same IEEE fp32 additions of the same stored leaves
    as the numpy walk, so the margins are equal and there is no tolerance"""
    d = C.predict_case(index)
    got = run_predict(d["X"], d["feat"], d["thr"], d["leaf"], d["n_trees"], d["init"])
    assert not np.isnan(got).any() and np.array_equal(got, d["want"]), (C.PREDICT_CASES[index], int((got != d["want"]).sum()))
    if d["n_trees"] == d["feat"].shape[0]:                                    # what lies below a stopped node may be anything: NaN leaves and features out of range
        feat, leaf = d["feat"].copy(), d["leaf"].copy()
        below = np.zeros(feat.shape, dtype=bool)
        for n in range(1, feat.shape[2]):
            below[..., n] = below[..., (n - 1) // 2] | (feat[..., (n - 1) // 2] < 0)
        feat[below], leaf[below] = 70000, np.float32("nan")
        assert np.array_equal(run_predict(d["X"], feat, d["thr"], leaf, d["n_trees"], d["init"]), d["want"])


@pytest.mark.parametrize("name", NAMES)
def test_prediction_of_held_out_rows(name):
    """each small fixture, fitted on the device, on 400 fresh rows (half scaled by 3, 20 with a column on one of its cuts): predict_margin is the numpy walk
    over the device's own state_dict bit for bit, it stays within the fixture's margin bound of the restatement's prediction (the structure is asserted equal), and
    predict / predict_proba agree with numpy on those margins -- the first of equal margins included"""
    ref, objective = C.reference(name), C.FIXTURES[name][0]
    model, _, _ = fit_device(name)
    assert_same_trees(model, ref, name)
    Xh = C.heldout(name)
    sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    pm_dev = model.predict_margin(Xh)
    pm = pm_dev.cpu().numpy()
    assert np.array_equal(pm, C.walk(Xh, sd["tree_feat"], sd["tree_thr"], sd["tree_leaf"], model.init_margin()))
    want = R.predict_margin(ref, Xh, objective)
    diff = float(np.abs(pm.astype(np.float64) - want.astype(np.float64)).max())
    print(f"{name}: held-out max |device margin - restatement margin| = {diff:.3e} (bound {FACTOR * MEASURED[name]:.1e})")
    assert diff <= FACTOR * MEASURED[name]
    pred = model.predict(Xh).cpu().numpy()
    m64 = pm.astype(np.float64)
    if objective == R.SQUARED:
        assert np.array_equal(pred, pm[:, 0])
        return
    proba = model.predict_proba(Xh).cpu().numpy()
    if objective == R.SOFTMAX:
        ex = np.exp(m64 - m64.max(axis=1, keepdims=True))
        assert pred.dtype == np.int64 and np.array_equal(pred, np.argmax(pm, axis=1))
        assert proba.shape == pm.shape and np.abs(proba - ex / ex.sum(axis=1, keepdims=True)).max() <= PROBA_TOL
        tied = dict(model.state_dict())                                       # class 1 gets class 0's trees: equal margins in every row, and class 0 must win them
        for key in ("tree_feat", "tree_bin", "tree_thr", "tree_leaf"):
            tied[key] = tied[key].clone()
            tied[key][:, 1] = tied[key][:, 0]
        other = gbt.XGBClassifier().load_state_dict({k: v.cpu() for k, v in tied.items()})
        tm = other.predict_margin(Xh).cpu().numpy()
        first = (tm[:, 0] == tm[:, 1]) & (tm[:, 0] >= tm[:, 2])
        tp = other.predict(Xh).cpu().numpy()
        assert (tm[:, 0] == tm[:, 1]).all() and first.sum() >= 40 and np.array_equal(tp, np.argmax(tm, axis=1)) and (tp[first] == 0).all() and not (tp == 1).any()
        return
    sig = 1.0 / (1.0 + np.exp(-m64))
    if pm.shape[1] == 1:
        assert pred.shape == (400,) and np.array_equal(pred, (pm[:, 0] > 0).astype(np.int64))
        assert proba.shape == (400, 2) and np.abs(proba[:, 1] - sig[:, 0]).max() <= PROBA_TOL and np.abs(proba[:, 0] - (1.0 - sig[:, 0])).max() <= PROBA_TOL
    else:
        assert pred.shape == (400, 5) and np.array_equal(pred, (pm > 0).astype(np.int64))
        assert proba.shape == (400, 5) and np.abs(proba - sig).max() <= PROBA_TOL


# ================================================================================================================== 2. gradients per objective
@pytest.mark.parametrize("objective,K", C.GRAD_CASES)
def test_gradients_against_fp64(objective, K):
    """oneprot_gbt_grad's softmax branch (K in {2, 3, 10}) and its logistic branch with the t / K decode (K in {1, 5, 585}) at every N around the work-group and
    with Gaussian, saturated and all-equal margins: [K, N] layout, dropped rows exactly 0, exponent 0, and every kept integer within
    0.5 + 2^20 x 4 x E32 of 2^20 x the fp64 value (tests/test_gbt_cpu.py holds the fp32 restatement inside the same bound)"""
    worst = (0.0, 0.0, 0.0)
    for label, m, y, keep in C.grad_cases(objective, K):
        n = m.shape[0]
        g64, h64, e32, bound = C.grad_reference(m, y, objective)
        gq, hq, expo = run_grad(m, y, objective, keep)
        assert tuple(gq.shape) == (K, n) and tuple(hq.shape) == (K, n) and gq.is_contiguous() and hq.is_contiguous()
        assert expo.cpu().numpy().tolist() == [0] * K, label
        gn, hn = gq.cpu().numpy().T, hq.cpu().numpy().T                       # [N, K], as the fp64 values
        assert not gn[~keep].any() and not hn[~keep].any(), label
        dg = float(np.abs(gn[keep] - 2.0 ** R.FRAC * g64[keep]).max(initial=0.0))
        dh = float(np.abs(hn[keep] - 2.0 ** R.FRAC * h64[keep]).max(initial=0.0))
        print(f"{label}: E32 {e32:.3e}, bound {bound:.3f} quanta, observed g {dg:.3f} h {dh:.3f}")
        assert dg <= bound and dh <= bound, (label, dg, dh, bound)
        worst = max(worst, (max(dg, dh), bound, e32))
    print(f"{objective} K {K}: largest observed {worst[0]:.3f} quanta under a bound of {worst[1]:.3f} (E32 {worst[2]:.3e})")


def squared_grad(m, y, keep, gmax):
    n = len(y)
    gq, hq = (torch.full((1, n), -9, dtype=torch.int32, device=DEV) for _ in range(2))
    expo = torch.full((1,), -9, dtype=torch.int32, device=DEV)
    hip.call("oneprot_gbt_grad", dev(m.reshape(n, 1), torch.float32), dev(y.reshape(n, 1), torch.float32), None, dev(keep.astype(np.uint8)), gq, hq, expo, gmax, n, 1,
             gbt.OBJECTIVES[R.SQUARED])
    return gq[0].cpu().numpy(), hq[0].cpu().numpy(), int(expo[0])


def test_squared_error_gradients_at_the_edges():
    """reg:squarederror, exact: residuals all zero (exponent 0, g = 0, h = 2^20 on kept rows), every row dropped, and a round with max |g| = 3e4 followed by one
    with 1e-6 through the SAME gmax buffer -- the second exponent is its own"""
    rng = np.random.default_rng(6)
    gmax = torch.full((1,), 0x7f000000, dtype=torch.int32, device=DEV)        # whatever the buffer held before
    for n in (1, 255, 256, 257, 5000):
        keep = rng.random(n) < 0.7
        y = rng.standard_normal(n).astype(np.float32)
        gq, hq, e = squared_grad(y.copy(), y, keep, gmax)
        assert e == 0 and not gq.any() and np.array_equal(hq, np.where(keep, ONE, 0)), n
        gq, hq, e = squared_grad(np.zeros(n, dtype=np.float32), y, np.zeros(n, dtype=bool), gmax)
        assert e == 0 and not gq.any() and not hq.any(), n
        if not keep.any():
            continue
        for scale in (3e4, 1e-6):
            t = rng.standard_normal(n).astype(np.float32)
            t *= np.float32(scale) / np.abs(t[keep]).max()
            m = np.zeros((n, 1), dtype=np.float32)
            gq, hq, e = squared_grad(m, t, keep, gmax)
            g, h = R.gradients(m, t.reshape(n, 1), R.SQUARED)
            want_e = R.exponent(g[:, 0], keep, R.SQUARED)
            wg, wh = R.quantise(g[:, 0], h[:, 0], keep, want_e)
            assert e == want_e and e == (15 if scale > 1 else -19), (n, scale, e, want_e)
            assert np.array_equal(gq, wg) and np.array_equal(hq, wh) and np.abs(wg).max() >= ONE >> 1, (n, scale)


# ================================================================================================================== 3. partition and update, called directly
def partition_case(rng, level, n, F, NN):
    """(bins uint8 [n, F], tree_feat, tree_bin int32 [3, NN], pos int32 [3, n], want, elsewhere): another hand-written tree per output (about 30 % of the nodes
    with feat = -1; the level's first node stops in output 0 and splits in output 1), a fifth of the rows parked in nodes of other levels, and the bin that
    decides planted at tree_bin, tree_bin + 1 and 255 (the bins are shared by the outputs: row i is planted for output i % 3)"""
    kc, L, base = 3, 1 << level, (1 << level) - 1
    tf = rng.integers(0, F, (kc, NN)).astype(np.int32)
    tf[rng.random((kc, NN)) < 0.3] = -1
    tf[0, base], tf[1, base] = -1, rng.integers(0, F)
    tb = rng.integers(0, 255, (kc, NN)).astype(np.int32)
    outside = np.array([v for v in range(NN) if not base <= v < base + L])
    pos = (base + rng.integers(0, L, (kc, n))).astype(np.int32)
    elsewhere = rng.random((kc, n)) < 0.2
    pos[elsewhere] = outside[rng.integers(0, len(outside), int(elsewhere.sum()))]
    bins = rng.integers(0, 256, (n, F)).astype(np.uint8)
    rows = np.arange(n)
    k_of = rows % kc
    p = pos[k_of, rows]
    f, b = tf[k_of, p], tb[k_of, p]
    for which, value in ((0, b), (1, b + 1), (2, np.full(n, 255))):
        r = rows[(f >= 0) & ((rows // kc) % 4 == which)]
        bins[r, f[r]] = value[r]
    want = pos.copy()
    for k in range(kc):
        pk = pos[k]
        fk = tf[k, pk]
        r = np.nonzero((pk >= base) & (pk < base + L) & (fk >= 0))[0]
        want[k, r] = 2 * pk[r] + 1 + (bins[r, fk[r]].astype(np.int32) > tb[k, pk[r]])
    return bins, tf, tb, pos, want, elsewhere


@pytest.mark.parametrize("level", range(6))
def test_partition_with_three_outputs(level):
    """oneprot_gbt_partition at every level with kc = 3 and another hand-written tree per output: rows in split nodes of the level move (bin == tree_bin goes
    left, tree_bin + 1 and 255 go right), rows in nodes of other levels and in nodes with feat = -1 keep their node; exact against numpy"""
    rng = np.random.default_rng(300 + level)
    for c, (n, F) in enumerate((n, F) for n in (1, 255, 256, 257, 5000) for F in (1, 7, 130)):
        NN = 127 if c % 2 else (4 << level) - 1                              # the smallest tree that has the level's children, and the deepest
        bins, tf, tb, pos, want, elsewhere = partition_case(rng, level, n, F, NN)
        if n >= 255:
            moved = want != pos
            assert moved.any() and (~moved & ~elsewhere).any() and elsewhere.any() and (want[moved] % 2 == 1).any() and (want[moved] % 2 == 0).any()
        got = dev(pos)
        hip.call("oneprot_gbt_partition", dev(bins), dev(tf), dev(tb), got, n, F, level, 3, NN)
        assert np.array_equal(got.cpu().numpy(), want), (level, n, F, NN)


def test_update_adds_into_its_own_columns_only():
    """oneprot_gbt_update with K = 7, k0 = 2, kc = 3: columns 2 .. 4 change by the fp32 add of the row's leaf, the other four keep their bits, and a node id of -1
    or of NN adds nothing"""
    rng = np.random.default_rng(31)
    K, k0, kc, NN = 7, 2, 3, 15
    for n in (1, 255, 256, 257, 5000):
        margin = rng.standard_normal((n, K)).astype(np.float32)
        leaf = (rng.uniform(0.05, 1.0, (kc, NN)) * rng.choice((-1.0, 1.0), (kc, NN))).astype(np.float32)
        pos = rng.integers(0, NN, (kc, n)).astype(np.int32)
        pos[rng.random((kc, n)) < 0.1] = -1
        pos[rng.random((kc, n)) < 0.1] = NN
        if n == 1:
            pos[:, 0] = (-1, NN, 3)
        want = margin.copy()
        for kk in range(kc):
            ok = (pos[kk] >= 0) & (pos[kk] < NN)
            want[ok, k0 + kk] = margin[ok, k0 + kk] + leaf[kk, pos[kk, ok]]
        got = dev(margin)
        hip.call("oneprot_gbt_update", got, dev(pos), dev(leaf), n, K, k0, kc, NN)
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), n
        assert np.array_equal(got[:, [0, 1, 5, 6]].view(np.int32), margin[:, [0, 1, 5, 6]].view(np.int32))
        if n >= 255:
            assert (pos == -1).any() and (pos == NN).any() and (got[:, 2:5] != margin[:, 2:5]).any()


# ================================================================================================================== 4. fits past one row chunk
def fit_big(name):
    X, y = C.big_data(name)
    objective = C.BIG_FIXTURES[name][0]
    kw = dict(C.BIG_PARAMS, objective=objective)
    if name == "sampled":
        kw.update(subsample=C.SAMPLE_RATE, colsample_bytree=C.SAMPLE_RATE, random_state=C.SAMPLE_SEED)
    cls = gbt.XGBRegressor if objective == R.SQUARED else gbt.XGBClassifier
    return cls(**kw).fit(X, y), X


def same_bits(a, b):
    return torch.equal(a.train_margin_, b.train_margin_) and all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))


@pytest.mark.parametrize("name", NAMES)
def test_fit_of_three_row_chunks_against_the_restatement(name, monkeypatch):
    """N = 4500 = 2047 + 2047 + 406 rows: every histogram of the fit is the sum of three work-groups' int64 atomics.  Tree structure exactly the restatement's;
    the squared-error margin bit-equal, the others within T x 2^-22 (margins below 2: see the module docstring); predict_margin of the training rows bit-equal to
    the margin fit ended with; a second fit, and for the multi-label fixture a fit of one output per histogram chunk, give the same bits"""
    ref = C.big_reference(name)
    model, X = fit_big(name)
    assert_same_trees(model, ref, f"4500 rows, {name}")
    got, want = model.train_margin_.cpu().numpy(), ref["margin"]
    assert float(np.abs(want).max()) < 2.0
    diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    bound = 0.0 if name == "squared" else C.BIG_ROUNDS * 2.0 ** -22
    print(f"4500 rows, {name}: max |device margin - restatement margin| = {diff:.3e} (bound {bound:.1e})")
    assert diff <= bound
    assert torch.equal(model.predict_margin(X), model.train_margin_)
    assert same_bits(fit_big(name)[0], model)
    if name == "multilabel":
        monkeypatch.setenv("ONEPROT_GBT_HIST_BYTES", str((1 << (C.BIG_DEPTH - 1)) * C.BIG_F * C.BIG_B * 16))
        assert gbt.plan_chunks(5, C.BIG_F, C.BIG_B, C.BIG_DEPTH) == [(k, k + 1) for k in range(5)]
        assert same_bits(fit_big(name)[0], model)


# ================================================================================================================== 5. the histogram kernel with its grid capped
def test_histogram_with_the_grid_capped():
    """level 5, F = 1280, max_bin 2, kc = 328 outputs, N = 40 x 2047 - 5: 640 feature tiles x 328 outputs leave room for 19 work-groups along the 40 row
    chunks, so a work-group takes chunks x, x + 19, x + 38 and clears its LDS tile in between.  All outputs share one (gq, hq, pos) pattern with full-scale
    entries; every output equals one np.bincount histogram (exact in fp64 below 2^53), compared on the device; a second launch equals the first"""
    level, F, B, kc, n = 5, 1280, 2, 328, 40 * 2047 - 5
    L, base, ft = 1 << level, (1 << level) - 1, 64 >> level
    gy, chunks = -(-F // ft), -(-n // 2047)
    cap = ((1 << 22) - 1) // (gy * kc)
    assert (gy * kc, cap, chunks, -(-chunks // cap)) == (209920, 19, 40, 3)
    g = torch.Generator(device=DEV).manual_seed(50)
    bins = torch.randint(0, B, (n, F), dtype=torch.uint8, device=DEV, generator=g)
    gq = torch.randint(-ONE, ONE + 1, (n,), dtype=torch.int32, device=DEV, generator=g)
    hq = torch.randint(0, ONE + 1, (n,), dtype=torch.int32, device=DEV, generator=g)
    gq[::5] = torch.where(gq[::5] < 0, -ONE, ONE)                             # |g| = 1 ...
    hq[::5] = 0                                                               # ... with h = 0
    pos = torch.randint(base, base + L, (n,), dtype=torch.int32, device=DEV, generator=g)
    pos[::11] = 5                                                             # rows that stopped above: not of this level
    bt = bins.t().contiguous().cpu().numpy()                                  # [F, N]
    gn, hn, pn = gq.cpu().numpy().astype(np.float64), hq.cpu().numpy().astype(np.float64), pos.cpu().numpy().astype(np.int64)
    rows = np.nonzero((pn >= base) & (pn < base + L))[0]
    node = (pn[rows] - base) * B
    want = np.zeros((L, F, B, 2), dtype=np.int64)
    for f in range(F):
        idx = node + bt[f, rows]
        want[:, f, :, 0] = np.bincount(idx, weights=gn[rows], minlength=L * B).reshape(L, B)
        want[:, f, :, 1] = np.bincount(idx, weights=hn[rows], minlength=L * B).reshape(L, B)
    assert np.array_equal(want[:, :3], hist_reference(bt[:3].T.copy(), gn[None].astype(np.int64), hn[None].astype(np.int64), pn[None], level, B)[0])
    d = [bins] + [t.expand(kc, n).contiguous() for t in (gq, hq, pos)]
    got = run_hist(*d, level, B)
    wd = dev(want)
    assert tuple(got.shape) == (kc, L, F, B, 2) and bool((got == wd[None]).all())
    assert torch.equal(run_hist(*d, level, B), got)


# ================================================================================================================== 6. cuts and bins at size
@pytest.mark.parametrize("B", [3, 256])
def test_cuts_and_bins_at_70000_rows(B):
    """build_cuts past the 2049 x 33 elements of the first pass: a column of ten distinct integers, one of +-0.0 and a Gaussian one; cuts bit for bit (a cut at
    zero is +0.0), bins exactly gbt_ref.make_cuts'"""
    rng = np.random.default_rng(70)
    n = 70000
    X = rng.standard_normal((n, 3)).astype(np.float32)
    X[:, 0] = rng.integers(-4, 6, n)
    X[:, 1] = rng.choice(np.array([-0.0, 0.0], dtype=np.float32), n)
    assert len(np.unique(X[:, 0])) == 10 and np.signbit(X[:, 1]).any() and not np.signbit(X[:, 1]).all()
    want_cuts, want_bins = R.make_cuts(X, B)
    cuts, ncuts, bins = gbt.build_cuts(dev(X), B)
    got = cuts_of(cuts, ncuts)
    for f in range(3):
        assert np.array_equal(got[f].view(np.int32), want_cuts[f].view(np.int32)), (B, f)
        assert np.isinf(cuts[f, int(ncuts[f]):].cpu().numpy()).all()
    assert len(want_cuts[1]) == 1 and len(want_cuts[0]) == min(B - 1, 10) and len(want_cuts[2]) == B - 1
    assert np.array_equal(bins.cpu().numpy(), want_bins)
