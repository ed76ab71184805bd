"""The host side of the gradient-boosted tree probes (oneprot_amd/gbt.py) and the restatement tests/gbt_ref.py, without a GPU: the restatement on cases with a
known answer, the decision gap of every end-to-end fixture the GPU tests use, the sampling rule, the constructor surface, `_target_` resolution, the yaml
files and scripts, and the header / binding of the new entry points."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import yaml

from oneprot_amd import gbt, hip
from tests import gbt_cases as C
from tests import gbt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("oneprot_gbt_cuts", "oneprot_gbt_bin", "oneprot_gbt_sample", "oneprot_gbt_grad", "oneprot_gbt_hist_bytes", "oneprot_gbt_hist", "oneprot_gbt_split_workspace", "oneprot_gbt_split",
                "oneprot_gbt_partition", "oneprot_gbt_update", "oneprot_gbt_predict")


def test_stump_recovers_the_separating_cut():
    """two clusters on feature 1 of 3, labels by cluster: the one split of a depth-1 tree is on feature 1 at a cut between the clusters, and it separates them"""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((200, 3)).astype(np.float32)
    X[:100, 1] = rng.uniform(-3.0, -1.0, 100)
    X[100:, 1] = rng.uniform(1.0, 3.0, 100)
    y = (np.arange(200) >= 100).astype(np.float32)
    m = R.fit(X, y, R.LOGISTIC, n_estimators=1, max_depth=1, max_bin=16)
    tr = m["trees"][0][0]
    assert tr["feat"][0] == 1
    assert X[:100, 1].max() < tr["thr"][0] <= X[100:, 1].min()
    assert tr["leaf"][1] < 0 < tr["leaf"][2]                                   # left = class 0: the margin goes down
    assert np.array_equal(tr["pos"], np.where(y > 0, 2, 1))
    assert np.array_equal(R.predict_margin(m, X, R.LOGISTIC), m["margin"])     # the walk on raw rows equals the fit's margin, bit for bit


@pytest.mark.parametrize("eta,lam", [(0.3, 1.0), (1.0, 0.0), (0.05, 10.0)])
def test_squared_error_training_loss_falls_every_round(eta, lam):
    """provable for reg:squarederror, subsample 1, 0 < eta <= 1, lambda >= 0: a leaf changes its rows' summed loss by -eta (1 - eta / 2) G^2 / (H + lambda) or less"""
    X, y = C.data("squared")
    m = R.fit(X, y, R.SQUARED, n_estimators=8, max_depth=3, max_bin=16, learning_rate=eta, reg_lambda=lam)
    mse = [float(np.mean((mm[:, 0].astype(np.float64) - y) ** 2)) for mm in m["margins"]]
    start = float(np.mean((0.5 - y.astype(np.float64)) ** 2))
    assert all(b < a for a, b in zip([start] + mse[:-1], mse)), mse


@pytest.mark.parametrize("name", sorted(C.FIXTURES))
def test_fixture_gaps(name):
    """every end-to-end fixture of tests/test_gbt_gpu.py decides its splits by a relative gain gap of at least 1e-4 (recorded: tests/gbt_cases.py GAPS), and is
    not vacuous: every round splits its root"""
    m = C.reference(name)
    print(f"{name}: gap {m['gap']:.3e} (recorded {C.GAPS[name]:.3e})")
    assert m["gap"] >= 1e-4
    assert abs(m["gap"] - C.GAPS[name]) <= 0.01 * C.GAPS[name]
    assert all(tr["feat"][0] >= 0 for rnd in m["trees"] for tr in rnd)
    assert len(m["trees"]) == C.ROUNDS and len(m["trees"][0]) == {"softmax": 3, "multilabel": 5}.get(name, 1)


def test_split_rule_corner_cases():
    """the restatement on hand-made integer histograms: min_child_weight, gamma, reg_alpha, ties between identical columns, an empty node"""
    one = 1 << R.FRAC
    H = np.zeros((2, 4, 2), dtype=np.int64)
    H[:, 0] = (-3 * one, 3 * one)                                              # bin 0: three rows of g = -1, h = 1
    H[:, 2] = (2 * one, 2 * one)                                               # bin 2: two rows of g = +1
    ncuts, keep = [3, 3], [True, True]
    d = R.best_split(H, ncuts, keep, 0, min_child_weight=1.0, reg_lambda=1.0)
    assert d["valid"] and d["split"] and (d["f"], d["j"]) == (0, 0)            # identical columns, cuts 0 and 1 give equal sums: lowest feature, lowest cut
    assert math.isclose(d["gain"], 9 / 4 + 4 / 3 - 1 / 6, rel_tol=1e-15)
    assert R.best_split(H, ncuts, [False, True], 0)["f"] == 1
    assert not R.best_split(H, ncuts, keep, 0, min_child_weight=2.5)["valid"]  # the right side holds H = 2
    d = R.best_split(H, ncuts, keep, 0, gamma=10.0)
    assert d["valid"] and not d["split"]
    d = R.best_split(H, ncuts, keep, 0, reg_alpha=2.5)                         # T(-3) = -0.5, T(2) = 0, T(-1) = 0
    assert math.isclose(d["gain"], 0.25 / 4, rel_tol=1e-15)
    assert not R.best_split(np.zeros_like(H), ncuts, keep, 0)["valid"]
    assert R.weight(0.0, 0.0, 0.0, 0.0) == 0.0


def test_cuts_and_bins_rule():
    X = np.array([[0.0, 5.0], [-0.0, 5.0], [1.0, 5.0], [2.0, 5.0]], dtype=np.float32)
    cuts, bins = R.make_cuts(X, 4)
    assert [c.tolist() for c in cuts] == [[0.0, 1.0, 2.0], [5.0]]
    assert not np.signbit(cuts[0][0])
    assert bins[:, 0].tolist() == [1, 1, 2, 3] and bins[:, 1].tolist() == [1, 1, 1, 1]
    for x, b in zip(X[:, 0], bins[:, 0]):                                     # bin <= j iff x < cut[j]
        assert all((b <= j) == (x < cuts[0][j]) for j in range(3))


def test_sampling_rule():
    s = C.slices16(20000, C.SAMPLE_SEED, C.stream_of(3))
    assert s.min() >= 0 and s.max() < 65536
    keep = R.row_mask_from_slices(s, 0.8)
    assert abs(keep.mean() - 0.8) < 5 * math.sqrt(0.8 * 0.2 / 20000)
    assert R.row_mask_from_slices(s, 1.0).all()
    fm = R.feat_mask_from_slices(np.array([5, 1, 5, 1, 9]), 0.6)
    assert fm.tolist() == [True, True, False, True, False]                     # the 3 smallest, equal uniforms to the lower index
    assert R.feat_mask_from_slices(np.array([5, 1]), 0.1).sum() == 1
    assert gbt.stream_of(7) == C.stream_of(7) == (6 << 60) | 7 and gbt.RNG_DOMAIN_GBT == 6


def test_constructor_keywords_defaults_and_refusals():
    m = gbt.XGBClassifier()
    p = m.get_params()
    assert (p["n_estimators"], p["max_depth"], p["learning_rate"], p["reg_lambda"], p["reg_alpha"], p["gamma"], p["min_child_weight"]) == (100, 6, 0.3, 1.0, 0.0, 0.0, 1.0)
    assert (p["subsample"], p["colsample_bytree"], p["base_score"], p["max_bin"], p["objective"]) == (1.0, 1.0, 0.5, 256, "binary:logistic")
    assert gbt.XGBRegressor().objective == "reg:squarederror"
    m = gbt.XGBClassifier(name="XGBClassifier", n_estimators=250, max_depth=5, learning_rate=0.1, objective="multi:softmax", booster="gbtree", tree_method="gpu_hist",
                          n_jobs=-1, min_child_weight=5, gamma=0.1, subsample=0.8, colsample_bytree=0.8, reg_alpha=0.1, reg_lambda=10, eval_metric="rmse", base_score=0.5,
                          max_bin=64, random_state=3, something_else=1)
    assert m.kwargs == {"name": "XGBClassifier", "something_else": 1} and m.get_params()["name"] == "XGBClassifier" and m.tree_method == "gpu_hist"
    assert m.tree_nodes == 63 and m.init_margin() == 0.5
    assert gbt.XGBClassifier().init_margin() == 0.0 and abs(gbt.XGBClassifier(base_score=0.25).init_margin() - math.log(1 / 3)) < 1e-6
    for bad in (dict(booster="gblinear"), dict(booster="dart"), dict(max_depth=9), dict(max_depth=0), dict(objective="rank:pairwise")):
        with pytest.raises(NotImplementedError):
            gbt.XGBClassifier(**bad)
    for bad in (dict(max_bin=1), dict(max_bin=257), dict(subsample=0.0), dict(colsample_bytree=1.5), dict(reg_lambda=-1.0), dict(n_estimators=0)):
        with pytest.raises(ValueError):
            gbt.XGBRegressor(**bad)
    with pytest.raises(RuntimeError):
        gbt.XGBRegressor().predict(np.zeros((2, 2), dtype=np.float32))


def test_plan_chunks_and_budget(monkeypatch):
    per = 16 * 1280 * 256 * 16
    assert gbt.plan_chunks(585, 1280, 256, 5, budget=1 << 30) == [(k, min(585, k + (1 << 30) // per)) for k in range(0, 585, (1 << 30) // per)]
    assert gbt.plan_chunks(3, 7, 16, 3, budget=4 * 7 * 16 * 16) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError):
        gbt.plan_chunks(3, 7, 16, 3, budget=4 * 7 * 16 * 16 - 1)
    monkeypatch.setenv("ONEPROT_GBT_HIST_BYTES", "12345")
    assert gbt.hist_bytes_budget() == 12345
    monkeypatch.delenv("ONEPROT_GBT_HIST_BYTES")
    assert gbt.hist_bytes_budget() == 1 << 30


def test_target_resolution_objective_rule_and_yaml_files():
    for fname, cls, target in (("xgboost_cls.yaml", gbt.XGBClassifier, "xgboost.XGBClassifier"), ("xgboost_reg.yaml", gbt.XGBRegressor, "xgboost.XGBRegressor")):
        with open(os.path.join(ROOT, "configs", "downstream_model", fname)) as f:
            dm = yaml.safe_load(f)
        assert dm["_target_"] == target
        model = gbt.build_model({"task_name": "ThermoStability" if cls is gbt.XGBRegressor else "DeepLoc10", "downstream_model": dm})
        assert type(model) is cls and model.max_depth == 3 and model.n_estimators == 100 and model.learning_rate == 0.1 and model.kwargs["name"] == dm["name"]
    assert model.objective == "reg:squarederror"
    with open(os.path.join(ROOT, "configs", "downstream_model", "xgboost_cls.yaml")) as f:
        dm = yaml.safe_load(f)
    want = {"HumanPPI": "binary:logistic", "MetalIonBinding": "binary:logistic", "DeepLoc2": "binary:logistic", "EC": "binary:logistic", "GO-BP": "binary:logistic",
            "ThermoStability": "reg:squarederror", "DeepLoc10": "multi:softmax", "TopEnzyme": "multi:softmax"}
    for task, obj in want.items():
        assert gbt.objective_of(task) == obj
        if obj != "reg:squarederror":
            assert gbt.build_model({"task_name": task, "downstream_model": dm}).objective == obj         # ref saprot_fit_cls.py:23-30 overrides the yaml's objective
    with pytest.raises(ValueError):
        gbt.build_model({"task_name": "EC", "downstream_model": {"_target_": "sklearn.ensemble.RandomForestClassifier"}})
    for fname in ("saprot_sweep_xgboost_cls.yaml", "saprot_sweep_xgboost_reg.yaml"):
        with open(os.path.join(ROOT, "configs", fname)) as f:
            cfg = yaml.safe_load(f)
        assert set(cfg["sweep"]) <= set(gbt.SWEEP_KEYS) and cfg["sweep"]["reg_lambda"] == [10] and all(d <= gbt.MAX_DEPTH for d in cfg["sweep"]["max_depth"])
        assert os.path.exists(os.path.join(ROOT, "configs", "downstream_model", cfg["downstream_model"] + ".yaml"))
        assert cfg["evaluate_on"] == ["train", "valid", "test"] and math.isinf(cfg["threshold"])


def test_scripts_import_without_xgboost_hydra_or_sklearn():
    import sys
    before = set(sys.modules)
    cls = importlib.import_module("src.saprot_fit_cls")
    reg = importlib.import_module("src.saprot_fit_reg")
    assert cls.XGBClassifier is gbt.XGBClassifier and reg.XGBRegressor is gbt.XGBRegressor and cls.evaluate is gbt.evaluate and callable(cls.main) and callable(reg.main)
    new = {m.split(".")[0] for m in set(sys.modules) - before}
    assert not new & {"xgboost", "hydra", "sklearn", "omegaconf"}


def test_header_declares_every_symbol_gbt_calls():
    assert hip.ABI_VERSION == 7
    src = open(gbt.__file__).read()
    called = set(re.findall(r'"(oneprot_\w+)"', src))
    assert {n for n in called if n.startswith("oneprot_gbt_")} == set(ENTRY_POINTS)
    assert called <= set(hip._SIGS)
    header = open(hip.HEADER_PATH).read()
    for name in ENTRY_POINTS:
        assert name in hip._SIGS and re.search(r"\b" + name + r"\s*\(", header)
    assert hip._PTR_DTYPES["oneprot_gbt_hist"] == "biiil"
    assert hip._PTR_DTYPES["oneprot_gbt_bin"] == "ffib"
    assert hip._PTR_DTYPES["oneprot_gbt_split"] == "lfibiiiffbb"
    assert hip._PTR_DTYPES["oneprot_gbt_sample"] == "bbi"
    assert hip._PTR_DTYPES["oneprot_gbt_grad"] == "ffibiiii"
    for section in ("saprot_fit_cls.py:32-38", "saprot_fit_reg.py:26-32", "xgboost_cls.yaml", "xgboost_reg.yaml"):
        assert section in header


# ================================================================================================================== the fixtures and references of tests/test_gbt_edges_gpu.py
@pytest.mark.parametrize("name", sorted(C.BIG_FIXTURES))
def test_big_fixture_gaps(name):
    """the 4500-row fixtures (three row chunks of the histogram kernel) under test_fixture_gaps' condition: every split decided by a relative gain gap of at
    least 1e-4, every round splitting its root; and the largest margin stays below 2, which the GPU test's bound of one ulp in [1, 2) per round rests on"""
    m = C.big_reference(name)
    print(f"{name}: gap {m['gap']:.3e} (recorded {C.BIG_GAPS[name]:.3e}), max |margin| {np.abs(m['margin']).max():.3f}")
    assert m["gap"] >= 1e-4
    assert abs(m["gap"] - C.BIG_GAPS[name]) <= 0.01 * C.BIG_GAPS[name]
    assert all(tr["feat"][0] >= 0 for rnd in m["trees"] for tr in rnd)
    assert len(m["trees"]) == C.BIG_ROUNDS and len(m["trees"][0]) == {"softmax": 3, "multilabel": 5}.get(name, 1)
    assert m["bins"].shape == (C.BIG_N, C.BIG_F) and C.BIG_N > 2 * 2047 and float(np.abs(m["margin"]).max()) < 2.0


@pytest.mark.parametrize("name", sorted(C.FIXTURES))
def test_vectorised_walk_equals_the_restatement_on_held_out_rows(name):
    """tests/gbt_cases.py walk (level-synchronous, the reference of the GPU prediction tests) against gbt_ref.predict_margin (a loop per row) on 200 rows the
    300-row fit has not seen: rows that sit on a cut, rows scaled by 3; bit for bit"""
    ref, objective = C.reference(name), C.FIXTURES[name][0]
    X = np.concatenate([C.heldout(name)[:100], C.heldout(name)[200:300]])
    feat, thr, leaf = C.pack_trees(ref)
    want = R.predict_margin(ref, X, objective)
    got = C.walk(X, feat, thr, leaf, R.initial_margin(objective, 0.5))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    cuts = ref["cuts"]
    assert sum(bool((X[i, f] == cuts[f]).any()) for i in range(20) for f in range(C.F)) >= 20       # the rows on a cut are there
    assert np.abs(X[100:]).max() > np.abs(X[:100]).max()


@pytest.mark.parametrize("index", range(len(C.PREDICT_CASES)))
def test_predict_inputs_tell_the_wrong_walks_apart(index):
    """on the X of every synthetic prediction case, a walk with <= in place of < and a walk that reads below a stopped node give other margins than the right
    walk -- wherever the case has the rows to show it (a single row is not asked to show both)"""
    depth, K, T, n_trees, F, n, init = C.PREDICT_CASES[index]
    d = C.predict_case(index)
    assert d["want"].shape == (n, K) and d["feat"].shape == (T, K, (2 << depth) - 1)
    inner = (1 << depth) - 1
    assert (d["feat"][0, 0, :inner] >= 0).all() and (d["feat"][..., inner:] == -1).all() and (d["leaf"] != 0).all() and (d["feat_full"] >= 0).all()
    if n_trees == 0:
        assert (d["want"] == np.float32(init)).all()
        return
    X = d["X"]
    live = d["feat"][:n_trees] >= 0
    assert np.isin(X, d["thr"][:n_trees][live]).any()
    if n >= 255:
        assert np.isposinf(X).any() and np.isneginf(X).any() and (X[np.signbit(X)] == 0).any() and np.abs(X).max() >= 3 * np.abs(d["thr"]).max()
        le = C.walk(X, d["feat"], d["thr"], d["leaf"], init, n_trees, le=True)
        assert (le != d["want"]).any()
        if n_trees * K > 1:
            through = C.walk(X, d["feat_full"], d["thr"], d["leaf"], init, n_trees)
            assert (through != d["want"]).any()


def test_predict_cases_cover_what_they_claim():
    depth, K, T, n_trees, F, n, _ = (set(v) for v in zip(*C.PREDICT_CASES))
    assert depth == {1, 3, 6} and K == {1, 3, 5} and {1, 7} <= T and 0 in n_trees and F == {1, 8, 1280} and n == {1, 255, 256, 257, 70001}
    assert any(c[3] not in (0, c[2]) for c in C.PREDICT_CASES) and any(c[6] != 0.0 for c in C.PREDICT_CASES)


@pytest.mark.parametrize("objective,K", C.GRAD_CASES)
def test_gradient_bound_admits_the_fp32_restatement(objective, K):
    """the bound of the GPU gradient test, 0.5 + 2^20 x 4 x E32 quanta around the fp64 value, holds for the restatement's own fp32 evaluation on every case, so
    it can never fail a correct fp32 evaluation; and it stays a few quanta wide while a wrong formula is thousands of quanta away"""
    worst = 0.0
    for label, m, y, keep in C.grad_cases(objective, K):
        g64, h64, e32, bound = C.grad_reference(m, y, objective)
        g, h = R.gradients(m, y, objective)
        for k in range(K):
            gq, hq = R.quantise(g[:, k], h[:, k], keep, 0)
            assert np.abs(gq[keep] - 2.0 ** R.FRAC * g64[keep, k]).max(initial=0.0) <= bound, label
            assert np.abs(hq[keep] - 2.0 ** R.FRAC * h64[keep, k]).max(initial=0.0) <= bound, label
            assert not gq[~keep].any() and not hq[~keep].any()
        worst = max(worst, bound)
        if objective == R.SOFTMAX and m.shape[0] >= 255 and "normal" in label:
            assert np.abs(2.0 ** R.FRAC * h64 / 2.0).max() > 1000 * bound                     # what a missing factor 2 in h would be off by
            assert {0, K - 1} <= set(y.tolist())
    print(f"{objective} K {K}: widest bound {worst:.3f} quanta")
    assert worst < 4.0
