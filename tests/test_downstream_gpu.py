"""Downstream metrics on the GPU (csrc/metrics.hip through oneprot_amd.hip and oneprot_amd.downstream): the stable sorts against numpy's stable argsort at
every edge size, midranks / scans / moments against numpy fp64, F1-max against the fp64 restatement of the rule (tests/downstream_ref.py) on every fixture
case, on one larger case and on tied scores, the sklearn / scipy numbers of the fixture, evaluate_predictions' keys, and bit-identical repeats."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import downstream_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from oneprot_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def D(hip):
    from oneprot_amd import downstream
    return downstream


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "downstream_metrics.json")) as f:
        return json.load(f)


def reached_at(pred, target, score, want):
    """the reported threshold is a score of the input at which the rule's F1 is the maximum (to the tolerance: two k may reach it within rounding)"""
    f, scores = R.f1_curve(pred, target)
    hit = np.nonzero(scores == np.float32(score))[0]
    return hit.size > 0 and np.abs(f[hit] - want).min() <= 1e-9


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def edge_sizes(tile):
    return [1, 2, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 5]


def keys_of(kind, n, rng):
    if kind == "random":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 1.5, np.float32)
    if kind == "two values":
        return rng.choice(np.array([-2.0, 3.0], np.float32), n)
    if kind == "sorted":
        return np.sort(rng.standard_normal(n).astype(np.float32))
    if kind == "reverse":
        return np.sort(rng.standard_normal(n).astype(np.float32))[::-1].copy()
    if kind == "negatives":
        return -np.abs(rng.standard_normal(n).astype(np.float32)) * np.float32(1e3)
    if kind == "denormals":
        return (rng.integers(-50, 50, n) * np.float32(1e-45) * rng.integers(1, 1000, n)).astype(np.float32)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), n)
    if kind == "inf":
        return rng.choice(np.array([np.inf, -np.inf, 0.0, 3.0e38, -3.0e38, 1.0], np.float32), n)
    raise KeyError(kind)


KINDS = ["random", "equal", "two values", "sorted", "reverse", "negatives", "denormals", "zeros", "inf"]


def want_order(x, descending):
    k = x.astype(np.float64) + 0.0
    return np.argsort(-k if descending else k, kind="stable")


# ---- sorts
@pytest.mark.parametrize("kind", KINDS)
def test_sort_f32_equals_numpy_stable_argsort(hip, kind):
    rng = np.random.default_rng(KINDS.index(kind))
    for n in edge_sizes(hip.SORT_TILE):
        x = keys_of(kind, n, rng)
        for descending in (False, True):
            perm, keys = hip.sort_f32(dev(x), descending=descending, want_keys=True)
            want = want_order(x, descending)
            assert np.array_equal(perm.cpu().numpy(), want), (kind, n, descending)
            assert np.array_equal(keys.cpu().numpy() + np.float32(0), x[want] + np.float32(0)), (kind, n, descending)


def test_sort_f32_many_tiles_and_repeat(hip):
    """more than 256 tiles: the [256, tiles] table's scan has a second level; two runs give the same permutation"""
    n = 300 * hip.SORT_TILE + 7
    rng = np.random.default_rng(11)
    x = (rng.integers(0, 5000, n) * 0.25 - 300).astype(np.float32)               # heavy ties across tiles
    xd = dev(x)
    for descending in (False, True):
        perm, _ = hip.sort_f32(xd, descending=descending)
        again, _ = hip.sort_f32(xd, descending=descending)
        assert np.array_equal(perm.cpu().numpy(), want_order(x, descending))
        assert torch.equal(perm, again)


@pytest.mark.parametrize("key_bits", [1, 8, 9, 16])
def test_sort_i32_equals_numpy_stable_argsort(hip, key_bits):
    rng = np.random.default_rng(key_bits)
    for n in edge_sizes(hip.SORT_TILE) + [20 * hip.SORT_TILE + 3]:
        keys = rng.integers(0, 1 << key_bits, n).astype(np.int32)
        if n > 2:
            keys[-1] = (1 << key_bits) - 1
        order = np.argsort(keys, kind="stable")
        kout, vout = hip.sort_i32(dev(keys), key_bits)                             # values NULL: 0 .. n-1
        assert np.array_equal(vout.cpu().numpy(), order), (key_bits, n)
        assert np.array_equal(kout.cpu().numpy(), keys[order]), (key_bits, n)
        vals = rng.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)
        kout, vout = hip.sort_i32(dev(keys), key_bits, values=dev(vals), want_keys=False)
        assert kout is None and np.array_equal(vout.cpu().numpy(), vals[order]), (key_bits, n)


# ---- midranks
def test_midranks_equal_the_restatement(hip, D):
    rng = np.random.default_rng(5)
    for n in edge_sizes(hip.SORT_TILE) + [40 * hip.SORT_TILE + 1]:
        for lv in (1, 2, 7, 10 ** 9):
            x = rng.integers(0, lv, n).astype(np.float32) - np.float32(lv // 2)
            if n > 3:
                x[1], x[3] = np.float32(-0.0), np.float32(0.0)
            rank2 = hip.midranks_f32(dev(x)).cpu().numpy()
            want = R.midranks(x)
            assert np.array_equal(rank2, np.round(2 * want).astype(np.int64)), (n, lv)
    assert np.array_equal(D.midranks([3.0, 1.0, 3.0, 2.0]).cpu().numpy(), np.array([3.5, 1.0, 3.5, 2.0]))


# ---- scans and moments
def test_scans_against_numpy(hip):
    rng = np.random.default_rng(6)
    T = hip.SCAN_TILE
    sizes = edge_sizes(T) + [T * T + T + 3]                                        # the last needs both levels of partial sums
    for n in sizes:
        xi = rng.integers(-3, 4, n).astype(np.int32)
        assert np.array_equal(hip.inclusive_scan(dev(xi)).cpu().numpy(), np.cumsum(xi, dtype=np.int64).astype(np.int32)), n
        xf = rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 3)
        got = hip.inclusive_scan(dev(xf)).cpu().numpy()
        assert np.max(np.abs(got - np.cumsum(xf))) <= n * 2.0 ** -52 * np.abs(xf).sum(), n
        again = hip.inclusive_scan(dev(xf)).cpu().numpy()
        assert np.array_equal(got, again), n
    for n, seg in [(1, 1), (257, 1), (5 * 37, 37), (3 * T, T), (4 * (T + 1), T + 1), (7 * T + 5, 3), (2 * (T * 3 + 11), T * 3 + 11), (300 * 1943, 1943)]:
        xi = rng.integers(0, 2, n).astype(np.int32)
        xf = rng.standard_normal(n)
        pad = (-n) % seg
        wi = np.cumsum(np.pad(xi, (0, pad)).reshape(-1, seg), axis=1).reshape(-1)[:n]
        wf = np.cumsum(np.pad(xf, (0, pad)).reshape(-1, seg), axis=1).reshape(-1)[:n]
        assert np.array_equal(hip.inclusive_scan(dev(xi), seg_len=seg).cpu().numpy(), wi), (n, seg)
        gf = hip.inclusive_scan(dev(xf), seg_len=seg).cpu().numpy()
        assert np.max(np.abs(gf - wf)) <= seg * 2.0 ** -52 * np.abs(xf).sum(), (n, seg)


def test_moments_against_numpy(hip):
    rng = np.random.default_rng(7)
    for n in edge_sizes(hip.SCAN_TILE) + [8191, 8192, 8193, 5 * 8192 + 1, 300 * 8192 + 17]:
        a, b = rng.integers(-40, 40, n).astype(np.int32), rng.integers(-40, 40, n).astype(np.int32)
        for sa, sb in ((0.0, 0.0), (3.0, -7.0)):
            x, y = a.astype(np.int64) - int(sa), b.astype(np.int64) - int(sb)
            want = [n, x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum(), ((x - y) ** 2).sum(), (a == b).sum()]
            got = hip.moments(dev(a), dev(b), shift_a=sa, shift_b=sb).cpu().numpy()
            assert np.array_equal(got, np.array(want, np.float64)), (n, sa)       # integers below 2^53: every tree gives the exact sum
        fa, fb = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        fb[::3] = fa[::3]
        x, y = fa.astype(np.float64) - 0.5, fb.astype(np.float64)
        terms = [np.ones(n), x, y, x * x, y * y, x * y, (x - y) ** 2, (fa == fb).astype(np.float64)]
        got = hip.moments(dev(fa), dev(fb), shift_a=0.5).cpu().numpy()
        for g, t in zip(got, terms):
            assert abs(g - math.fsum(t)) <= n * 2.0 ** -52 * np.abs(t).sum(), n
        assert np.array_equal(got, hip.moments(dev(fa), dev(fb), shift_a=0.5).cpu().numpy())


# ---- F1-max
def test_f1_max_on_every_fixture_case(D, golden):
    for c in golden["f1_max"]:
        pred, target = R.f1_inputs(c)
        want, at = R.f1_max_walk(pred, target)
        for tgt in (target, target.astype(np.float32), dev(target), target.astype(np.int64)):
            got, score = D.f1_max_and_threshold(pred, tgt)
            print(c["name"], got, got - want, got - c["ref_fp64"])
            assert abs(got - want) <= 1e-9 and abs(got - c["ref_fp64"]) <= 1e-9, c["name"]
            assert reached_at(pred, target, score, want), c["name"]
        assert D.count_f1_max(torch.from_numpy(pred), torch.from_numpy(target)) == got


@pytest.fixture(scope="module")
def larger_case():
    rng = np.random.default_rng(8)
    B, N = 257, 1943
    target = (rng.random((B, N)) < 0.05).astype(np.int32)
    target[3] = 0
    noisy = rng.standard_normal((B, N)) + 3.0 * target
    rank = np.empty(B * N, np.int64)
    rank[np.argsort(noisy.reshape(-1), kind="stable")] = np.arange(B * N)
    pred = ((rank + 0.5) / (B * N)).astype(np.float32).reshape(B, N)
    assert R.tie_free(pred)
    return pred, target, R.f1_max_vectorised(pred, target)


def test_f1_max_larger_case_and_repeat(hip, D, larger_case):
    pred, target, (want, at) = larger_case
    p, t = dev(pred), dev(target)
    first = hip.f1max(p, t)
    second = hip.f1max(p, t)
    got, score = first.cpu().tolist()
    print("257 x 1943", got, got - want)
    assert abs(got - want) <= 1e-9 and reached_at(pred, target, score, want)
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))         # bit-identical
    assert D.count_f1_max(p, t) == got


def test_f1_max_with_ties_follows_the_documented_rule(D):
    rng = np.random.default_rng(9)
    for B, N, lv in [(5, 40, 7), (3, 300, 2), (64, 65, 50), (2, 2049, 1)]:
        target = (rng.random((B, N)) < 0.3).astype(np.int32)
        pred = (rng.integers(0, lv, (B, N)) + 2 * target).astype(np.float32) * np.float32(0.125) - np.float32(0.25)
        want, at = R.f1_max_walk(pred, target)
        got, score = D.f1_max_and_threshold(pred, target)
        print((B, N, lv), got, got - want)
        assert abs(got - want) <= 1e-9 and reached_at(pred, target, score, want), (B, N, lv)


# ---- the sklearn / scipy numbers
def test_rank_metrics_equal_the_fixture(D, golden):
    for c in golden["ranked"]:
        a, b = R.levels(c["a"], c["scale"]), R.levels(c["b"], c["scale"])
        y = np.array([int(ch) for ch in c["y_true"]])
        assert abs(D.binary_auc(y, a) - c["auc"]) <= 1e-10, c["n"]
        assert abs(D.binary_auc(dev(y), dev(a)) - c["auc"]) <= 1e-10, c["n"]
        rho = D.spearman_rho(a, b)
        assert (math.isnan(rho) and math.isnan(c["spearman"])) or abs(rho - c["spearman"]) <= 1e-10, c["n"]
        assert D.spearman_rho(dev(a), dev(b)) == rho or math.isnan(rho)
    assert math.isnan(D.spearman_rho(np.ones(5), np.arange(5.0)))
    with pytest.raises(ValueError, match="Only one class"):
        D.binary_auc(dev(np.ones(4, np.int64)), dev(np.arange(4, dtype=np.float32)))


def test_label_and_regression_metrics_equal_the_fixture(D, golden):
    for c in golden["labels"]:
        assert abs(D.accuracy(c["y_true"], c["y_pred"]) - c["accuracy"]) <= 1e-10
        assert abs(D.accuracy(dev(np.array(c["y_true"])), dev(np.array(c["y_pred"]))) - c["f1_micro"]) <= 1e-10
    for c in golden["regression"]:
        yt, yp = R.levels(c["y_true"], c["scale"]), R.levels(c["y_pred"], c["scale"])
        mse, r2 = D.regression_scores(yt, yp)
        assert abs(mse - c["mse"]) <= 1e-10 * max(1.0, abs(c["mse"])) and abs(r2 - c["r2"]) <= 1e-10, c["n"]
        assert abs(D.spearman_rho(yt, yp) - c["spearman"]) <= 1e-10, c["n"]
    assert D.regression_scores([2.0, 2.0, 2.0], [2.0, 2.0, 2.0]) == (0.0, 1.0) and D.regression_scores([2.0, 2.0], [1.0, 3.0]) == (1.0, 0.0)


def test_evaluate_predictions_keys_per_task_group(D, golden):
    c = golden["ranked"][4]
    y, score = np.array([int(ch) for ch in c["y_true"]]), R.levels(c["a"], c["scale"])
    for task in D.BINARY_TASKS:
        out = D.evaluate_predictions(task, score.reshape(-1, 1), y, "valid")
        assert list(out) == ["valid_accuracy", "valid_f1_micro", "valid_auc"]
        assert abs(out["valid_auc"] - c["auc"]) <= 1e-10 and out["valid_accuracy"] == R.accuracy(y, score > 0.5) == out["valid_f1_micro"]
    f = golden["f1_max"][3]
    pred, target = R.f1_inputs(f)
    for task in D.MULTILABEL_TASKS:
        out = D.evaluate_predictions(task, torch.from_numpy(pred), torch.from_numpy(target), "test")
        assert list(out) == ["test_f1_max"] and abs(out["test_f1_max"] - f["ref_fp64"]) <= 1e-9
    r = golden["regression"][2]
    out = D.evaluate_predictions("ThermoStability", R.levels(r["y_pred"], r["scale"]), R.levels(r["y_true"], r["scale"]), "test")
    assert list(out) == ["test_mse", "test_r2", "test_spearman_rho"]
    assert abs(out["test_mse"] - r["mse"]) <= 1e-10 * r["mse"] and abs(out["test_r2"] - r["r2"]) <= 1e-10 and abs(out["test_spearman_rho"] - r["spearman"]) <= 1e-10
    lab = golden["labels"][2]
    for task in D.MULTICLASS_TASKS:
        out = D.evaluate_predictions(task, np.array(lab["y_pred"]), np.array(lab["y_true"]), "valid")
        assert list(out) == ["valid_accuracy", "valid_f1_micro"] and abs(out["valid_accuracy"] - lab["accuracy"]) <= 1e-10
    with pytest.raises(ValueError, match="unknown task"):
        D.evaluate_predictions("Nope", pred, target, "test")
