"""Downstream metrics without a GPU: the fp64 restatements of the scoring rules (tests/downstream_ref.py) against what the reference's count_f1_max, sklearn
and scipy returned (tests/golden/downstream_metrics.json), the fixture's own health (tie-free F1 cases), the refusals of oneprot_amd.downstream and of the
C entry points, the re-export's signature, and the header / binding of the new entry points."""
import ctypes
import inspect
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import downstream_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("oneprot_sort_workspace", "oneprot_sort_f32", "oneprot_sort_i32", "oneprot_midranks_workspace", "oneprot_midranks_f32", "oneprot_scan_workspace",
                "oneprot_inclusive_scan", "oneprot_moments_workspace", "oneprot_moments", "oneprot_f1max_workspace", "oneprot_f1max")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "downstream_metrics.json")) as f:
        return json.load(f)


# ---- the restatement against the fixture
def test_f1_cases_cover_the_asked_shapes_and_are_tie_free(golden):
    shapes = [tuple(c["shape"]) for c in golden["f1_max"]]
    for want in [(1, 1), (1, 5), (3, 1), (7, 37), (64, 65), (33, 257)]:
        assert want in shapes
    targets = [R.f1_inputs(c)[1] for c in golden["f1_max"]]
    assert any((t.sum(1) == 0).any() and t.sum() > 0 for t in targets)              # a row without positives
    assert any((t.sum(1) == t.shape[1]).any() and t.shape[1] > 1 for t in targets)  # an all-positive row
    assert any(t.sum() == 0 for t in targets)                                       # an all-zero target matrix
    for c in golden["f1_max"]:
        pred, _ = R.f1_inputs(c)
        assert R.tie_free(pred), c["name"]                                          # a fixture with ties would pin nothing: the reference is undefined there
        assert sorted(c["rank"]) == list(range(pred.size)), c["name"]


def test_f1_restatement_equals_the_reference(golden):
    gap = golden["f1_max_fp32_gap"]
    assert 0 < gap < 1e-6
    assert gap == max(abs(c["ref_fp32"] - c["ref_fp64"]) for c in golden["f1_max"])
    for c in golden["f1_max"]:
        pred, target = R.f1_inputs(c)
        walk, at = R.f1_max_walk(pred, target)
        twin, at2 = R.f1_max_vectorised(pred, target)
        assert abs(walk - c["ref_fp64"]) <= 1e-12, c["name"]
        assert abs(twin - c["ref_fp64"]) <= 1e-12, c["name"]
        assert abs(walk - c["ref_fp32"]) <= gap + 1e-12, c["name"]                   # the reference as its scripts call it: inside its own fp32 noise
        assert at == at2 and (walk == 0 or at in pred), c["name"]


def test_rank_metrics_equal_sklearn_and_scipy(golden):
    assert any(c["levels"] == 2 for c in golden["ranked"]) and any(c["levels"] == 1000 for c in golden["ranked"])
    assert min(c["n"] for c in golden["ranked"]) == 2 and max(c["n"] for c in golden["ranked"]) >= 4097
    for c in golden["ranked"]:
        a, b = R.levels(c["a"], c["scale"]), R.levels(c["b"], c["scale"])
        y = np.array([int(ch) for ch in c["y_true"]])
        assert c["n"] <= 3 or len(np.unique(a)) < c["n"]                            # ties are what these cases are for
        assert abs(R.binary_auc(y, a) - c["auc"]) <= 1e-12, c["n"]
        rho = R.spearman_rho(a, b)
        assert (math.isnan(rho) and math.isnan(c["spearman"])) or abs(rho - c["spearman"]) <= 1e-12, c["n"]
    assert math.isnan(R.spearman_rho(np.ones(5), np.arange(5.0)))


def test_label_and_regression_metrics_equal_sklearn(golden):
    for c in golden["labels"]:
        assert c["accuracy"] == c["f1_micro"] or abs(c["accuracy"] - c["f1_micro"]) <= 1e-12        # one count serves both
        assert abs(R.accuracy(c["y_true"], c["y_pred"]) - c["accuracy"]) <= 1e-12
    for c in golden["regression"]:
        mse, r2 = R.regression_scores(R.levels(c["y_true"], c["scale"]), R.levels(c["y_pred"], c["scale"]))
        assert abs(mse - c["mse"]) <= 1e-12 * max(1.0, abs(c["mse"])) and abs(r2 - c["r2"]) <= 1e-12, c["n"]
        assert abs(R.spearman_rho(R.levels(c["y_true"], c["scale"]), R.levels(c["y_pred"], c["scale"])) - c["spearman"]) <= 1e-12


# ---- the host module: refusals before the device is touched
@pytest.fixture()
def no_device(monkeypatch):
    from oneprot_amd import downstream as D

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(D, "_device", touched)
    return D


def test_refusals(no_device):
    D = no_device
    p, t = np.linspace(0.1, 0.9, 6, dtype=np.float32).reshape(2, 3), np.array([[0, 1, 0], [1, 0, 0]])
    with pytest.raises(ValueError, match="same shape"):
        D.count_f1_max(p, t[:, :2])
    with pytest.raises(ValueError, match=r"\[B, N\]"):
        D.count_f1_max(p.reshape(-1), t.reshape(-1))
    with pytest.raises(ValueError, match="empty"):
        D.count_f1_max(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    with pytest.raises(ValueError, match="dimensions"):
        D.count_f1_max(p.reshape(1, 2, 3), t.reshape(1, 2, 3))
    with pytest.raises(ValueError, match="outside"):
        D.count_f1_max(p, t * 2)
    with pytest.raises(ValueError, match="outside"):
        D.count_f1_max(torch.from_numpy(p), torch.from_numpy(t).float() * 0.5)
    with pytest.raises(ValueError, match="2\\^31"):
        D.count_f1_max(torch.zeros(1).expand(46341, 46341), torch.zeros(1).expand(46341, 46341))      # 2^31 + 4,281 elements, no memory behind them
    with pytest.raises(ValueError, match="Only one class"):
        D.binary_auc([1, 1, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="outside"):
        D.binary_auc([0, 2, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="labels"):
        D.binary_auc([0, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="vector"):
        D.argsort(p)
    with pytest.raises(ValueError, match="empty"):
        D.midranks([])
    with pytest.raises(ValueError, match="elements"):
        D.spearman_rho([1.0, 2.0], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="predictions"):
        D.accuracy([1, 2], [1])
    with pytest.raises(ValueError, match="predictions"):
        D.regression_scores([1.0, 2.0], [1.0])
    with pytest.raises(ValueError, match="unknown task"):
        D.evaluate_predictions("NoSuchTask", p, t, "test")


def test_task_lists_are_the_references():
    from oneprot_amd import downstream as D
    assert D.BINARY_TASKS == ("MetalIonBinding", "DeepLoc2", "HumanPPI") and D.MULTILABEL_TASKS == ("EC", "GO-BP", "GO-MF", "GO-CC")
    assert D.REGRESSION_TASKS == ("ThermoStability",) and D.MULTICLASS_TASKS == ("DeepLoc10", "TopEnzyme")


def test_missing_library_raises(monkeypatch):
    from oneprot_amd import downstream as D
    from oneprot_amd import hip
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", "/nonexistent/liboneprot_hip.so")
    with pytest.raises(hip.HipLibraryMissing):
        D.count_f1_max(np.array([[0.2, 0.7]], np.float32), np.array([[0, 1]]))


def test_reexport_has_the_references_signature(golden):
    from oneprot_amd import downstream as D
    from src.utils.downstream import count_f1_max
    assert count_f1_max is D.count_f1_max
    assert list(inspect.signature(count_f1_max).parameters) == golden["signatures"]["count_f1_max"] == ["pred", "target"]


# ---- the ABI
def test_header_declares_and_binding_maps_the_entry_points():
    from oneprot_amd import hip
    P, I, L64, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    for name in ENTRY_POINTS:
        assert name in hip._SIGS, name
    assert hip.ABI_VERSION == 7
    assert hip._SIGS["oneprot_sort_workspace"] == (SZ, [L64])
    assert hip._SIGS["oneprot_sort_f32"] == (I, [P, L64, I, P, P, P, SZ, P])
    assert hip._SIGS["oneprot_sort_i32"] == (I, [P, P, L64, I, P, P, P, SZ, P])
    assert hip._SIGS["oneprot_midranks_f32"] == (I, [P, L64, P, P, SZ, P])
    assert hip._SIGS["oneprot_inclusive_scan"] == (I, [P, P, L64, L64, I, P, SZ, P])
    assert hip._SIGS["oneprot_moments"] == (I, [P, P, L64, I, F, F, P, P, SZ, P])
    assert hip._SIGS["oneprot_f1max_workspace"] == (SZ, [I, I])
    assert hip._SIGS["oneprot_f1max"] == (I, [P, P, I, I, I, P, P, SZ, P])
    assert hip._PTR_DTYPES["oneprot_sort_f32"] == "fifb"
    assert hip._PTR_DTYPES["oneprot_sort_i32"] == "iiiib"                           # uint32 keys travel as int*
    assert hip._PTR_DTYPES["oneprot_midranks_f32"] == "fib"
    assert hip._PTR_DTYPES["oneprot_inclusive_scan"] == "**b"                       # int32 or fp64, stated by is_f64
    assert hip._PTR_DTYPES["oneprot_moments"] == "**bb"                             # the 8 doubles travel as bytes
    assert hip._PTR_DTYPES["oneprot_f1max"] == "f*bb"
    assert hip.SORT_TILE >= 256 and hip.SORT_TILE % 256 == 0 and hip.SCAN_TILE % 256 == 0
    with open(hip.HEADER_PATH) as f:
        text = f.read()
    for cite in ("downstream.py:12-59", "roc_auc_score", "spearmanr"):
        assert cite in text


@pytest.fixture(scope="module")
def lib():
    from oneprot_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        subprocess.check_call(["bash", os.path.join(ROOT, "oneprot_amd", "csrc", "build.sh")])
    return h.lib()


def test_entry_points_reject_bad_arguments(lib):
    keep = [ctypes.create_string_buffer(64) for _ in range(6)]
    a, b, c, d, e, f = [ctypes.addressof(x) for x in keep]
    for q in (lib.oneprot_sort_workspace, lib.oneprot_midranks_workspace, lib.oneprot_scan_workspace, lib.oneprot_moments_workspace):
        assert q(0) == 0 and q(-1) == 0 and q(2 ** 31) == 0 and q(1) > 0 and q(2 ** 31 - 1) > 0
    assert lib.oneprot_f1max_workspace(0, 5) == 0 and lib.oneprot_f1max_workspace(5, 0) == 0 and lib.oneprot_f1max_workspace(46341, 46341) == 0
    assert lib.oneprot_f1max_workspace(46340, 46341) > 0 and lib.oneprot_f1max_workspace(1, 1) > 0
    big = 1 << 40                                                                  # a workspace size no query exceeds for n = 8
    assert lib.oneprot_sort_f32(None, 8, 0, b, None, c, big, None) == -1
    assert lib.oneprot_sort_f32(a, 8, 0, None, None, c, big, None) == -1
    assert lib.oneprot_sort_f32(a, 8, 0, b, None, None, big, None) == -1
    assert lib.oneprot_sort_f32(a, 0, 0, b, None, c, big, None) == -1
    assert lib.oneprot_sort_f32(a, 2 ** 31, 0, b, None, c, big, None) == -1
    assert lib.oneprot_sort_f32(a, 8, 2, b, None, c, big, None) == -1
    assert lib.oneprot_sort_f32(a, 8, 0, b, None, c, lib.oneprot_sort_workspace(8) - 1, None) == -1
    for bits in (0, 32, -1):
        assert lib.oneprot_sort_i32(a, None, 8, bits, None, b, c, big, None) == -1
    assert lib.oneprot_sort_i32(a, None, 8, 8, a, b, c, big, None) == -1           # in place
    assert lib.oneprot_sort_i32(a, b, 8, 8, None, b, c, big, None) == -1
    assert lib.oneprot_sort_i32(a, None, 8, 8, None, None, c, big, None) == -1
    assert lib.oneprot_midranks_f32(a, 8, None, c, big, None) == -1
    assert lib.oneprot_midranks_f32(a, 8, b, c, lib.oneprot_midranks_workspace(8) - 1, None) == -1
    assert lib.oneprot_inclusive_scan(a, b, 8, -1, 0, c, big, None) == -1
    assert lib.oneprot_inclusive_scan(a, b, 8, 0, 2, c, big, None) == -1
    assert lib.oneprot_inclusive_scan(a, b, 0, 0, 0, c, big, None) == -1
    assert lib.oneprot_moments(a, None, 8, 0, 0.0, 0.0, d, c, big, None) == -1
    assert lib.oneprot_moments(a, b, 8, 3, 0.0, 0.0, d, c, big, None) == -1
    assert lib.oneprot_moments(a, b, 8, 0, 0.0, 0.0, None, c, big, None) == -1
    assert lib.oneprot_f1max(a, b, 0, 0, 4, d, c, big, None) == -1
    assert lib.oneprot_f1max(a, b, 2, 2, 4, d, c, big, None) == -1
    assert lib.oneprot_f1max(a, b, 0, 46341, 46341, d, c, big, None) == -1
    assert lib.oneprot_f1max(a, None, 0, 2, 4, d, c, big, None) == -1
    assert lib.oneprot_f1max(a, b, 0, 2, 4, d, c, lib.oneprot_f1max_workspace(2, 4) - 1, None) == -1


# ---- the launchers: the positional tuple handed to hip.call (no library launch)
def test_launchers_order_their_arguments_as_the_header_declares(monkeypatch):
    from oneprot_amd import hip
    rec = []
    monkeypatch.setattr(hip, "call", lambda name, *args: rec.append((name,) + args))
    monkeypatch.setattr(hip, "query", lambda name, *args: 4096 + len(args))
    x, k, v = torch.zeros(5), torch.zeros(5, dtype=torch.int32), torch.ones(5, dtype=torch.int32)
    perm, keys = hip.sort_f32(x, descending=True, want_keys=True)
    name, a_keys, n, desc, a_perm, a_sorted, ws, nbytes = rec[-1]
    assert (name, n, desc, nbytes) == ("oneprot_sort_f32", 5, 1, 4097) and a_keys is x and a_perm is perm and a_sorted is keys
    assert perm.dtype == torch.int32 and keys.dtype == torch.float32 and ws.dtype == torch.uint8 and ws.numel() == 4097
    assert hip.sort_f32(x)[1] is None and rec[-1][3] == 0 and rec[-1][5] is None
    kout, vout = hip.sort_i32(k, 9, values=v)
    assert rec[-1][:5] == ("oneprot_sort_i32", k, v, 5, 9) and rec[-1][5] is kout and rec[-1][6] is vout and rec[-1][8] == 4097
    kout, vout = hip.sort_i32(k, 1, want_keys=False)
    assert kout is None and rec[-1][2] is None and rec[-1][5] is None and rec[-1][6] is vout
    r2 = hip.midranks_f32(x)
    assert rec[-1][:3] == ("oneprot_midranks_f32", x, 5) and rec[-1][3] is r2 and r2.dtype == torch.int32
    y = hip.inclusive_scan(k, seg_len=3)
    assert rec[-1][:6] == ("oneprot_inclusive_scan", k, y, 5, 3, 0) and y.dtype == torch.int32
    d = torch.zeros(4, dtype=torch.float64)
    assert hip.inclusive_scan(d).dtype == torch.float64 and rec[-1][4:6] == (0, 1)
    m = hip.moments(k, v, shift_a=2.0)
    assert rec[-1][:7] == ("oneprot_moments", k, v, 5, 1, 2.0, 0.0) and m.dtype == torch.float64 and m.numel() == 8 and rec[-1][7].numel() == 64
    assert hip.moments(x, x).numel() == 8 and rec[-1][4] == 0
    p, t = torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32)
    out = hip.f1max(p, t)
    assert rec[-1][:6] == ("oneprot_f1max", p, t, 0, 2, 3) and out.dtype == torch.float64 and out.numel() == 2 and rec[-1][8] == 4098
    assert hip.f1max(p, t.float()).numel() == 2 and rec[-1][3] == 1
    for bad in (lambda: hip.inclusive_scan(x), lambda: hip.moments(x, k), lambda: hip.moments(x, torch.zeros(4)), lambda: hip.f1max(p, t.long()),
                lambda: hip.f1max(p, t[:1])):
        with pytest.raises(hip.HipKernelError):
            bad()
    monkeypatch.setattr(hip, "query", lambda name, *args: 0)
    with pytest.raises(hip.HipKernelError, match="invalid size"):
        hip.sort_f32(x)
