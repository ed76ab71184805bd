#!/usr/bin/env python
"""Writes tests/golden/downstream_metrics.json: what the reference's count_f1_max, sklearn and scipy return on drawn inputs, with the inputs.

TEST INFRASTRUCTURE, like make_msa_select_golden.py: it runs only where the reference checkout is mounted read-only at /root/reference, loads the reference's
src/utils/downstream.py by file (a stub module stands in for `omegaconf`, which count_f1_max never touches) and records
  - count_f1_max (ref downstream.py:12-59) on TIE-FREE cases, called as the reference's scripts call it (fp32 pred, integer target) AND with float64 tensors,
    and the largest gap between the two (`f1_max_fp32_gap`);
  - sklearn's roc_auc_score and scipy's spearmanr on inputs WITH ties (2 to 1,000 score levels, n from 2 to 4,100), sklearn's accuracy_score,
    f1_score(average="micro"), mean_squared_error and r2_score;
  - the parameter names of count_f1_max.
No reference source is copied.  Scores are stored compactly: an F1 case keeps the RANK of every score (pred = (rank + 0.5) / (B N), distinct in fp32, drawn so
that the ranking is informative about the target); tied scores are small integers times a power of two.  tests/downstream_ref.py decodes both."""
import contextlib
import importlib.util
import inspect
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
F1_SHAPES = [(1, 1), (1, 5), (3, 1), (7, 37), (64, 65), (33, 257)]


def _import_reference():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not present; goldens are generated in the build container only")
    if "omegaconf" not in sys.modules:
        try:
            import omegaconf  # noqa: F401
        except Exception:
            oc = types.ModuleType("omegaconf")
            oc.DictConfig = dict
            sys.modules["omegaconf"] = oc
    spec = importlib.util.spec_from_file_location("_ref_downstream", os.path.join(REF, "src/utils/downstream.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _f1_case(ref, name, B, N, target, rng):
    import torch
    sys.path.insert(0, ROOT)
    from tests import downstream_ref as R
    noisy = rng.standard_normal((B, N)) + 2.0 * target
    rank = np.empty(B * N, np.int64)
    rank[np.argsort(noisy.reshape(-1), kind="stable")] = np.arange(B * N)
    case = dict(name=name, shape=[B, N], rank=rank.tolist(), target=["".join(str(int(v)) for v in row) for row in target])
    pred, tgt = R.f1_inputs(case)
    assert R.tie_free(pred)
    with contextlib.redirect_stdout(io.StringIO()):
        case["ref_fp32"] = float(ref.count_f1_max(torch.from_numpy(pred), torch.from_numpy(tgt.astype(np.int64))))
        case["ref_fp64"] = float(ref.count_f1_max(torch.from_numpy(pred.astype(np.float64)), torch.from_numpy(tgt.astype(np.float64))))
    return case


def main():
    from scipy.stats import spearmanr
    from sklearn.metrics import accuracy_score, f1_score, mean_squared_error, r2_score, roc_auc_score
    ref = _import_reference()
    rng = np.random.default_rng(20261020)
    f1 = []
    for B, N in F1_SHAPES:
        target = (rng.random((B, N)) < 0.3).astype(np.int64)
        if B * N == 1:
            target[:] = 1
        f1.append(_f1_case(ref, f"{B}x{N}", B, N, target, rng))
    target = (rng.random((4, 6)) < 0.5).astype(np.int64)
    target[1, :] = 0
    target[2, :] = 1
    f1.append(_f1_case(ref, "4x6 with a row without positives and an all-positive row", 4, 6, target, rng))
    f1.append(_f1_case(ref, "5x9 all-zero target", 5, 9, np.zeros((5, 9), np.int64), rng))
    gap = max(abs(c["ref_fp32"] - c["ref_fp64"]) for c in f1)

    ranked = []
    for n, lv in [(2, 2), (3, 2), (17, 3), (255, 2), (257, 16), (1000, 1000), (2049, 50), (4100, 1000), (4097, 7)]:
        y = (rng.random(n) < 0.4).astype(np.int64)
        y[0], y[1] = 0, 1
        a = rng.integers(0, lv, n)
        a = np.minimum(lv - 1, a + (y * rng.integers(0, max(1, lv // 3) + 1, n)))      # informative, still lv levels
        b = rng.integers(0, lv, n)
        b = np.where(rng.random(n) < 0.5, a, b)
        if n == 17:
            a[5] = -a[5]                                                              # a -0.0 among the zeros, a negative among the rest
        scale = 0.125
        fa, fb = (a * scale).astype(np.float32), (b * scale).astype(np.float32)
        ranked.append(dict(n=n, levels=lv, scale=scale, y_true="".join(map(str, y.tolist())), a=a.tolist(), b=b.tolist(),
                           auc=float(roc_auc_score(y, fa.astype(np.float64))), spearman=float(spearmanr(fa.astype(np.float64), fb.astype(np.float64))[0])))
    const = spearmanr(np.ones(5), np.arange(5.0))[0]
    assert np.isnan(const)

    labels = []
    for n, k in [(1, 2), (7, 2), (300, 10), (4100, 826)]:
        yt = rng.integers(0, k, n)
        yp = np.where(rng.random(n) < 0.7, yt, rng.integers(0, k, n))
        labels.append(dict(n=n, classes=k, y_true=yt.tolist(), y_pred=yp.tolist(), accuracy=float(accuracy_score(yt, yp)),
                           f1_micro=float(f1_score(yt, yp, average="micro"))))

    regression = []
    for n in [2, 9, 257, 4100]:
        yt = np.round((50 + 10 * rng.standard_normal(n)) * 64)
        yp = np.round(yt + 5 * 64 * rng.standard_normal(n))
        scale = 1.0 / 64
        ft, fp = (yt * scale).astype(np.float32).astype(np.float64), (yp * scale).astype(np.float32).astype(np.float64)
        regression.append(dict(n=n, scale=scale, y_true=yt.astype(np.int64).tolist(), y_pred=yp.astype(np.int64).tolist(), mse=float(mean_squared_error(ft, fp)),
                               r2=float(r2_score(ft, fp)), spearman=float(spearmanr(ft, fp)[0])))

    import scipy
    import sklearn
    out = dict(source="ref src/utils/downstream.py:12-59 count_f1_max; sklearn %s, scipy %s, numpy %s" % (sklearn.__version__, scipy.__version__, np.__version__),
               f1_max=f1, f1_max_fp32_gap=gap, ranked=ranked, labels=labels, regression=regression,
               signatures=dict(count_f1_max=list(inspect.signature(ref.count_f1_max).parameters)))
    path = os.path.join(HERE, "downstream_metrics.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(f1)} F1 cases (fp32 - fp64 gap {gap:.2e}), {len(ranked)} ranked, {len(labels)} label, {len(regression)} regression cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
