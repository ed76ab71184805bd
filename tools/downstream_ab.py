#!/usr/bin/env python
"""F1-max and the stable sort, device against torch against host: writes profiles/downstream_metrics.json.

F1-max at [rows, labels] = 3,000 x 585 / 1,943 / 320: the label counts are EC / GO-BP / GO-CC of ref src/saprot_fit_mlp.py:137-144; the ROW count is a
STAND-IN (the benchmark splits are not in the tree).  Scores are informative and tie-free: sigmoid(randn + 3 target) replaced by its rank, (rank + 0.5) / (B N).
Three paths alternate in one process, median of --reps windows, every timed window closed by a device synchronise; a window of a device path is --inner
calls back to back (one call is a millisecond: too short a window to time alone) and the figure is the window over --inner:
  device   oneprot_amd.downstream.count_f1_max on device tensors (csrc/metrics.hip; includes its one readback)
  torch    the same rule written with torch ops on the same GPU in fp64 (torch.sort(stable=True), cumsum), one readback
  host     the fp64 numpy restatement (tests/downstream_ref.py f1_max_vectorised) on the host's CPU
Sort alone: oneprot_sort_f32 against torch.sort (default and stable=True) at n = 2^20 and 2^23, argsort only.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oneprot_amd import downstream as D  # noqa: E402
from oneprot_amd import hip  # noqa: E402
from tests import downstream_ref as R  # noqa: E402

LABELS = {"EC": 585, "GO-BP": 1943, "GO-CC": 320}


def draw(seed, B, N):
    rng = np.random.default_rng(seed)
    target = (rng.random((B, N)) < 0.03).astype(np.int32)
    score = 1.0 / (1.0 + np.exp(-(rng.standard_normal((B, N)) + 3.0 * target)))
    rank = np.empty(B * N, np.int64)
    rank[np.argsort(score.reshape(-1), kind="stable")] = np.arange(B * N)
    return ((rank + 0.5) / (B * N)).astype(np.float32).reshape(B, N), target


def torch_rule(pred, target):
    """descending score, ascending flat index, F after every element -- torch ops on the device, fp64"""
    B, N = pred.shape
    order = torch.sort(pred.reshape(-1), descending=True, stable=True).indices
    by_row = torch.sort(torch.div(order, N, rounding_mode="floor"), stable=True).indices
    tp = target.reshape(-1)[order[by_row]].reshape(B, N).double().cumsum(1)
    prec = tp / torch.arange(1, N + 1, device=pred.device, dtype=torch.float64)
    rec = tp / (tp[:, -1:] + 1e-10)
    zero = torch.zeros(B, 1, device=pred.device, dtype=torch.float64)
    start = torch.zeros(B, N, device=pred.device, dtype=torch.float64)
    start[:, 0] = 1
    inc = torch.empty(3, B * N, device=pred.device, dtype=torch.float64)
    inc[0, by_row] = torch.diff(prec, dim=1, prepend=zero).reshape(-1)
    inc[1, by_row] = torch.diff(rec, dim=1, prepend=zero).reshape(-1)
    inc[2, by_row] = start.reshape(-1)
    run = inc.cumsum(1)
    P, Rc = run[0] / run[2], run[1] / B
    return float((2 * P * Rc / (P + Rc + 1e-10)).max())


def timed(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, out


def stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), reps=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window of a device path")
    ap.add_argument("--host-reps", type=int, default=3, help="the host restatement takes seconds per call: fewer repeats of it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "downstream_metrics.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("downstream_ab.py measures the device path: no GPU, no number")
    out = dict(device=torch.cuda.get_device_name(0), rows=a.rows, rows_are="a stand-in: the benchmark splits are not in the tree",
               inner=a.inner, host_threads=torch.get_num_threads(), sort_tile=hip.SORT_TILE, f1_max={}, sort={})
    for task, N in LABELS.items():
        pred, target = draw(N, a.rows, N)
        p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
        paths = dict(device=lambda: D.count_f1_max(p, t), torch=lambda: torch_rule(p, t), host=lambda: R.f1_max_vectorised(pred, target)[0])
        ms, val = {k: [] for k in paths}, {}
        for k in ("device", "torch"):
            paths[k]()                                              # code objects, allocator
        for rep in range(a.reps):
            for k, fn in paths.items():
                if k == "host" and rep >= a.host_reps:
                    continue
                dt, val[k] = timed(fn, 1 if k == "host" else a.inner)
                ms[k].append(dt)
        rec = dict(labels=N, elements=a.rows * N, **{k: stats(v) for k, v in ms.items()}, values=val,
                   device_minus_host=val["device"] - val["host"], torch_minus_host=val["torch"] - val["host"])
        rec["torch_over_device"] = rec["torch"]["median_ms"] / rec["device"]["median_ms"]
        rec["host_over_device"] = rec["host"]["median_ms"] / rec["device"]["median_ms"]
        out["f1_max"][task] = rec
        print(f"{task} {a.rows} x {N}: device {rec['device']['median_ms']:.2f} ms, torch {rec['torch']['median_ms']:.2f} ms, host {rec['host']['median_ms']:.0f} ms; "
              f"device - host {rec['device_minus_host']:.2e}", flush=True)
    for lg in (20, 23):
        n = 1 << lg
        x = torch.randn(n, device="cuda", generator=torch.Generator("cuda").manual_seed(lg))
        paths = dict(device=lambda: hip.sort_f32(x)[0], torch=lambda: torch.sort(x).indices, torch_stable=lambda: torch.sort(x, stable=True).indices)
        ms = {k: [] for k in paths}
        for fn in paths.values():
            fn()
        for rep in range(a.reps):
            for k, fn in paths.items():
                dt, res = timed(fn, a.inner)
                ms[k].append(dt)
        same = bool(torch.equal(hip.sort_f32(x)[0].long(), torch.sort(x, stable=True).indices))
        rec = dict(n=n, **{k: stats(v) for k, v in ms.items()}, equals_torch_stable_sort=same)
        rec["device_over_torch"] = rec["device"]["median_ms"] / rec["torch"]["median_ms"]
        rec["device_mkeys_per_s"] = n / rec["device"]["median_ms"] / 1e3
        out["sort"][f"2^{lg}"] = rec
        print(f"sort n 2^{lg}: device {rec['device']['median_ms']:.3f} ms, torch.sort {rec['torch']['median_ms']:.3f} ms, stable {rec['torch_stable']['median_ms']:.3f} ms, "
              f"equal {same}", flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["device"]["median_ms"], v["torch"]["median_ms"], v["host"]["median_ms"]) for k, v in out["f1_max"].items()}))


if __name__ == "__main__":
    main()
