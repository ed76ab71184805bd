#!/usr/bin/env python3
"""Time per round and per fit of the gradient-boosted tree probe (oneprot_amd/gbt.py, csrc/gbt.hip) at the downstream benchmark's shapes, beside sklearn's
HistGradientBoostingClassifier on this box's CPUs at matched depth, rounds and learning rate, alternating in one process.

sklearn's estimator is ANOTHER ALGORITHM and a loose yardstick: other binning (255 quantile bins of its own), other regularisation (no min_child_weight, its
own l2), float histograms, one label at a time.  xgboost, the reference's tool, is not installed; the parent commit has no such path to compare with.  Both
sides' held-out accuracy on the synthetic task is reported so that "faster" is not read off a model that learned nothing.

Workloads (synthetic Gaussian embeddings, a noisy linear label):
  binary   15,000 x 1,280, depth 5, 250 rounds (the sweep's setting), learning rate 0.1, reg_lambda 10
  ec       15,000 x 1,280 with 585 labels, 5 rounds; the 250-round figure is an EXTRAPOLATION (setup + 250 x the per-round time); sklearn fits `--ec-labels`
           labels one after the other for 5 rounds and is scaled to 585 labels, which is an extrapolation too
Timing: a host clock around a fit that ends in a device synchronise; the per-round time is (fit - setup) / rounds with the setup (cuts and bins) timed on
its own.  `--profile-round` runs only a short HIP fit, for a kernel trace taken in a run of its own.

    python tools/gbt_ab.py [--reps 2] [--out profiles/gbt_fit.json]"""
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

from oneprot_amd import gbt, hip                                                 # noqa: E402

DEV = "cuda:0"
N_TRAIN, N_TEST, WIDTH, LABELS, DEPTH, LR, LAMBDA = 15000, 3000, 1280, 585, 5, 0.1, 10.0


def synthetic(labels, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N_TRAIN + N_TEST, WIDTH, generator=g)
    W = torch.randn(WIDTH, labels, generator=g) / WIDTH ** 0.5
    Y = ((X @ W + 0.3 * torch.randn(N_TRAIN + N_TEST, labels, generator=g)) > (0.0 if labels == 1 else 1.5)).float()
    return X[:N_TRAIN], Y[:N_TRAIN], X[N_TRAIN:], Y[N_TRAIN:]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts), runs=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=250)
    ap.add_argument("--ec-labels", type=int, default=4, help="labels sklearn fits at the EC shape (scaled to 585)")
    ap.add_argument("--profile-round", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbt_fit.json"))
    args = ap.parse_args()
    hip.lib()
    xt, yt, xs, ys = synthetic(1)
    xt_d, xs_d = xt.to(DEV), xs.to(DEV)
    if args.profile_round:                                                        # three rounds under the tracer; the first also carries the cuts and bins
        gbt.XGBClassifier(n_estimators=3, max_depth=DEPTH, learning_rate=LR, reg_lambda=LAMBDA).fit(xt_d, yt[:, 0])
        torch.cuda.synchronize()
        return
    from sklearn.ensemble import HistGradientBoostingClassifier
    cpus = len(os.sched_getaffinity(0))
    threads = int(os.environ.get("OMP_NUM_THREADS", "16"))
    out = {"device": torch.cuda.get_device_name(0), "cpu_threads_sklearn": threads, "cpus_visible": cpus,
           "note": "sklearn.ensemble.HistGradientBoostingClassifier is another algorithm and a loose yardstick (module docstring)", "workloads": {}}

    # ---- setup alone: cuts and bins
    gbt.build_cuts(xt_d, 256)
    t_setup = [wall(lambda: gbt.build_cuts(xt_d, 256))[0] for _ in range(3)]

    # ---- binary, 250 rounds
    def fit_hip(rounds, y):
        return gbt.XGBClassifier(n_estimators=rounds, max_depth=DEPTH, learning_rate=LR, reg_lambda=LAMBDA).fit(xt_d, y)

    def fit_sk(rounds, y):
        return HistGradientBoostingClassifier(max_iter=rounds, max_depth=DEPTH, learning_rate=LR, max_leaf_nodes=None, l2_regularization=LAMBDA, early_stopping=False,
                                              max_bins=255).fit(xt.numpy(), y.numpy())

    fit_hip(3, yt[:, 0])                                                          # warm-up of every kernel and of the allocator
    t_hip, t_sk = [], []
    for _ in range(args.reps):
        dt, model = wall(lambda: fit_hip(args.rounds, yt[:, 0]))
        t_hip.append(dt)
        dt, sk = wall(lambda: fit_sk(args.rounds, yt[:, 0]))
        t_sk.append(dt)
    acc_hip = float((model.predict(xs_d).cpu() == ys[:, 0].long()).float().mean())
    acc_sk = float((torch.from_numpy(sk.predict(xs.numpy())).long() == ys[:, 0].long()).float().mean())
    mh, ms, su = statistics.median(t_hip), statistics.median(t_sk), statistics.median(t_setup)
    out["workloads"]["binary"] = dict(rows=N_TRAIN, features=WIDTH, depth=DEPTH, rounds=args.rounds, learning_rate=LR, hip_fit_s=summary(t_hip), hip_setup_s=summary(t_setup),
                                      hip_ms_per_round=(mh - su) * 1e3 / args.rounds, sklearn_fit_s=summary(t_sk), sklearn_ms_per_round=ms * 1e3 / args.rounds,
                                      sklearn_over_hip=ms / mh, heldout_accuracy_hip=acc_hip, heldout_accuracy_sklearn=acc_sk)
    print(json.dumps(out["workloads"]["binary"]))

    # ---- the EC shape, 5 rounds
    xt2, yt2, xs2, ys2 = synthetic(LABELS, seed=1)
    xt_d, xs_d = xt2.to(DEV), xs2.to(DEV)
    xt = xt2
    yt2_d = yt2.to(DEV)
    fit_hip(1, yt2_d)
    t_hip, t_sk = [], []
    for _ in range(args.reps):
        dt, model = wall(lambda: fit_hip(5, yt2_d))
        t_hip.append(dt)
        dt, sks = wall(lambda: [fit_sk(5, yt2[:, l]) for l in range(args.ec_labels)])
        t_sk.append(dt * LABELS / args.ec_labels)
    acc_hip = float((model.predict(xs_d).cpu()[:, :args.ec_labels] == ys2[:, :args.ec_labels].long()).float().mean())
    acc_sk = float(np.mean([(torch.from_numpy(m.predict(xs2.numpy())).long() == ys2[:, l].long()).float().mean() for l, m in enumerate(sks)]))
    mh, ms = statistics.median(t_hip), statistics.median(t_sk)
    per_round = (mh - su) / 5
    out["workloads"]["ec"] = dict(rows=N_TRAIN, features=WIDTH, labels=LABELS, depth=DEPTH, rounds=5, learning_rate=LR, chunks=len(gbt.plan_chunks(LABELS, WIDTH, 256, DEPTH)),
                                  hip_fit_s=summary(t_hip), hip_s_per_round=per_round, hip_fit_s_250_rounds_EXTRAPOLATED=su + 250 * per_round,
                                  sklearn_fit_s_585_labels_EXTRAPOLATED_from=args.ec_labels, sklearn_fit_s=summary(t_sk), sklearn_over_hip=ms / mh,
                                  heldout_accuracy_first_labels_hip=acc_hip, heldout_accuracy_first_labels_sklearn=acc_sk,
                                  positive_rate=float(yt2.mean()))
    print(json.dumps(out["workloads"]["ec"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
