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
  regression (--deep)  15,000 x 1,280, XGBRegressor at depths 3, 5 and 9 (the regression sweep's grid; depth 9 runs levels 6 .. 8 over the rows in node order),
           beside sklearn's HistGradientBoostingRegressor at depth 9; held-out R2 on 3,000 further rows.  Also: the time of every launch of one depth-9 fit by
           entry point and level (HIP events around the launches), and the node-ordered histogram at every tile shape on that fit's own node layout.  Merged
           into the output file under "regression"; the other workloads' entries stay.
Timing: a host clock around a fit that ends in a device synchronise; the per-round time is (fit - setup) / rounds with the setup (cuts and bins) timed on
its own.  `--profile-round` runs only a short HIP fit, for a kernel trace taken in a run of its own.

    python tools/gbt_ab.py [--reps 2] [--out profiles/gbt_fit.json]
    python tools/gbt_ab.py --deep [--rounds 250]"""
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


def synthetic_regression(seed=2):
    """a target that a deep tree can use: a linear part, two products and a sine of the first columns, noise of a tenth of the signal"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N_TRAIN + N_TEST, WIDTH, generator=g)
    w = torch.randn(WIDTH, generator=g) / WIDTH ** 0.5
    y = X @ w + X[:, 0] * X[:, 1] + torch.sin(2.0 * X[:, 2]) + 0.5 * X[:, 3] * X[:, 4] + 0.15 * torch.randn(N_TRAIN + N_TEST, generator=g)
    return X[:N_TRAIN], y[:N_TRAIN], X[N_TRAIN:], y[N_TRAIN:]


def r2(pred, y):
    pred, y = pred.double().cpu(), y.double().cpu()
    return float(1.0 - ((pred - y) ** 2).sum() / ((y - y.mean()) ** 2).sum())


DEEP_WATCH = ("oneprot_gbt_sample", "oneprot_gbt_grad", "oneprot_gbt_hist", "oneprot_gbt_split", "oneprot_gbt_partition", "oneprot_gbt_update", "oneprot_gbt_node_keys",
              "oneprot_sort_i32", "oneprot_gbt_node_seg", "oneprot_gbt_hist_nodes", "oneprot_gbt_split_nodes")
LEVEL_ARG = {"oneprot_gbt_hist": 3, "oneprot_gbt_split": 3, "oneprot_gbt_partition": 2, "oneprot_gbt_node_keys": 1, "oneprot_gbt_node_seg": 1, "oneprot_gbt_hist_nodes": 3,
             "oneprot_gbt_split_nodes": 3}      # where the level stands among an entry point's scalar arguments


def deep(args):
    from oneprot_amd import gbt_deep
    xt, yt, xs, ys = synthetic_regression()
    xt_d, xs_d, yt_d = xt.to(DEV), xs.to(DEV), yt.to(DEV)
    rounds = args.rounds

    def fit_hip(depth, n):
        return gbt.XGBRegressor(n_estimators=n, max_depth=depth, learning_rate=LR, reg_lambda=LAMBDA).fit(xt_d, yt_d)

    if args.profile_round:                                                        # three depth-9 rounds under the tracer
        fit_hip(9, 3)
        torch.cuda.synchronize()
        return
    out = {"rows": N_TRAIN, "features": WIDTH, "rounds": rounds, "learning_rate": LR, "reg_lambda": LAMBDA, "max_bin": 256, "depths": {}}
    gbt.build_cuts(xt_d, 256)
    su = statistics.median([wall(lambda: gbt.build_cuts(xt_d, 256))[0] for _ in range(3)])
    out["hip_setup_s"] = su
    for depth in (3, 5, 9):
        fit_hip(depth, 3)
    t = {3: [], 5: [], 9: []}
    models = {}
    for _ in range(args.reps):                                                    # the depths alternate
        for depth in (3, 5, 9):
            dt, models[depth] = wall(lambda: fit_hip(depth, rounds))
            t[depth].append(dt)
    for depth in (3, 5, 9):
        m = statistics.median(t[depth])
        out["depths"][str(depth)] = dict(hip_fit_s=summary(t[depth]), hip_ms_per_round=(m - su) * 1e3 / rounds, heldout_r2=r2(models[depth].predict(xs_d), ys),
                                         train_r2=r2(models[depth].predict(xt_d), yt))
        print(json.dumps({depth: out["depths"][str(depth)]}))
    try:
        from sklearn.ensemble import HistGradientBoostingRegressor
        ts = []
        for _ in range(args.reps):
            dt, sk = wall(lambda: HistGradientBoostingRegressor(max_iter=rounds, max_depth=9, learning_rate=LR, max_leaf_nodes=None, l2_regularization=LAMBDA, early_stopping=False,
                                                                 max_bins=255).fit(xt.numpy(), yt.numpy()))
            ts.append(dt)
        out["sklearn_depth_9"] = dict(note="sklearn.ensemble.HistGradientBoostingRegressor: another algorithm and a loose yardstick (module docstring)",
                                      threads=int(os.environ.get("OMP_NUM_THREADS", "16")), fit_s=summary(ts), ms_per_round=statistics.median(ts) * 1e3 / rounds,
                                      heldout_r2=r2(torch.from_numpy(sk.predict(xs.numpy())), ys), over_hip=statistics.median(ts) / statistics.median(t[9]))
        print(json.dumps(out["sklearn_depth_9"]))
    except ImportError as e:
        out["sklearn_depth_9"] = f"not importable: {e}"

    # ---- every launch of a 20-round depth-9 fit, by entry point and level (HIP events around the launches: the host's launch gaps are not in these figures)
    n_prof = 20
    hip.profile_begin({name: None for name in DEEP_WATCH})
    fit_hip(9, n_prof)
    per = hip.profile_end()
    table, total = {}, 0.0
    for name, launches in per.items():
        for ms, sc in launches:
            ints = [a for a in sc[:-1] if isinstance(a, int)]
            key = f"{name} level {ints[LEVEL_ARG[name]]}" if name in LEVEL_ARG else name
            table.setdefault(key, []).append(ms)
            total += ms
    out["launches_depth_9"] = {"rounds": n_prof, "ms_per_round_in_launches": total / n_prof,
                               "us_per_launch_median": {k: statistics.median(v) * 1e3 for k, v in sorted(table.items())},
                               "launches_per_round": {k: len(v) / n_prof for k, v in sorted(table.items())},
                               "share_of_round": {k: sum(v) / total for k, v in sorted(table.items())}}
    print(json.dumps(out["launches_depth_9"]))

    # ---- the node-ordered histogram at every tile shape, on the node layout of the last round of the depth-9 fit
    model = models[9]
    _, _, bins = gbt.build_cuts(xt_d, 256)
    pos9 = model.train_pos_[0].clone()
    gq = torch.randint(-(1 << 20), 1 << 20, (N_TRAIN,), dtype=torch.int32, device=DEV)
    hq = torch.full((N_TRAIN,), 1 << 20, dtype=torch.int32, device=DEV)
    shapes = {}
    for level in (6, 7, 8):
        L = 1 << level
        pos = pos9.clone()
        for _ in range(9 - level):                                                # the ancestor at this level; rows that stopped above stay where they are
            pos = torch.where(pos >= 2 * L - 1, (pos - 1) // 2, pos)
        pos = pos.to(torch.int32).contiguous()
        order, skeys, seg = gbt_deep.node_order(pos, level)
        n0, n1 = gbt.plan_node_groups(WIDTH, 256, level)[0]
        hist = torch.empty(hip.query("oneprot_gbt_hist_nodes_bytes", WIDTH, 256, n1 - n0) // 8, dtype=torch.int64, device=DEV)
        rows_in_level = int(seg[L].item())
        res = {}
        for tile in (64, 32, 16, 8, 4, 2, 1):
            ts = []
            for rep in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.call("oneprot_gbt_hist_nodes", bins, gq, hq, order, skeys, seg, hist, N_TRAIN, WIDTH, 256, level, n0, n1 - n0, tile)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ts.append(e0.elapsed_time(e1) * 1e3)
            res[str(tile)] = statistics.median(ts)
        shapes[str(level)] = dict(group=[n0, n1], rows_in_level=rows_in_level, us_by_tile_features=res)
        print(json.dumps({level: shapes[str(level)]}))
    out["hist_nodes_tile_shapes"] = shapes
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged["regression"] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
    print(f"wrote {args.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=250)
    ap.add_argument("--ec-labels", type=int, default=4, help="labels sklearn fits at the EC shape (scaled to 585)")
    ap.add_argument("--profile-round", action="store_true")
    ap.add_argument("--deep", action="store_true", help="the regression workload at depths 3, 5 and 9 (with --profile-round: three depth-9 rounds for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbt_fit.json"))
    args = ap.parse_args()
    hip.lib()
    if args.deep:
        return deep(args)
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
