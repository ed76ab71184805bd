#!/usr/bin/env python3
"""A/B of one fit epoch of the downstream MLP probe: the HIP path of oneprot_amd/probe.py (fused "few rows" kernels, one AdamW launch, no autograd) against a
plain-torch fp32 restatement on the same GPU (nn.Sequential, F.binary_cross_entropy_with_logits, torch.optim.AdamW), alternating in one process.  The opponent
is torch eager because the reference's own loop needs Lightning, which is not installed; the parent commit has no such path to compare with.

Workload: the EC shape on synthetic data -- 15,000 x 1280 training embeddings, 1,700 validation, 585 labels -- hidden [512, 256], BatchNorm, ReLU, dropout
0.25, batch 32 and 64.  An epoch is what fit() runs: a device permutation, every batch as an index range of it (the tail kept), the eval-mode validation
loss, one readback.  Timing is by device events around whole epochs after a warm-up epoch of each side; `--reps` rounds of 2 epochs each, the median and the
spread (min .. max) per side.  The launch boundary: `launches` per step (counted at hip.call, the loss counts twice, the BatchNorm counters once) times the
measured cost of one dependent launch (a chain of 1-element AdamW steps), as a share of the HIP epoch.

    python tools/probe_ab.py [--reps 3] [--out profiles/probe_fit.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oneprot_amd import hip, probe                                                # noqa: E402
from oneprot_amd.optim import FusedAdamW                                          # noqa: E402

DEV = "cuda:0"
N_TRAIN, N_VALID, WIDTH, LABELS, HIDDEN, DROPOUT, LR = 15000, 1700, 1280, 585, [512, 256], 0.25, 1e-3


def timed_epochs(fn, epochs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(epochs):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / epochs


def launch_gap_us(n=2000):
    """cost of one dependent launch: a chain of n one-element AdamW steps"""
    t = [torch.zeros(1, device=DEV) for _ in range(4)]
    for _ in range(50):
        hip.call("oneprot_adamw_step", *t, 1, 1e-3, 0.1, 0.001, 1e-8, 0.01, 1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        hip.call("oneprot_adamw_step", *t, 1, 1e-3, 0.1, 0.001, 1e-8, 0.01, 1)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_fit.json"))
    args = ap.parse_args()
    hip.lib()
    gen = torch.Generator().manual_seed(0)
    xt, xv = torch.randn(N_TRAIN, WIDTH, generator=gen).to(DEV), torch.randn(N_VALID, WIDTH, generator=gen).to(DEV)
    yt, yv = (torch.rand(N_TRAIN, LABELS, generator=gen) < 0.02).float().to(DEV), (torch.rand(N_VALID, LABELS, generator=gen) < 0.02).float().to(DEV)
    gap = launch_gap_us()
    out = {"workload": dict(train=N_TRAIN, valid=N_VALID, width=WIDTH, labels=LABELS, hidden=HIDDEN, norm="batch", activation="relu", dropout=DROPOUT, lr=LR),
           "device": torch.cuda.get_device_name(0), "launch_gap_us": gap, "epochs_per_round": args.epochs, "rounds": args.reps, "batch": {}}
    for bs in (32, 64):
        torch.manual_seed(1)
        model = probe.MLP(WIDTH, LABELS, HIDDEN, DROPOUT, True, False, "relu", False).to(DEV)
        opt = FusedAdamW([model.arena()], lr=LR)
        sums, ws = torch.zeros(2, dtype=torch.float64, device=DEV), hip.probe_loss_workspace(DEV)
        g = torch.Generator(device=DEV).manual_seed(2)
        hip_loss = []

        def epoch_hip():
            model.train()
            perm = torch.randperm(N_TRAIN, generator=g, device=DEV).to(torch.int32)
            sums.zero_()
            for s in range(0, N_TRAIN, bs):
                model.train_step(xt, yt, perm[s:s + bs], hip.PROBE_LOSS_BCE, opt, sums[0:1], ws)
            model.eval()
            model.eval_loss(xv, yv, hip.PROBE_LOSS_BCE, sums[1:2], ws)
            hip_loss.append(sums.cpu().tolist()[1] / N_VALID)

        torch.manual_seed(1)
        ref = nn.Sequential(nn.Linear(WIDTH, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(DROPOUT), nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(),
                            nn.Dropout(DROPOUT), nn.Linear(256, LABELS)).to(DEV)
        ropt = torch.optim.AdamW(ref.parameters(), lr=LR)
        g2 = torch.Generator(device=DEV).manual_seed(2)
        torch_loss = []

        def epoch_torch():
            ref.train()
            perm = torch.randperm(N_TRAIN, generator=g2, device=DEV)
            for s in range(0, N_TRAIN, bs):
                idx = perm[s:s + bs]
                loss = F.binary_cross_entropy_with_logits(ref(xt[idx]), yt[idx])
                ropt.zero_grad(set_to_none=True)
                loss.backward()
                ropt.step()
            ref.eval()
            with torch.no_grad():
                total = torch.zeros((), device=DEV)
                for s in range(0, N_VALID, probe.EVAL_SLAB):
                    total += F.binary_cross_entropy_with_logits(ref(xv[s:s + probe.EVAL_SLAB]), yv[s:s + probe.EVAL_SLAB]) * min(probe.EVAL_SLAB, N_VALID - s)
            torch_loss.append(float(total.cpu()) / N_VALID)

        calls, real = [], hip.call
        epoch_hip()                                                                # warm-up epochs
        epoch_torch()
        hip.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        model.train()
        model.train_step(xt, yt, torch.arange(bs, dtype=torch.int32, device=DEV), hip.PROBE_LOSS_BCE, opt, sums[0:1], ws)
        hip.call = real
        launches = len(calls) + calls.count("oneprot_probe_loss_fwd_bwd") + 1     # the loss is two launches; the BatchNorm step counters one foreach launch
        t_hip, t_torch = [], []
        for _ in range(args.reps):
            t_hip.append(timed_epochs(epoch_hip, args.epochs))
            t_torch.append(timed_epochs(epoch_torch, args.epochs))
        steps = (N_TRAIN + bs - 1) // bs
        mh, mt = statistics.median(t_hip), statistics.median(t_torch)
        out["batch"][str(bs)] = dict(steps_per_epoch=steps, launches_per_step=launches, hip_epoch_ms=dict(median=mh, min=min(t_hip), max=max(t_hip)),
                                     torch_epoch_ms=dict(median=mt, min=min(t_torch), max=max(t_torch)), torch_over_hip=mt / mh,
                                     hip_us_per_step=mh * 1e3 / steps, torch_us_per_step=mt * 1e3 / steps,
                                     launch_boundary_share_of_hip_epoch=launches * gap * steps / (mh * 1e3), val_loss_hip=hip_loss, val_loss_torch=torch_loss)
        print(json.dumps({"batch": bs, **out["batch"][str(bs)]}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
