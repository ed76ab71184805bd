#!/usr/bin/env python3
"""Streaming retrieval against the matrix path, and the streaming kernels at database scale -> profiles/retrieval_stream.json.

One process, device-synchronised; every shape is warmed up, then every variant is timed `--reps` (>= 5) times, the variants of a shape alternating.
  ranks_16k    N = 16 384, D = 1024: retrieval.pair_ranks against oneprot_sgemm + oneprot_diag_rank (both fit), the ranks' equality, and the GATE:
               the streaming median may exceed the matrix median by no more than the larger of the two spreads (max - min)
  ranks_131k   N = 131 072, D = 1024, streaming alone: time and fp32 FLOP/s (2 N^2 D) against the 157.3 TF peak
  topk_1m      nq = 4096, N = 1 048 576, D = 1024, k = 100: time and FLOP/s (2 nq N D)
The merge kernel's share of the top-k time comes from a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/retrieval_ab.py --only topk_1m --reps 1 --out /dev/null
  python tools/retrieval_ab.py --fold-trace DIR            (adds topk_1m.merge_share to the JSON written before)
usage: retrieval_ab.py [--only NAME[,NAME]] [--reps 5] [--out profiles/retrieval_stream.json] [--small]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32 = 157.3e12


def timed(fn, reps_list):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    reps_list.append(a.elapsed_time(b))
    return out


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def features(n, d, seed, scale=1.0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, device="cuda", generator=g)
    x /= x.norm(dim=1, keepdim=True)
    if scale != 1.0:
        x *= scale
    return x


def ranks_16k(reps, small):
    import torch
    from oneprot_amd import metrics, retrieval
    N, D = (2048, 256) if small else (16384, 1024)
    s, m = features(N, D, 1), features(N, D, 2, 1 / 0.07)
    variants = {"matrix": lambda: metrics._ranks_matrix(s, m), "stream": lambda: retrieval.pair_ranks(s, m)}
    res = {k: f() for k, f in variants.items()}                    # warm-up (and the results to compare)
    torch.cuda.synchronize()
    equal = bool(torch.equal(res["matrix"][0], res["stream"][0]) and torch.equal(res["matrix"][1], res["stream"][1]))
    del res
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():                              # alternating
            timed(f, ms[k])
    out = {"N": N, "D": D, "ranks_equal": equal, "matrix": stats(ms["matrix"]), "stream": stats(ms["stream"])}
    flops = 2.0 * N * N * D
    for k in ("matrix", "stream"):
        out[k]["tflops"] = flops / (out[k]["median_ms"] * 1e-3) / 1e12
    allowed = max(out["matrix"]["spread_ms"], out["stream"]["spread_ms"])
    out["gate"] = {"rule": "stream median <= matrix median + max(spread of either)", "allowed_ms": allowed,
                   "passed": bool(out["stream"]["median_ms"] <= out["matrix"]["median_ms"] + allowed and equal)}
    return out


def ranks_131k(reps, small):
    import torch
    from oneprot_amd import retrieval
    N, D = (8192, 256) if small else (131072, 1024)
    s, m = features(N, D, 3), features(N, D, 4, 1 / 0.07)
    slab = retrieval.default_slab_rows(N, D)
    retrieval.pair_ranks(s, m)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        rr, rc = timed(lambda: retrieval.pair_ranks(s, m), ms)
    out = {"N": N, "D": D, "slab_rows": slab, "launches": -(-N // slab), **stats(ms)}
    out["tflops"] = 2.0 * N * N * D / (out["median_ms"] * 1e-3) / 1e12
    out["fraction_of_fp32_peak"] = out["tflops"] * 1e12 / PEAK_FP32
    out["R@1_row"] = float((rr < 1).float().mean())
    return out


def topk_1m(reps, small):
    import torch
    from oneprot_amd import hip, retrieval
    nq, N, D, k = (256, 65536, 256, 100) if small else (4096, 1 << 20, 1024, 100)
    q, db = features(nq, D, 5), features(N, D, 6)
    retrieval.topk(q, db, k)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        scores, idx = timed(lambda: retrieval.topk(q, db, k), ms)
    out = {"nq": nq, "N": N, "D": D, "k": k, "workspace_bytes": int(hip.query("oneprot_sim_topk_workspace", nq, N, k)), **stats(ms)}
    out["tflops"] = 2.0 * nq * N * D / (out["median_ms"] * 1e-3) / 1e12
    out["fraction_of_fp32_peak"] = out["tflops"] * 1e12 / PEAK_FP32
    out["descending"] = bool((scores[:, 1:] <= scores[:, :-1]).all())
    return out


def fold_trace(trace_dir, out_path):
    tot = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("Name") or ""
                if "k_sim_topk" in name:
                    key = "merge" if "merge" in name else "select"
                    tot[key] = tot.get(key, 0) + int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
    if "merge" not in tot or "select" not in tot:
        sys.exit(f"no k_sim_topk dispatches in a *kernel_trace.csv under {trace_dir}")
    doc = json.load(open(out_path))
    doc["topk_1m"]["merge_share"] = tot["merge"] / (tot["merge"] + tot["select"])
    doc["topk_1m"]["trace_ns"] = tot
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc["topk_1m"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ranks_16k,ranks_131k,topk_1m")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_stream.json"))
    ap.add_argument("--small", action="store_true", help="small shapes: a dry run of the tool, not a measurement")
    ap.add_argument("--fold-trace", default=None)
    a = ap.parse_args()
    if a.fold_trace:
        return fold_trace(a.fold_trace, a.out)
    import torch
    doc = {"device": torch.cuda.get_device_name(0), "small_shapes": a.small, "fp32_peak_tflops": PEAK_FP32 / 1e12}
    for name in a.only.split(","):
        doc[name] = {"ranks_16k": ranks_16k, "ranks_131k": ranks_131k, "topk_1m": topk_1m}[name](a.reps, a.small)
        print(name, json.dumps(doc[name]), flush=True)
        torch.cuda.empty_cache()
    if a.out != "/dev/null":
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
