#!/usr/bin/env python
"""Host against device for the MSA depth selection: writes profiles/msa_select.json.

Host: the reference's algorithm (ref src/data/utils/msa_utils.py:21-40: one scipy `cdist(..., "hamming")` row per step, the fp64 mean over the rows chosen so
far, argmax over the unselected) restated here on numpy + scipy when scipy is importable, else the library's exact host path; the file says which.
Device: oneprot_amd.msa_data.DeviceMsaBatch (the copy of the bytes to the GPU, timed separately) + oneprot_msa_select + oneprot_msa_tokenize.
Both on the same drawn alignments (mutated copies of a query), N in --sizes, L = 512, depth 50, batches of 16, alternating in one process, every timed
window closed by a device synchronise.  The host is single-process; at sizes where the whole batch would take minutes it is timed on the first
--host-msas MSAs of the batch and the batch figure is that time scaled, marked as such.  A second table times one MSA at small N (library host path
against the device) for the crossover behind oneprot_amd.msa_data.DEVICE_MIN_BYTES.  Needs a GPU: there is no fallback."""
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

from oneprot_amd import msa_data as D  # noqa: E402

try:
    from scipy.spatial.distance import cdist
except Exception:                                             # noqa: BLE001
    cdist = None


def draw(seed, N, L):
    rng = np.random.default_rng(seed)
    rows = np.tile(rng.integers(65, 86, L, dtype=np.uint8), (N, 1))
    hit = rng.integers(0, 256, (N, L), dtype=np.uint8) < rng.integers(0, 160, (N, 1), dtype=np.uint8)
    hit[0] = False
    rows[hit] = rng.integers(65, 86, int(hit.sum()), dtype=np.uint8)
    return rows


def host_reference_algorithm(rows, depth):
    """the reference's arithmetic: fp64 Hamming fractions from scipy, their mean over the chosen rows, the best unselected row"""
    chosen, dists = [0], []
    free = np.ones(len(rows), dtype=bool)
    free[0] = False
    for _ in range(min(depth, len(rows)) - 1):
        dists.append(cdist(rows[chosen[-1]][None, :], rows, "hamming")[0])
        score = np.mean(np.stack(dists), axis=0)
        cand = np.flatnonzero(free)
        nxt = int(cand[np.argmax(score[cand])])
        chosen.append(nxt)
        free[nxt] = False
    return sorted(chosen)


def host_select(rows, depth):
    return host_reference_algorithm(rows, depth) if cdist is not None else D.select_host(rows, depth, "max")[0]


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), reps=len(xs))


def device_collate(arrays, depth, conv, dev):
    ks = [depth] * len(arrays)
    t_copy, batch = sync_time(lambda: D.DeviceMsaBatch(arrays, ks, dev))
    t_sel, idx = sync_time(lambda: batch.select("max"))
    t_tok, _ = sync_time(lambda: conv.device(batch, idx))
    return dict(copy=t_copy, select=t_sel, tokenize=t_tok, total=t_copy + t_sel + t_tok), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-msas", type=int, default=2, help="MSAs of the batch the host is timed on when N >= --host-full-below")
    ap.add_argument("--host-full-below", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msa_select.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msa_select_ab.py measures the device path: no GPU, no number")
    dev = torch.device("cuda:0")
    conv = D.MsaBatchConverter(max_length=1024)
    out = dict(device=torch.cuda.get_device_name(0), L=a.length, depth=a.depth, batch=a.batch,
               host="reference algorithm (numpy + scipy cdist, fp64 means)" if cdist is not None else "library host path (exact rule, numpy)",
               host_threads=torch.get_num_threads(), sizes={}, single_msa={})
    device_collate([draw(1, 256, a.length)] * 2, a.depth, conv, dev)                           # code objects, the pinned allocator
    for N in a.sizes:
        arrays = [draw(100 * N + b, N, a.length) for b in range(a.batch)]
        n_host = a.batch if N < a.host_full_below else min(a.host_msas, a.batch)
        host_ms, parts = [], dict(copy=[], select=[], tokenize=[], total=[])
        device_collate(arrays, a.depth, conv, dev)                                             # this size's allocations
        for rep in range(a.reps):
            t0 = time.perf_counter()
            host_idx = [host_select(arrays[b], a.depth) for b in range(n_host)]
            host_ms.append((time.perf_counter() - t0) * 1e3)
            t, idx = device_collate(arrays, a.depth, conv, dev)
            for k in parts:
                parts[k].append(t[k])
            print(f"N {N} rep {rep}: host {host_ms[-1]:.1f} ms for {n_host} MSAs; device copy {t['copy']:.2f} select {t['select']:.2f} tokenize {t['tokenize']:.2f} ms for {a.batch}",
                  flush=True)
        dev_idx = idx.cpu().tolist()
        exact = [D.select_host(arrays[b], a.depth, "max")[0] for b in range(min(2, a.batch))]
        rec = dict(N=N, row_bytes=a.batch * N * a.length, host_msas_timed=n_host, host=stats(host_ms),
                   host_batch_ms=statistics.median(host_ms) * a.batch / n_host, host_batch_is_scaled=n_host != a.batch,
                   device={k: stats(v) for k, v in parts.items()},
                   device_equals_exact_host_path=all(dev_idx[b][:len(e)] == e for b, e in enumerate(exact)),
                   msas_where_reference_algorithm_agrees=sum(dev_idx[b][:len(h)] == h for b, h in enumerate(host_idx)), msas_compared=n_host)
        rec["host_over_device"] = rec["host_batch_ms"] / rec["device"]["total"]["median_ms"]
        out["sizes"][str(N)] = rec
    for N in (64, 256, 1000, 4000):                                                            # one MSA: where the device starts to pay
        rows = draw(7 * N, N, a.length)
        h, d = [], []
        device_collate([rows], a.depth, conv, dev)
        for _ in range(max(a.reps, 5)):
            t0 = time.perf_counter()
            D.select_host(rows, a.depth, "max")
            h.append((time.perf_counter() - t0) * 1e3)
            ks = [a.depth]
            d.append(sync_time(lambda: D.DeviceMsaBatch([rows], ks, dev).select("max"))[0])
        out["single_msa"][str(N)] = dict(row_bytes=N * a.length, library_host_path=stats(h), device_copy_and_select=stats(d))
        print(f"single MSA N {N}: library host path {statistics.median(h):.2f} ms, device {statistics.median(d):.2f} ms", flush=True)
    enc = os.path.join(ROOT, "profiles", "msa_encoder.json")
    if os.path.exists(enc) and "10000" in out["sizes"]:
        with open(enc) as f:
            fwd = json.load(f)["b16_r50_l512"]["hip"]["median_ms"]
        out["next_to_the_tower"] = dict(tower_forward_b16_r50_l512_ms=fwd, source="profiles/msa_encoder.json",
                                        device_collate_b16_n10000_ms=out["sizes"]["10000"]["device"]["total"]["median_ms"])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["host_batch_ms"], v["device"]["total"]["median_ms"]) for k, v in out["sizes"].items()}))


if __name__ == "__main__":
    main()
