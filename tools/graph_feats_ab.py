#!/usr/bin/env python
"""Device against host for the featurisation of a pocket / struct_graph batch: writes profiles/graph_feats.json.

Two paths on the same records (oneprot_amd.graph_data.synthetic_atom_records: nested arrays, so no HDF5 read is counted), alternating in one process
after warm-up, every timed window closed by a device synchronise:
  host    protein_to_graph's arithmetic per record + GraphBatch.from_data_list + .to(device): what StructDataset.collate_fn does with device = None;
  device  featurize_batch(records, device): the vectorised host preparation, one pinned staging buffer, one copy, two launches (csrc/graph_feats.hip).
Also recorded: the two launches' own time (device events around the entry point), the host preparation alone, the share of the device path that is
not kernel time (preparation, staging, copy, allocation, launch), and the ProNet forward + backward on the device batch (the shipped tower of
tools/pronet_ab.py: backbone level, 4 blocks, h 128, out 1024, eval mode) on the same box, the sub-step this input feeds.
Shapes: the shipped pocket batch (16 records x 100 residues) and 16 structures of 100 .. 1000 residues.  Needs a GPU: there is no fallback.

    python tools/graph_feats_ab.py [--reps 15] [--out profiles/graph_feats.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oneprot_amd import graph_data as G   # noqa: E402
from oneprot_amd import hip               # noqa: E402
from oneprot_amd.pronet import ProNet     # noqa: E402


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), reps=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_feats.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_feats_ab.py measures the device path: no GPU, no number")
    dev = torch.device("cuda:0")
    hip.lib()
    torch.manual_seed(0)
    tower = ProNet(level="backbone", out_channels=1024).to(dev).eval()
    gen = torch.Generator().manual_seed(5)
    shapes = {"pocket_16x100": [100] * 16, "struct_graph_16x100-1000": torch.randint(100, 1001, (16,), generator=gen).tolist()}
    out = dict(device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(), reps=a.reps,
               host_path="protein_to_graph's arithmetic per record + GraphBatch.from_data_list + .to(device)",
               device_path="featurize_batch(records, device): prepare_batch + pinned staging + one copy + oneprot_graph_featurize",
               tower="ProNet backbone, 4 blocks, h 128, out 1024, eval mode, fp32, forward + backward", shapes={})
    for name, sizes in shapes.items():
        records = [G.synthetic_atom_records(n, gen) for n in sizes]
        host_fn = lambda: G.featurize_batch(records, device="cpu").to(dev)      # noqa: E731
        dev_fn = lambda: G.featurize_batch(records, device=dev)                 # noqa: E731
        for _ in range(3):                                                      # code object, pinned allocator, torch's thread pool
            host_fn()
            dev_fn()
        times = dict(host=[], device=[], prepare=[], kernel=[])
        for _ in range(a.reps):                                                 # alternate: A B A B
            times["host"].append(sync_time(host_fn)[0])
            times["device"].append(sync_time(dev_fn)[0])
            t0 = time.perf_counter()
            G.prepare_batch(records)
            times["prepare"].append((time.perf_counter() - t0) * 1e3)
        for _ in range(a.reps):                                                 # the launches' own time, in calls of their own (the events cost host time)
            hip.profile_begin("oneprot_graph_featurize")
            dev_fn()
            times["kernel"] += hip.profile_end()
        want, got = host_fn(), dev_fn()
        cot = torch.randn(len(sizes), 1024, device=dev)

        def step():
            tower.zero_grad(set_to_none=True)
            (tower(got) * cot).sum().backward()
        for _ in range(2):
            step()
        tower_ms = [sync_time(step)[0] for _ in range(max(a.reps // 2, 5))]
        rec = dict(graphs=len(sizes), residues=got.num_nodes, atoms=int(sum(len(r[1]) for r in records)), host=stats(times["host"]), device=stats(times["device"]),
                   host_preparation=stats(times["prepare"]), kernel=stats(times["kernel"]), pronet_fwd_bwd=stats(tower_ms))
        rec["host_over_device"] = rec["host"]["median_ms"] / rec["device"]["median_ms"]
        rec["share_of_device_path_outside_the_kernel"] = 1.0 - rec["kernel"]["median_ms"] / rec["device"]["median_ms"]
        rec["share_of_device_path_in_prepare_batch"] = rec["host_preparation"]["median_ms"] / rec["device"]["median_ms"]
        rec["host_over_pronet_fwd_bwd"] = rec["host"]["median_ms"] / rec["pronet_fwd_bwd"]["median_ms"]
        rec["device_over_pronet_fwd_bwd"] = rec["device"]["median_ms"] / rec["pronet_fwd_bwd"]["median_ms"]
        rec["device_faster"] = bool(rec["device"]["median_ms"] < rec["host"]["median_ms"])
        rec["copies_equal"] = all(torch.equal(torch.nan_to_num(getattr(got, k)), torch.nan_to_num(getattr(want, k))) for k in ("x", "coords_ca", "coords_n", "coords_c", "batch", "ptr"))
        rec["max_feature_difference"] = max(float((getattr(got, k) - getattr(want, k)).abs().max()) for k in ("bb_embs", "side_chain_embs"))
        out["shapes"][name] = rec
        print(f"{name}: {rec['residues']} residues, {rec['atoms']} atoms: host {rec['host']['median_ms']:.3f} ms, device {rec['device']['median_ms']:.3f} ms "
              f"(prepare_batch {rec['host_preparation']['median_ms']:.3f} ms, launches {rec['kernel']['median_ms']:.4f} ms), ProNet fwd+bwd "
              f"{rec['pronet_fwd_bwd']['median_ms']:.3f} ms, host / device {rec['host_over_device']:.1f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
