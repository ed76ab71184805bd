#!/usr/bin/env python3
"""A/B of the ProNet tower: forward + backward on the HIP kernels (oneprot_amd/pronet.py) against the plain-torch restatement (tests/pronet_ref.py) run
in fp32 on the same GPU, on the same batches, alternating in one process.  Writes profiles/pronet.json: time and peak memory of both, their ratios, and
the HIP step's time per entry point.

Shapes: the reference's pocket batch (16 graphs x 100 residues) and a struct_graph batch (16 graphs of 100 .. 1000 residues), synthetic backbones
(oneprot_amd.graph_data.synthetic_protein).  The tower is the shipped configuration (backbone level, 4 blocks, h = 128) in eval mode, so that both
sides compute the same function.  The HIP step includes building the graph and the edge features on the device; the restatement is handed the graph
(its own radius graph is a host loop) and builds its features in torch inside the timed region.

    python tools/pronet_ab.py [--reps 7] [--out profiles/pronet.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oneprot_amd import hip                                                       # noqa: E402
from oneprot_amd.graph_data import GraphBatch, synthetic_protein                  # noqa: E402
from oneprot_amd.pronet import ProNet                                             # noqa: E402
from tests import pronet_ref as R                                                 # noqa: E402

DEV = "cuda:0"
ENTRY_POINTS = ["oneprot_radius_graph", "oneprot_graph_by_source", "oneprot_pronet_edge_features", "oneprot_edge_conv_fwd", "oneprot_edge_conv_bwd_x",
                "oneprot_edge_conv_bwd_w", "oneprot_sgemm", "oneprot_wgrad_f32", "oneprot_pronet_bias_act", "oneprot_pronet_act_bwd", "oneprot_colsum_f32",
                "oneprot_dropout_add_f32", "oneprot_pronet_embed_fwd", "oneprot_segment_sum_f32", "oneprot_segment_sum_bwd_f32"]


def make_batch(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return GraphBatch.from_data_list([synthetic_protein(n, gen) for n in sizes])


def timed(fn, reps):
    """(median ms, peak MiB above what was allocated before) of fn over `reps` runs after two warm-up runs"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pronet.json"))
    args = ap.parse_args()
    hip.lib()
    torch.manual_seed(0)
    tower = ProNet(level="backbone", out_channels=1024).to(DEV).eval()
    cfg = dict(num_blocks=4, num_radial=6, num_pos_emb=16, cutoff=10.0, max_num_neighbors=32, int_emb_layers=3, out_layers=2)
    gen = torch.Generator().manual_seed(5)
    shapes = {"pocket_16x100": [100] * 16, "struct_graph_16x100-1000": torch.randint(100, 1001, (16,), generator=gen).tolist()}
    result = {"device": torch.cuda.get_device_name(0), "tower": "ProNet backbone, 4 blocks, h 128, out 1024, eval mode, fp32", "reps": args.reps, "shapes": {}}
    for name, sizes in shapes.items():
        host = make_batch(sizes, 11)
        batch = host.to(DEV)
        graph = R.radius_graph(host.coords_ca.numpy(), host.ptr.numpy(), cfg["cutoff"], cfg["max_num_neighbors"])
        cot = torch.randn(len(sizes), 1024, device=DEV)
        params = {k: v.detach().clone().requires_grad_() for k, v in tower.state_dict().items()}

        def hip_step():
            tower.zero_grad(set_to_none=True)
            (tower(batch) * cot).sum().backward()

        def torch_step():
            for p in params.values():
                p.grad = None
            (R.forward(params, batch, dtype=torch.float32, graph=graph, **cfg) * cot).sum().backward()
        rows = []
        for _ in range(2):                                                        # alternate: A B A B
            rows.append((timed(hip_step, args.reps), timed(torch_step, args.reps)))
        hip_ms, hip_mib = min(r[0][0] for r in rows), max(r[0][1] for r in rows)
        torch_ms, torch_mib = min(r[1][0] for r in rows), max(r[1][1] for r in rows)
        # agreement of the two sides on this batch (output, relative L2)
        with torch.no_grad():
            a, b = tower(batch), R.forward(params, batch, dtype=torch.float32, graph=graph, **cfg)
        hip.profile_begin({k: None for k in ENTRY_POINTS})
        hip_step()
        prof = hip.profile_end()
        per_kernel = {k: {"launches": len(v), "ms": round(sum(ms for ms, _ in v), 4)} for k, v in prof.items() if v}
        forms = {(0, 0): "forward x W^T", (0, 1): "data gradient dz W", (1, 1): "weight gradient dz^T x (contraction over the nodes)", (1, 0): "folded operand W1^T W2^T"}
        by_form = {}
        for ms, sc in prof["oneprot_sgemm"]:                                      # scalar arguments: M, N, K, transA, b_is_kn, alpha, accumulate
            row = by_form.setdefault(forms[(sc[3], sc[4])], {"launches": 0, "ms": 0.0})
            row["launches"], row["ms"] = row["launches"] + 1, round(row["ms"] + ms, 4)
        result["shapes"][name] = {
            "graphs": len(sizes), "nodes": host.num_nodes, "edges": int(graph[1].sum()),
            "hip_fwd_bwd_ms": round(hip_ms, 3), "torch_fp32_fwd_bwd_ms": round(torch_ms, 3), "time_ratio_hip_over_torch": round(hip_ms / torch_ms, 4),
            "hip_peak_mib": round(hip_mib, 1), "torch_fp32_peak_mib": round(torch_mib, 1), "memory_ratio_hip_over_torch": round(hip_mib / torch_mib, 4),
            "output_rel_l2_hip_vs_torch_fp32": float((a - b).norm() / b.norm()), "hip_ms_per_entry_point": per_kernel, "sgemm_ms_by_form": by_form,
            "hip_no_slower": bool(hip_ms <= torch_ms), "hip_lower_peak_memory": bool(hip_mib < torch_mib)}
        print(name, json.dumps(result["shapes"][name]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
