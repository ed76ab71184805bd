#!/usr/bin/env python3
"""The MSA tower forward on the HIP kernels against the only alternative a user of this tree has -- the torch restatement tests/msa_ref.py on the same
device under bf16 autocast -> profiles/msa_encoder.json.

One process, device-synchronised; each shape is warmed up, then both variants are timed `--reps` (>= 5) times, alternating.  Published architecture
(12 layers, d 768, 12 heads, FFN 3072), random weights, ragged synthetic MSAs:
  b16_r50_l512    B = 16, R = 50, L = 512  (the reference's batch: configs/data/modalities/msa.yaml)
  b4_r50_l1024    B = 4,  R = 50, L = 1024
GATE, recorded per shape: the HIP median is lower than the torch median by more than the larger of the two spreads (max - min).  A miss is a defect of the
new kernels and is reported as such.
Per-kernel shares come from a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/msa_ab.py --only b16_r50_l512 --reps 1 --hip-only --out /dev/null
  python tools/msa_ab.py --fold-trace DIR            (adds kernel_shares to the JSON written before)
--dropout: a second comparison at the same two shapes, HIP against HIP -- the default forward and the forward with fair-esm's train-mode dropouts
(`drop=True`: masked row / column probabilities, six Philox passes per layer), alternating in one process; the medians and their ratio are ADDED to the JSON
written before under "dropout_ab" (the other keys stay).  A record of the cost, not a gate.
--ragged: a third comparison at the same two shapes, HIP against HIP -- the padded [B, R, L] batch against the same MSAs as an oneprot_amd.packing.PackedMsa
(each MSA at its own depth and length), alternating in one process; ADDED to the JSON written before under "ragged_ab".  Two cases per shape: "ragged", the
MSAs drawn by SyntheticPairs' ragged rule (seed 50) -- GATE: the packed median is lower than the padded median by more than the larger of the two spreads --
and "control", the same frames with no padding at all, where only the packed / padded ratio is recorded (the cost of the geometry decoder at full blocks).
usage: msa_ab.py [--only NAME[,NAME]] [--reps 5] [--out profiles/msa_encoder.json] [--small] [--hip-only] [--dropout] [--ragged]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"b16_r50_l512": (16, 50, 512), "b4_r50_l1024": (4, 50, 1024)}
SMALL = {"b16_r50_l512": (2, 6, 96), "b4_r50_l1024": (1, 6, 160)}


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


def run_shape(tr, sd, name, reps, small, hip_only):
    import torch
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.msa import plan_groups
    from tests import msa_ref as MR
    B, R, L = (SMALL if small else SHAPES)[name]
    tok = SyntheticPairs._msa_frame(torch.Generator().manual_seed(50), B, R, L, True).cuda()
    n = tr.n_layers

    def hip_fwd():
        return tr(tok)["representations"][n]

    def torch_fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return MR.forward(tok, sd, tr.H, dtype=torch.float32)

    variants = {"hip": hip_fwd} if hip_only else {"hip": hip_fwd, "torch_bf16_autocast": torch_fwd}
    res = {k: f().float() for k, f in variants.items()}                # warm-up (and the outputs to compare)
    torch.cuda.synchronize()
    out = {"B": B, "R": R, "L": L, "tokens": B * R * L, "score_groups": len(plan_groups(B, R, L, tr.H))}
    if not hip_only:
        m = tok.ne(1).unsqueeze(-1)
        a, b = res["hip"] * m, res["torch_bf16_autocast"] * m
        out["hidden_cosine_hip_vs_torch"] = float(torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0))
    del res                                                            # (the allocator keeps its blocks: the timed repetitions do not pay hipMalloc)
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():                                  # alternating
            timed(f, ms[k])
    for k in variants:
        out[k] = stats(ms[k])
    if not hip_only:
        allowed = max(out["hip"]["spread_ms"], out["torch_bf16_autocast"]["spread_ms"])
        out["gate"] = {"rule": "hip median < torch median - max(spread of either)", "margin_ms": allowed,
                       "passed": bool(out["hip"]["median_ms"] < out["torch_bf16_autocast"]["median_ms"] - allowed)}
    return out


def run_dropout_ab(tr, name, reps, small):
    """the default forward against the forward with the train-mode dropouts: same tokens, alternating"""
    import torch
    from oneprot_amd.data import SyntheticPairs
    B, R, L = (SMALL if small else SHAPES)[name]
    tok = SyntheticPairs._msa_frame(torch.Generator().manual_seed(50), B, R, L, True).cuda()
    n = tr.n_layers
    variants = {"hip": lambda: tr(tok)["representations"][n], "hip_dropout": lambda: tr(tok, drop=True)["representations"][n]}
    for f in variants.values():                                        # warm-up
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            timed(f, ms[k])
    out = {"B": B, "R": R, "L": L, "tokens": B * R * L, "probabilities": list(tr._drop_probs())}
    for k in variants:
        out[k] = stats(ms[k])
    out["dropout_over_default"] = out["hip_dropout"]["median_ms"] / out["hip"]["median_ms"]
    return out


def run_ragged_ab(tr, name, reps, small):
    """padded against packed on the same MSAs: the ragged draw (gated) and the full frames (control)"""
    import torch
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.packing import PackedMsa
    B, R, L = (SMALL if small else SHAPES)[name]
    n = tr.n_layers
    out = {"B": B, "R": R, "L": L}
    for case, ragged in (("ragged", True), ("control", False)):
        tok = SyntheticPairs._msa_frame(torch.Generator().manual_seed(50), B, R, L, ragged).cuda()
        pk = PackedMsa.from_padded(tok)
        variants = {"padded": lambda: tr(tok)["representations"][n], "packed": lambda: tr(pk)["representations"][n]}
        res = {k: f() for k, f in variants.items()}                    # warm-up (builds the packed batch's device tables once, as a data loader's batch would carry them)
        torch.cuda.synchronize()
        diff = max(float((a - b[:r, :l]).abs().max()) for a, b, (r, l) in zip(pk.unpack(res["packed"]), res["padded"], pk.shapes))
        del res
        ms = {k: [] for k in variants}
        for _ in range(reps):
            for k, f in variants.items():                              # alternating
                timed(f, ms[k])
        c = out[case] = {"tokens_padded": B * R * L, "tokens_packed": pk.n_tokens, "stream_rows": pk.T_pad, "token_ratio": pk.T_pad / (B * R * L),
                         "score_element_ratio": sum(l * l for _, l in pk.shapes) / (B * L * L),
                         "score_work_ratio": sum(r * l * l for r, l in pk.shapes) / (B * R * L * L), "max_abs_difference_packed_vs_padded": diff}
        for k in variants:
            c[k] = stats(ms[k])
        c["packed_over_padded"] = c["packed"]["median_ms"] / c["padded"]["median_ms"]
        if ragged:
            allowed = max(c["padded"]["spread_ms"], c["packed"]["spread_ms"])
            c["gate"] = {"rule": "packed median < padded median - max(spread of either)", "margin_ms": allowed,
                         "passed": bool(c["packed"]["median_ms"] < c["padded"]["median_ms"] - allowed)}
        torch.cuda.empty_cache()
    return out


def fold_trace(trace_dir, out_path):
    groups = (("k_msa_row_scores", "msa_row_scores"), ("k_msa_row_softmax", "msa_row_context"), ("k_msa_v_transpose", "msa_row_context"),
              ("k_msa_row_pv", "msa_row_context"), ("k_msa_col_attn", "msa_col_attn"), ("k_msa_embed", "msa_embed"),
              ("gemm", "nt_gemm"), ("layernorm", "layernorm"), ("lnpool", "layernorm"))
    tot = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("Name") or ""
                key = next((g for pat, g in groups if pat in name), "other")
                tot[key] = tot.get(key, 0) + int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
    if not any(k.startswith("msa_") for k in tot):
        sys.exit(f"no k_msa_* dispatches in a *kernel_trace.csv under {trace_dir}")
    total = sum(tot.values())
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["kernel_shares"] = {"note": "whole traced process (warm-up + 1 repetition, HIP variant only)", "trace_ns": tot,
                            "share": {k: v / total for k, v in sorted(tot.items(), key=lambda kv: -kv[1])}}
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc["kernel_shares"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msa_encoder.json"))
    ap.add_argument("--small", action="store_true", help="small shapes: a dry run of the tool, not a measurement")
    ap.add_argument("--hip-only", action="store_true", help="run the HIP variant alone (for the kernel trace)")
    ap.add_argument("--fold-trace", default=None)
    ap.add_argument("--dropout", action="store_true", help="default forward against the forward with the train-mode dropouts; adds dropout_ab to --out")
    ap.add_argument("--ragged", action="store_true", help="padded batch against the same MSAs as a PackedMsa; adds ragged_ab to --out")
    a = ap.parse_args()
    if a.fold_trace:
        return fold_trace(a.fold_trace, a.out)
    import torch
    from oneprot_amd.msa import MsaTransformer
    os.environ["ONEPROT_ALLOW_RANDOM_INIT"] = "1"
    warnings.filterwarnings("ignore", message=".*no weight file.*")
    torch.manual_seed(0)
    tr = MsaTransformer.from_pretrained("esm_msa1b_t12_100M_UR50S.pt").cuda()
    if a.dropout:
        doc = json.load(open(a.out)) if a.out != "/dev/null" and os.path.exists(a.out) else {}
        ab = doc["dropout_ab"] = {"device": torch.cuda.get_device_name(0), "small_shapes": a.small,
                                  "variants": "MsaTransformer.forward(tokens) against forward(tokens, drop=True), alternating in one process"}
        for name in a.only.split(","):
            ab[name] = run_dropout_ab(tr, name, max(a.reps, 1), a.small)
            print(name, json.dumps(ab[name]), flush=True)
            torch.cuda.empty_cache()
        if a.out != "/dev/null":
            json.dump(doc, open(a.out, "w"), indent=1)
        return
    if a.ragged:
        doc = json.load(open(a.out)) if a.out != "/dev/null" and os.path.exists(a.out) else {}
        ab = doc["ragged_ab"] = {"device": torch.cuda.get_device_name(0), "small_shapes": a.small,
                                 "variants": "MsaTransformer.forward(tokens [B, R, L]) against forward(PackedMsa.from_padded(tokens)), alternating in one process"}
        for name in a.only.split(","):
            ab[name] = run_ragged_ab(tr, name, max(a.reps, 1), a.small)
            print(name, json.dumps(ab[name]), flush=True)
        if a.out != "/dev/null":
            json.dump(doc, open(a.out, "w"), indent=1)
        return
    sd = {k: v.detach() for k, v in tr.state_dict().items() if not k.startswith(("lm_head.", "contact_head."))}
    doc = {"device": torch.cuda.get_device_name(0), "small_shapes": a.small, "weights": "random (published architecture)",
           "torch_variant": "tests/msa_ref.py forward, fp32 weights, torch.autocast(bfloat16)"}
    for name in a.only.split(","):
        doc[name] = run_shape(tr, sd, name, max(a.reps, 1), a.small, a.hip_only)
        print(name, json.dumps(doc[name]), flush=True)
        torch.cuda.empty_cache()
    if a.out != "/dev/null":
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
