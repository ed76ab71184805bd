"""Activation recomputation off against on (segments of k layers), in one process, on identical data (EsmTransformer.recompute_layers; DESIGN.md section 6,
"Recomputation").

cfg-2 shapes: ESM-2-150M x2 (sequence tower frozen, struct-token tower trainable), L = 512, 256 pairs per sub-step.  The sides -- off, k = 3, 6, 10 --
alternate sub-step by sub-step on ONE module, so clock and power drift fall on all alike; each side is timed between HIP events around its own sub-steps,
and its peak memory is torch.cuda.max_memory_allocated over that sub-step (the counter is reset before it).

  cfg2      the sub-step above, every side
  big_650m  one trainable ESM-2-650M tower, 256 sequences of L = 1024, forward + backward, k = 3.  Its off side is COUNTED above the 288 GB of the device
            (every layer's record: 32 d + 16 + 4 H bytes per token and layer), so only the on side runs; the off side is reported as counted bytes,
            "not run"

Every case also carries the counted bytes (activation_bytes below: from the allocations of oneprot_amd/esm.py, not measured).  --tiny swaps in 6-layer,
320-wide towers and a small batch (a functional run of the tool itself); --count-only prints the counted table and needs no GPU.

usage: python tools/recompute_ab.py [--steps 4] [--out profiles/recompute_ab.json]
"""
import argparse
import functools
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEVICE_BYTES = 288e9


def activation_bytes(T, d, H, n_layers, k=0):
    """counted bytes a trainable tower holds for its backward on T tokens: per layer and token x_mid + x_out (fp32, x_in is the layer below's x_out),
    h1 q k v ctx h2 (bf16, d each) and u (bf16, f = 4 d), the one-byte gelu' codes (f), four row statistics and lse per head: 32 d + 16 + 4 H; per boundary
    record x_in (fp32), h1 (bf16) and two statistics: 6 d + 8.  With recomputation the peak holds one segment of k layers and a record per lower segment."""
    layer, bound = (32 * d + 16 + 4 * H) * T, (6 * d + 8) * T
    if not k or k >= n_layers:
        return dict(per_layer=layer, per_boundary=bound, kept_layers=n_layers, boundaries=0, total=n_layers * layer)
    segs = -(-n_layers // k)
    return dict(per_layer=layer, per_boundary=bound, kept_layers=k, boundaries=segs - 1, total=k * layer + (segs - 1) * bound)


def extra_forward_share(n_layers, k):
    """layers a backward with recomputation runs again, as a share of one tower forward: every segment but the top one"""
    if not k or k >= n_layers:
        return 0.0
    top = n_layers - (-(-n_layers // k) - 1) * k
    return round((n_layers - top) / n_layers, 3)


def _tiny_dir(tmp):
    path = os.path.join(tmp, "esm_tiny")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="esm", vocab_size=33, hidden_size=320, num_hidden_layers=6, num_attention_heads=20, intermediate_size=1280), f)
    return path


def build_pair(name, dev):
    import torch
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.struct_token_encoder import StructTokenEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(1881)
    seq = SequenceEncoder(name, output_dim=1024, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=True)
    st = StructTokenEncoder(name, output_dim=1024, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    m = OneProtLitModule(components={"sequence": seq, "struct_token": st}, optimizer=functools.partial(FusedAdam, lr=1e-3, weight_decay=0.0), loss_fn="CLIP",
                         use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(dev)
    m.train()
    return m


def timed_sides(sides, steps, warm=1):
    """sides: {label: fn}; the sides alternate sub-step by sub-step.  Per side: median seconds between HIP events, every step's seconds, peak bytes."""
    import torch
    for _ in range(warm):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    secs, peak = {s: [] for s in sides}, {s: 0 for s in sides}
    for _ in range(steps):
        for label, fn in sides.items():
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            secs[label].append(e0.elapsed_time(e1) * 1e-3)
            peak[label] = max(peak[label], torch.cuda.max_memory_allocated())
    med = lambda v: sorted(v)[len(v) // 2]
    return {s: dict(s=round(med(secs[s]), 5), peak_bytes=peak[s], steps_s=[round(x, 5) for x in secs[s]]) for s in sides}


def case_cfg2(name, B, L, ks, steps):
    import torch
    from oneprot_amd.data import SyntheticPairs
    dev = torch.device("cuda")
    module = build_pair(name, dev)
    enc = module.network["struct_token"]
    tr = enc.transformer
    rag = next(iter(SyntheticPairs("struct_token", B, L, seed=1881, ragged=True)))
    batch = {"struct_token": (rag[0].to(dev), rag[1].to(dev), "struct_token", None)}

    def side(k):
        def fn():
            enc.set_activation_recompute(k)
            module.training_step(batch, 0)
        return fn

    res = timed_sides({("off" if k == 0 else f"k{k}"): side(k) for k in [0] + list(ks)}, steps)
    enc.set_activation_recompute(None)
    off = res["off"]
    off.update(pairs_per_s=round(B / off["s"], 1), counted=activation_bytes(B * L, tr.d, tr.H, tr.n_layers))
    for k in ks:
        r = res[f"k{k}"]
        r.update(pairs_per_s=round(B / r["s"], 1), time_over_off=round(r["s"] / off["s"], 3), peak_saved_bytes=off["peak_bytes"] - r["peak_bytes"],
                 counted=activation_bytes(B * L, tr.d, tr.H, tr.n_layers, k), extra_forward_share=extra_forward_share(tr.n_layers, k))
    out = dict(pairs=B, L=L, tower=dict(layers=tr.n_layers, d=tr.d, heads=tr.H), **res)
    del module
    torch.cuda.empty_cache()
    return out


def case_big(name, B, L, k, steps):
    """one trainable tower whose kept activations are counted above the device's memory: the on side alone"""
    import torch
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.esm import resolve_config
    from src.models.components.sequence_encoder import SequenceEncoder
    cfg, _ = resolve_config(name)
    d, H, n = cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers
    counted_off, counted_on = activation_bytes(B * L, d, H, n), activation_bytes(B * L, d, H, n, k)
    out = dict(sequences=B, L=L, tower=dict(layers=n, d=d, heads=H), off=dict(status="not run", counted=counted_off,
                                                                                counted_over_device=round(counted_off["total"] / DEVICE_BYTES, 3)))
    if counted_off["total"] <= DEVICE_BYTES:
        out["off"]["status"] = "not run (counted below the device's memory at this size: a functional run of the on side only)"
    dev = torch.device("cuda")
    torch.manual_seed(1881)
    enc = SequenceEncoder(name, output_dim=1024, pooling_type="mean", proj_type="linear", use_lora=False, frozen=False).to(dev).train()
    enc.set_activation_recompute(k)
    ids = next(iter(SyntheticPairs("sequence", B, L, seed=7, ragged=False)))[0].to(dev)
    w = torch.randn(B, 1024, device=dev)

    def fn():
        enc.zero_grad(set_to_none=True)
        (enc(ids) * w).sum().backward()

    res = timed_sides({f"k{k}": fn}, steps)[f"k{k}"]
    res.update(seq_per_s=round(B / res["s"], 1), counted=counted_on, extra_forward_share=extra_forward_share(n, k))
    out[f"k{k}"] = res
    del enc
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--big-len", type=int, default=1024)
    ap.add_argument("--ks", type=int, nargs="+", default=[3, 6, 10])
    ap.add_argument("--tiny", action="store_true", help="6-layer 320-wide towers, 8 pairs of 128 / 256 tokens: a functional run of the tool")
    ap.add_argument("--count-only", action="store_true", help="the counted bytes alone (no GPU)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ["ONEPROT_ALLOW_RANDOM_INIT"] = "1"
    import warnings
    warnings.filterwarnings("ignore", message=".*no weight file.*")
    import torch
    t0 = time.time()
    small, big = "facebook/esm2_t30_150M_UR50D", "facebook/esm2_t33_650M_UR50D"
    B, L, Lb, ks = args.batch, args.seq_len, args.big_len, list(args.ks)
    tmp = None
    if args.tiny:
        tmp = tempfile.TemporaryDirectory()
        small = big = _tiny_dir(tmp.name)
        B, L, Lb, ks = 8, 128, 256, [1, 2, 4]
    from oneprot_amd.esm import resolve_config
    out = dict(tool="tools/recompute_ab.py", steps=args.steps, tiny=bool(args.tiny))
    counted = {}
    for label, name, T in (("cfg2", small, B * L), ("big_650m", big, B * Lb)):
        cfg, _ = resolve_config(name)
        d, H, n = cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers
        counted[label] = {("off" if k == 0 else f"k{k}"): activation_bytes(T, d, H, n, k) for k in [0] + ks}
    out["counted"] = counted
    if args.count_only or not torch.cuda.is_available():
        if not args.count_only:
            print("no GPU in this process: the counted bytes alone; every timed side is 'not run'", file=sys.stderr)
        out["timed"] = "not run"
    else:
        out["device"] = torch.cuda.get_device_name(0)
        out["cfg2"] = case_cfg2(small, B, L, ks, args.steps)
        out["big_650m"] = case_big(big, B, Lb, ks[0], max(args.steps // 2, 1))
    out["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
