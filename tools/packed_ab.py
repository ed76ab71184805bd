"""Padded against packed batches (ESM towers, BERT text tower), in one process, on identical data (oneprot_amd.packing; DESIGN.md section 6, "Packed batches").

cfg-2 shapes: ESM-2-150M x2 (sequence tower frozen, struct-token tower trainable), L = 512, 256 pairs per sub-step.  The padded and the packed
form of the SAME batch (SyntheticPairs(ragged=True) and SyntheticPairs(packed=True), one seed) alternate sub-step by sub-step, so clock and
power drift fall on both alike; each side is timed between HIP events around its own sub-steps.

  ragged   lengths uniform in [L/4, L] (what shuffled real data looks like; the reference pads each batch to its longest row)
  full     every row L tokens long: packing saves nothing, this prices its overhead
  anchor   ESM-2-650M attention1d tower (the cfg-5 anchor), forward only, ragged rows
  text     cfg-4 shapes: ESM-2-150M (L = 512, frozen) <-> BERT-base text tower (T = 256, frozen, cls pooling + mlp head, HF's train-mode dropout on as in
           the reference), both sides packed (SyntheticPairs(packed=True, packed_text=True)), ragged and full-length rows; --text-only runs just these
           two and writes them alone (profiles/packed_ab_text.json)

Per case: pairs/s and real tokens/s of both layouts, the measured speed-up, and the FLOP ratio padded / packed computed from the lengths (GEMM rows;
attention, whose per-sequence cost goes with the square of the length).  PACKED_AB_PROFILE=1 runs only the ragged cfg-2 case, a few steps, for
`rocprofv3 --kernel-trace --stats -- python tools/packed_ab.py`; `tools/rocpd_stats.py` turns its database into the per-kernel table that
profiles/packed_ab_kernels.txt compares (the varlen attention kernels' time per FLOP against the padded ones').

usage: python tools/packed_ab.py [--steps 6] [--out profiles/packed_ab.json]
       python tools/packed_ab.py --text-only [--out profiles/packed_ab_text.json]
"""
import argparse
import functools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flops_ratio(lengths, L, d, f, n_layers):
    """padded / packed FLOPs of one tower's forward from the lengths: GEMM rows (8 d^2 + 4 d f per row and layer) and attention (4 d per query-key pair)"""
    B = len(lengths)
    T_pad = -(-sum(lengths) // 256) * 256
    gemm_pad, gemm_pk = B * L, T_pad
    att_pad, att_pk = B * L * L, sum(n * n for n in lengths)
    per_row, per_pair = 8 * d * d + 4 * d * f, 4 * d
    tot_pad = n_layers * (gemm_pad * per_row + att_pad * per_pair)
    tot_pk = n_layers * (gemm_pk * per_row + att_pk * per_pair)
    return dict(gemm_rows=round(gemm_pad / gemm_pk, 3), attention=round(att_pad / att_pk, 3), total=round(tot_pad / tot_pk, 3))


def timed_alternating(fn_a, fn_b, steps, warm=2):
    """alternate a, b sub-steps; seconds of each between HIP events on the current stream"""
    import torch
    for _ in range(warm):
        fn_a(); fn_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(steps):
        for fn, acc in ((fn_a, ta), (fn_b, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e-3)
    med = lambda v: sorted(v)[len(v) // 2]
    return med(ta), med(tb), ta, tb


def build_pair(dev):
    import torch
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.struct_token_encoder import StructTokenEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(1881)
    seq = SequenceEncoder("facebook/esm2_t30_150M_UR50D", output_dim=1024, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=True)
    st = StructTokenEncoder("facebook/esm2_t30_150M_UR50D", output_dim=1024, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    m = OneProtLitModule(components={"sequence": seq, "struct_token": st}, optimizer=functools.partial(FusedAdam, lr=1e-3, weight_decay=0.0), loss_fn="CLIP",
                         use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(dev)
    m.train()
    return m


def case_substep(module, B, L, ragged, steps, seed=1881):
    import torch
    from oneprot_amd.data import SyntheticPairs
    rag = next(iter(SyntheticPairs("struct_token", B, L, seed=seed, ragged=ragged)))
    pk = next(iter(SyntheticPairs("struct_token", B, L, seed=seed, packed=True))) if ragged else None
    if not ragged:      # full-length rows in packed form
        from oneprot_amd.packing import PackedTokens
        pk = (PackedTokens.from_padded(rag[0]), PackedTokens.from_padded(rag[1]), "struct_token", None)
    dev = torch.device("cuda")
    b_pad = {"struct_token": (rag[0].to(dev), rag[1].to(dev), "struct_token", None)}
    b_pk = {"struct_token": (pk[0].to(dev), pk[1].to(dev), "struct_token", None)}
    t_pad, t_pk, ta, tb = timed_alternating(lambda: module.training_step(b_pad, 0), lambda: module.training_step(b_pk, 0), steps)
    lens = [int(n) for n in (rag[0] != 1).sum(1)] + [int(n) for n in (rag[1] != 1).sum(1)]
    tr = module.network["struct_token"].transformer
    real = sum(lens)
    return dict(pairs=B, L=L, real_tokens=real, padded_tokens=2 * B * L, packed_T_pad=[pk[0].T_pad, pk[1].T_pad],
                padded=dict(s=round(t_pad, 5), pairs_per_s=round(B / t_pad, 1), real_tokens_per_s=round(real / t_pad)),
                packed=dict(s=round(t_pk, 5), pairs_per_s=round(B / t_pk, 1), real_tokens_per_s=round(real / t_pk)),
                speedup=round(t_pad / t_pk, 3), flop_ratio_padded_over_packed=flops_ratio(lens[:B], L, tr.d, tr.f, tr.n_layers),
                steps_s=dict(padded=[round(x, 5) for x in ta], packed=[round(x, 5) for x in tb]))


def build_text_pair(dev):
    import torch
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.text_encoder import TextEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(1881)
    seq = SequenceEncoder("facebook/esm2_t30_150M_UR50D", output_dim=1024, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=True)
    txt = TextEncoder("microsoft/BiomedNLP-BiomedBERT-base-uncased-abstract-fulltext", output_dim=1024, pooling_type="cls", proj_type="mlp",
                      use_logit_scale=True, learnable_logit_scale=False, frozen=True, use_lora=False)
    m = OneProtLitModule(components={"sequence": seq, "text": txt}, optimizer=functools.partial(FusedAdam, lr=1e-3, weight_decay=0.0), loss_fn="CLIP",
                         use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(dev)
    m.train()
    return m


def case_text(module, B, L, T, ragged, steps, seed=1881):
    """one seq <-> text sub-step, padded against both sides packed"""
    import torch
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.packing import PackedTokens
    rag = next(iter(SyntheticPairs("text", B, L, mod_len=T, seed=seed, ragged=ragged)))
    if ragged:
        pk = next(iter(SyntheticPairs("text", B, L, mod_len=T, seed=seed, packed=True, packed_text=True)))
    else:               # full-length rows in packed form
        pk = (PackedTokens.from_padded(rag[0], pad_id=1), PackedTokens.from_padded(rag[1], pad_id=0), "text", None)
    dev = torch.device("cuda")
    b_pad = {"text": (rag[0].to(dev), rag[1].to(dev), "text", None)}
    b_pk = {"text": (pk[0].to(dev), pk[1].to(dev), "text", None)}
    t_pad, t_pk, ta, tb = timed_alternating(lambda: module.training_step(b_pad, 0), lambda: module.training_step(b_pk, 0), steps)
    lens_s, lens_t = [int(n) for n in (rag[0] != 1).sum(1)], [int(n) for n in (rag[1] != 0).sum(1)]
    trs, trt = module.network["sequence"].transformer, module.network["text"].transformer
    real = sum(lens_s) + sum(lens_t)
    spread = lambda v: round(max(v) - min(v), 5)
    return dict(pairs=B, L=L, T=T, real_tokens=real, padded_tokens=B * (L + T), packed_T_pad=[pk[0].T_pad, pk[1].T_pad],
                padded=dict(s=round(t_pad, 5), pairs_per_s=round(B / t_pad, 1), real_tokens_per_s=round(real / t_pad), spread_s=spread(ta)),
                packed=dict(s=round(t_pk, 5), pairs_per_s=round(B / t_pk, 1), real_tokens_per_s=round(real / t_pk), spread_s=spread(tb)),
                speedup=round(t_pad / t_pk, 3),
                flop_ratio_padded_over_packed=dict(sequence=flops_ratio(lens_s, L, trs.d, trs.f, trs.n_layers), text=flops_ratio(lens_t, T, trt.d, trt.f, trt.n_layers)),
                steps_s=dict(padded=[round(x, 5) for x in ta], packed=[round(x, 5) for x in tb]))


def case_anchor(B, L, steps):
    import torch
    from oneprot_amd.data import SyntheticPairs
    from src.models.components.sequence_encoder import SequenceEncoder
    torch.manual_seed(1881)
    dev = torch.device("cuda")
    enc = SequenceEncoder("facebook/esm2_t33_650M_UR50D", output_dim=1024, pooling_type="attention1d", proj_type="linear", use_lora=False, frozen=True).to(dev).eval()
    rag = next(iter(SyntheticPairs("sequence", B, L, seed=7, ragged=True)))[0].to(dev)
    pk = next(iter(SyntheticPairs("sequence", B, L, seed=7, packed=True)))[0].to(dev)
    with torch.no_grad():
        t_pad, t_pk, ta, tb = timed_alternating(lambda: enc(rag), lambda: enc(pk), steps)
    lens = [int(n) for n in (rag != 1).sum(1)]
    tr = enc.transformer
    real = sum(lens)
    del enc
    torch.cuda.empty_cache()
    return dict(sequences=B, L=L, real_tokens=real, packed_T_pad=pk.T_pad,
                padded=dict(s=round(t_pad, 5), seq_per_s=round(B / t_pad, 1), real_tokens_per_s=round(real / t_pad)),
                packed=dict(s=round(t_pk, 5), seq_per_s=round(B / t_pk, 1), real_tokens_per_s=round(real / t_pk)),
                speedup=round(t_pad / t_pk, 3), flop_ratio_padded_over_packed=flops_ratio(lens, L, tr.d, tr.f, tr.n_layers))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--anchor-batch", type=int, default=64)
    ap.add_argument("--text-len", type=int, default=256)
    ap.add_argument("--text-only", action="store_true", help="only the cfg-4 text cases (both sides packed)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ["ONEPROT_ALLOW_RANDOM_INIT"] = "1"
    import warnings
    warnings.filterwarnings("ignore", message=".*no weight file.*")
    import torch
    dev = torch.device("cuda")
    t0 = time.time()
    out = dict(tool="tools/packed_ab.py", device=torch.cuda.get_device_name(0), steps=args.steps)

    def text_cases():
        module = build_text_pair(dev)
        out["ragged_cfg4_text"] = case_text(module, args.batch, args.seq_len, args.text_len, True, args.steps)
        out["full_cfg4_text"] = case_text(module, args.batch, args.seq_len, args.text_len, False, args.steps)
        del module
        torch.cuda.empty_cache()

    if args.text_only:
        text_cases()
        out["wall_s"] = round(time.time() - t0, 1)
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    module = build_pair(dev)
    if os.environ.get("PACKED_AB_PROFILE") == "1":
        out["ragged_cfg2"] = case_substep(module, args.batch, args.seq_len, True, min(args.steps, 3))
    else:
        out["ragged_cfg2"] = case_substep(module, args.batch, args.seq_len, True, args.steps)
        out["full_cfg2"] = case_substep(module, args.batch, args.seq_len, False, args.steps)
        del module
        torch.cuda.empty_cache()
        out["anchor_650m_attention1d_fwd"] = case_anchor(args.anchor_batch, args.seq_len, args.steps)
        text_cases()
    out["wall_s"] = round(time.time() - t0, 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
