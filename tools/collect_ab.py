"""Embedding collection: the reference's batching against the token-budget plan, in one process, on identical splits (oneprot_amd/collect.py; DESIGN.md
section 6, "Embedding collection").

  arm A   the reference's batching on our kernels: file order, 32 rows per batch, each batch padded to its longest row (ref collect_embeddings.py:81-87,
          222-229), every row embedded -- for ppi both columns of every pair
  arm B   collect.embed_sequences: unique sequences in canonical order, packed into token budgets of 8 192, 32 768 and 131 072

Both arms compute the esm2 baseline (masked mean of the last hidden state) on the same randomly initialised tower.  Arm A's ids are tokenised before its
clock starts; arm B's clock includes its tokenizer and plan.  The arms alternate pass by pass, so clock and power drift fall on all alike.

  synthetic   4 096 rows, token counts drawn as SyntheticPairs(..., ragged=True) draws them at L = 1 024 (uniform in [256, 1 024])
  ppi         1 024 pairs over 410 proteins of such lengths: each protein occurs in about 5 pairs

at the 150M shape (30 x 640) and the 650M shape (33 x 1 280).  Per arm: sequences/s (rows of the split), real tokens/s, and the share of the wall time the
device sat idle between batches (from timing events around every batch).  `choice` is the smallest budget whose throughput is within 3 % of the best arm-B
throughput, per shape and split; `default_max_tokens` the largest of those choices.

usage: python tools/collect_ab.py [--reps 2] [--out profiles/collect_embed.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUDGETS = (8192, 32768, 131072)
SHAPES = {"150m": "facebook/esm2_t30_150M_UR50D", "650m": "facebook/esm2_t33_650M_UR50D"}


def synthetic_sequences(n, seed, L=1024):
    """n letter strings whose token counts (<cls> and <eos> included) are SyntheticPairs' ragged lengths at L"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(L // 4, 2), L + 1, (n,), generator=gen)
    letters = "LAGVSERTIDPKQNFYMHWC"
    body = torch.randint(0, 20, (int(lens.sum()),), generator=gen).tolist()
    out, at = [], 0
    for m in lens.tolist():
        out.append("".join(letters[i] for i in body[at:at + m - 2]))
        at += m - 2
    return out


def ppi_columns(pairs, proteins, seed):
    import torch
    prot = synthetic_sequences(proteins, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    a, b = torch.randint(0, proteins, (pairs,), generator=gen).tolist(), torch.randint(0, proteins, (pairs,), generator=gen).tolist()
    return [prot[i] for i in a], [prot[i] for i in b]


def idle_share(events, wall_s):
    """device time between the end of a batch and the start of the next, over the wall time"""
    gaps = sum(max(0.0, e0[1].elapsed_time(e1[0])) for e0, e1 in zip(events[:-1], events[1:]))
    return gaps * 1e-3 / wall_s


def arm_a(tr, rows_ids, dev, batch=32):
    """file order, 32 rows, padded to the longest; rows_ids: per-row int64 arrays"""
    import torch
    from oneprot_amd import layout
    from oneprot_amd.collect import _MeanMode
    out = torch.empty(len(rows_ids), tr.d, device=dev)
    events = []
    with torch.no_grad():
        for lo in range(0, len(rows_ids), batch):
            rows = rows_ids[lo:lo + batch]
            L = max(r.size for r in rows)
            ids = torch.ones(len(rows), L, dtype=torch.int64, pin_memory=True)
            for b, r in enumerate(rows):
                ids[b, :r.size] = torch.from_numpy(r)
            ids = ids.to(dev, non_blocking=True)
            events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            events[-1][0].record()
            x, _ = tr.run_layers(ids, save=False)
            out[lo:lo + len(rows)] = layout.of(tr, ids).pool_fwd(tr, x, _MeanMode, False)[0]
            events[-1][1].record()
    return out, events


def run_split(tr, name, sequences, reps, dev):
    import torch
    from oneprot_amd import collect as C
    tok = C.EsmSequenceTokenizer()
    flat, off = tok.encode_all(sequences)
    rows_ids = [flat[off[i]:off[i + 1]] for i in range(len(sequences))]
    tokens = int(off[-1])
    arms = {"A_ref_batching_32": lambda: arm_a(tr, rows_ids, dev)}
    for budget in BUDGETS:
        def arm_b(budget=budget):
            events = []
            return C.embed_sequences(tr, sequences, "esm2", max_tokens=budget, max_seqs=budget, timings=events), events
        arms[f"B_max_tokens_{budget}"] = arm_b
    warm = sequences[:256]
    wf, wo = tok.encode_all(warm)
    arm_a(tr, [wf[wo[i]:wo[i + 1]] for i in range(len(warm))], dev)
    for budget in BUDGETS:
        C.embed_sequences(tr, warm, "esm2", max_tokens=budget, max_seqs=budget)
    torch.cuda.synchronize()
    res = {k: dict(s=[], idle_share=[]) for k in arms}
    ref = None
    for _ in range(reps):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, events = fn()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            res[k]["s"].append(round(wall, 4))
            res[k]["idle_share"].append(round(idle_share(events, wall), 4))
            res[k]["batches"] = len(events)
            if ref is None:
                ref = out
            else:           # the arms embed the same rows (bf16 towers, two layouts: close, not equal)
                res[k]["min_row_cosine_vs_A"] = round(float(torch.nn.functional.cosine_similarity(out, ref, dim=-1).min()), 6)
    plan = C.plan_sequences(sequences, 1024, BUDGETS[0], BUDGETS[0])
    summary = dict(rows=len(sequences), unique=len(plan["uniq"]), real_tokens=tokens, unique_tokens=int(plan["off"][-1]),
                   padded_tokens_A=sum(max(r.size for r in rows_ids[lo:lo + 32]) * len(rows_ids[lo:lo + 32]) for lo in range(0, len(rows_ids), 32)), arms={})
    for k, v in res.items():
        s = sorted(v["s"])[len(v["s"]) // 2]
        summary["arms"][k] = dict(s=s, seq_per_s=round(len(sequences) / s, 1), real_tokens_per_s=round(tokens / s), idle_share=sorted(v["idle_share"])[len(v["s"]) // 2],
                                  batches=v["batches"], passes_s=v["s"], **({"min_row_cosine_vs_A": v["min_row_cosine_vs_A"]} if "min_row_cosine_vs_A" in v else {}))
    b = {budget: summary["arms"][f"B_max_tokens_{budget}"]["seq_per_s"] for budget in BUDGETS}
    best = max(b.values())
    summary["choice"] = min(budget for budget, v in b.items() if v >= 0.97 * best)
    summary["B_over_A"] = round(summary["arms"][f"B_max_tokens_{summary['choice']}"]["seq_per_s"] / summary["arms"]["A_ref_batching_32"]["seq_per_s"], 3)
    print(name, json.dumps(summary), flush=True)
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--proteins", type=int, default=410)
    ap.add_argument("--shapes", default="150m,650m")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["ONEPROT_ALLOW_RANDOM_INIT"] = "1"
    import warnings
    warnings.filterwarnings("ignore", message=".*no weight file.*")
    import torch
    from oneprot_amd.esm import EsmTransformer
    dev = torch.device("cuda")
    t0 = time.time()
    out = dict(tool="tools/collect_ab.py", device=torch.cuda.get_device_name(0), reps=args.reps, budgets=list(BUDGETS), shapes={})
    synthetic = synthetic_sequences(args.rows, 1881)
    col1, col2 = ppi_columns(args.pairs, args.proteins, 7)
    for shape in args.shapes.split(","):
        torch.manual_seed(1881)
        tr = EsmTransformer.from_pretrained(SHAPES[shape], add_pooling_layer=False).to(dev).eval()
        out["shapes"][shape] = dict(model=SHAPES[shape], synthetic=run_split(tr, f"{shape}/synthetic", synthetic, args.reps, dev),
                                    ppi=run_split(tr, f"{shape}/ppi", col1 + col2, args.reps, dev))
        del tr
        torch.cuda.empty_cache()
    out["default_max_tokens"] = max(v[s]["choice"] for v in out["shapes"].values() for s in ("synthetic", "ppi"))
    out["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
