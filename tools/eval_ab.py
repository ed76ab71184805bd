#!/usr/bin/env python3
"""The evaluation script's two choices, measured -> profiles/eval_embed.json.

One process, wall clock around device-synchronised calls (the host side -- tokenising, reading records, staging -- is part of what is compared); every variant is
warmed up once, then the variants alternate A B A B for `--reps` rounds.
  embed_A / embed_B   evaluate.embed_modalities (the whole-dataset pass) against evaluate.encode_inputs over collate_fn batches of 50 in file order (the
                      reference's loop), all five modalities, dataset.device = the GPU in both.  Table A: 4 096 rows, sequences of 50 .. 1 000 letters, texts of
                      10 .. 400 words, struct_token strings as long as the sequences, 100-residue pockets and structures.  Table B: table A with every text
                      shared by about 8 rows.  Towers: random-init ESM 6 x 320 (sequence, struct_token), BERT 2 x 256, ProNet 2 blocks x 128, output_dim 256.
                      LOOKED FOR: the whole-dataset median is no larger than the loop's, on either table.
  rank_ties           retrieval.pair_ranks(ties=True) (oneprot_sim_rank_ties) against pair_ranks (oneprot_sim_rank) at N = 16 384, D = 1 024, and the same pair
                      at D = 32, where the tile's multiply is 1/32 of the work and the difference of the two forms is what the extra compare + ballot costs.
                      LOOKED FOR: ties median <= plain median + max(spread of either) + that cost.
No ratio is fixed in advance; a miss is recorded as `passed: false` next to the numbers.
usage: eval_ab.py [--only embed_A,embed_B,rank_ties] [--reps 3] [--rows 4096] [--out profiles/eval_embed.json] [--small]"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(200)] + [f"##s{i}" for i in range(50)]
LETTERS = "ARNDCQEGHILKMFPSTWYV"


def stats(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "spread_s": max(xs) - min(xs), "reps": len(xs)}


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def build_model(tmp):
    import torch
    from oneprot_amd.encoders import SequenceEncoder, StructEncoder, StructTokenEncoder, TextEncoder
    from oneprot_amd.module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    from oneprot_amd.pronet import ProNet
    import functools
    esm, bert = os.path.join(tmp, "esm"), os.path.join(tmp, "bert")
    for path, cfg in ((esm, dict(model_type="esm", vocab_size=33, hidden_size=320, num_hidden_layers=6, num_attention_heads=20, intermediate_size=1280)),
                      (bert, dict(model_type="bert", vocab_size=len(VOCAB), hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                                  max_position_embeddings=512, pad_token_id=0))):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(cfg, f)
    torch.manual_seed(0)
    graph = lambda: StructEncoder(ProNet(level="backbone", num_blocks=2, hidden_channels=128, out_channels=256), output_dim=256, proj_type="linear", use_logit_scale=True)
    comps = {"sequence": SequenceEncoder(esm, output_dim=256, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=True),
             "struct_token": StructTokenEncoder(esm, output_dim=256, pooling_type="mean", proj_type="linear", use_logit_scale=True),
             "text": TextEncoder(bert, output_dim=256, pooling_type="mean", proj_type="linear", use_logit_scale=True, frozen=True, use_lora=False),
             "struct_graph": graph(), "pocket": graph()}
    return OneProtLitModule(components=comps, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP").cuda().eval()


def build_tables(tmp, rows, small):
    """(cfg of table A, cfg of table B, structure file, pocket file): the files are nested mappings; 64 distinct 100-residue graphs serve all rows"""
    import torch
    from oneprot_amd.graph_data import synthetic_atom_records
    gen = torch.Generator().manual_seed(5)
    lo, hi = (20, 200) if small else (50, 1000)
    pick = lambda letters, n: "".join(letters[int(i)] for i in torch.randint(0, len(letters), (n,), generator=gen))
    words = [v for v in VOCAB[5:] if not v.startswith("##")]
    struct_file, pocket_file = {}, {}
    entry = lambda r: {"structure": {"0": {"A": {"residues": {"seq1": "".join(LETTERS[a] for a in r[0]).encode()},
                                                 "polypeptide": {"atom_amino_id": r[1], "type": r[2], "xyz": r[3]}}}}}
    for g in range(64):
        struct_file[f"G{g}"] = entry(synthetic_atom_records(100, gen))
        pocket_file[f"K{g}"] = entry(synthetic_atom_records(100, gen))
    table, texts = [], []
    for k in range(rows):
        n = int(torch.randint(lo, hi + 1, (1,), generator=gen))
        struct_file[f"Q{k}"] = {"structure": {"0": {"A": {"residues": {"seq1": pick("LAGVSERTIDPKQNFYMHWC", n).encode()}}}}}
        texts.append(" ".join(words[int(j)] for j in torch.randint(0, len(words), (int(torch.randint(10, 401, (1,), generator=gen)),), generator=gen)))
        table.append([f"r{k}", "", None, pick("pynwrqhgdlvtmfsaeikc", n), f"G{k % 64}", f"Q{k}", f"K{(7 * k) % 64}"])
    with open(os.path.join(tmp, "vocab.txt"), "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    cfgs = []
    for name, text_of in (("A", lambda k: texts[k]), ("B", lambda k: texts[k // 8])):
        path = os.path.join(tmp, f"table_{name}.csv")
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["ids", "msa_files", "text", "struct_token", "struct_graph", "sequence", "pocket"])
            w.writerows(r[:2] + [text_of(k)] + r[3:] for k, r in enumerate(table))
        cfgs.append({"dataset": {"csv_file_path": path, "data_dir": tmp, "max_sequence_length": 1024, "text_max_length": 512, "text_tokenizer": tmp,
                                 "seq_tokenizer": "facebook/esm2_t33_650M_UR50D", "remove_hash": True}})
    return cfgs[0], cfgs[1], struct_file, pocket_file


def embed_ab(cfg, struct_file, pocket_file, model, reps):
    import torch
    from oneprot_amd import evaluate as E
    ds = E.CombinedDataset(cfg, struct_file=struct_file, pocket_file=pocket_file)
    ds.device = next(model.parameters()).device

    def loop():
        parts = [E.encode_inputs(model, ds.collate_fn(ds.data[lo:lo + 50])) for lo in range(0, len(ds), 50)]
        return {m: torch.cat([p[m] for p in parts]) for m in E.MODALITIES}
    variants = {"whole_dataset": lambda: E.embed_modalities(model, ds), "loop_of_50": loop}
    first = {k: wall(f) for k, f in variants.items()}                     # warm-up, and the two results
    cos = {m: float(torch.nn.functional.cosine_similarity(first["whole_dataset"][1][m], first["loop_of_50"][1][m], dim=-1).min()) for m in E.MODALITIES}
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            times[k].append(wall(f)[0])
    out = {"rows": len(ds), "distinct_texts": len({r["text"] for r in ds.data}), "warmup_s": {k: v[0] for k, v in first.items()}, "min_row_cosine": cos,
           **{k: stats(v) for k, v in times.items()}}
    out["looked_for"] = {"rule": "whole_dataset median <= loop_of_50 median", "passed": bool(out["whole_dataset"]["median_s"] <= out["loop_of_50"]["median_s"])}
    return out


def rank_ties(reps, small):
    import torch
    from oneprot_amd import retrieval
    N = 2048 if small else 16384
    out = {"N": N}
    for D in (1024, 32):
        g = torch.Generator(device="cuda").manual_seed(D)
        s = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=-1)
        m = torch.nn.functional.normalize(s + 0.6 * torch.randn(N, D, device="cuda", generator=g), dim=-1)
        m[1::8], s[1::8] = m[0::8], s[0::8]                              # an eighth of the pairs repeated: exact ties, as an evaluation table has them
        variants = {"plain": lambda: retrieval.pair_ranks(s, m), "ties": lambda: retrieval.pair_ranks(s, m, ties=True)}
        res = {k: f() for k, f in variants.items()}
        torch.cuda.synchronize()
        equal = bool(torch.equal(res["plain"][0], res["ties"][0]) and torch.equal(res["plain"][1], res["ties"][1]))
        tied_rows = int((res["ties"][2] > 0).sum())
        times = {k: [] for k in variants}
        for _ in range(max(reps, 5)):
            for k, f in variants.items():
                times[k].append(wall(f)[0])
        out[f"D{D}"] = {"ranks_equal": equal, "rows_with_ties": tied_rows, **{k: stats(v) for k, v in times.items()}}
    big, thin = out["D1024"], out["D32"]
    cost = max(0.0, thin["ties"]["median_s"] - thin["plain"]["median_s"])
    allowed = max(big["plain"]["spread_s"], big["ties"]["spread_s"]) + cost
    out["looked_for"] = {"rule": "D1024 ties median <= plain median + max(spread of either) + (D32 ties median - D32 plain median)", "compare_ballot_cost_s": cost,
                         "allowed_s": allowed, "excess_s": big["ties"]["median_s"] - big["plain"]["median_s"],
                         "passed": bool(big["ties"]["median_s"] <= big["plain"]["median_s"] + allowed and big["ranks_equal"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="embed_A,embed_B,rank_ties")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_embed.json"))
    ap.add_argument("--small", action="store_true", help="small shapes: a dry run of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("ONEPROT_ALLOW_RANDOM_INIT", "1")):
        os.environ.setdefault(k, v)
    only = a.only.split(",")
    doc = {"device": torch.cuda.get_device_name(0), "small_shapes": a.small}
    if "embed_A" in only or "embed_B" in only:
        with tempfile.TemporaryDirectory() as tmp:
            model = build_model(tmp)
            cfg_a, cfg_b, struct_file, pocket_file = build_tables(tmp, 256 if a.small else a.rows, a.small)
            for name, cfg in (("embed_A", cfg_a), ("embed_B", cfg_b)):
                if name in only:
                    doc[name] = embed_ab(cfg, struct_file, pocket_file, model, a.reps)
                    print(name, json.dumps(doc[name]), flush=True)
            del model
            torch.cuda.empty_cache()
    if "rank_ties" in only:
        doc["rank_ties"] = rank_ties(a.reps, a.small)
        print("rank_ties", json.dumps(doc["rank_ties"]), flush=True)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
