"""The evaluation tables of tests/test_eval_cpu.py and tests/test_eval_gpu.py: a CSV in the reference's seven positional columns, a WordPiece vocabulary, and
the structure and pocket files as nested mappings (graphs from graph_data.synthetic_atom_records)."""
import csv
import os

import torch

from oneprot_amd.graph_data import synthetic_atom_records

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the", "protein", "bind", "##ing", "##s", "kinase", "a", ",", ".", "of", "zinc", "finger", "domain", "##like"]
WORDS = ["the", "protein", "binding", "binds", "kinase", "kinases", "a", ",", ".", "of", "zinc", "finger", "domain", "kinaselike", "membrane"]
AA = "LAGVSERTIDPKQNFYMHWC"
FOLD = "pynwrqhgdlvtmfsaeikc"
LETTERS = "ARNDCQEGHILKMFPSTWYV"          # residue type -> letter (graph_data.res1int)


def _pick(gen, letters, k):
    return "".join(letters[int(i)] for i in torch.randint(0, len(letters), (k,), generator=gen))


def graph_entry(record):
    return {"structure": {"0": {"A": {"residues": {"seq1": "".join(LETTERS[a] for a in record[0]).encode()},
                                      "polypeptide": {"atom_amino_id": record[1], "type": record[2], "xyz": record[3]}}}}}


def build_table(tmp_path, seq_lens, text_words, struct_lens, graph_sizes, pocket_sizes, same_text=(), same_seq=(), missing_pocket=(), missing_struct=(),
                missing_seq=(), seed=1881, name="test_all.csv"):
    """Row k: id r<k>, sequence Q<k> (seq_lens[k] letters in the structure file), text of text_words[k] words, a struct_token string of struct_lens[k] letters
    with some '#', struct_graph G<k> and pocket K<k> of the given residue counts.  same_text / same_seq: groups of rows that share the first one's text /
    sequence string (under their own ids); missing_*: rows whose id is absent from its file.  Returns dict(cfg, struct_file, pocket_file, rows, records)."""
    gen = torch.Generator().manual_seed(seed)
    n = len(seq_lens)
    seqs = [_pick(gen, AA, k) for k in seq_lens]
    texts = [" ".join(WORDS[int(j)] for j in torch.randint(0, len(WORDS), (k,), generator=gen)) for k in text_words]
    structs = [_pick(gen, FOLD + "#", k) for k in struct_lens]
    structs = [s[:1] + "#" + s[2:] if len(s) >= 2 else s for s in structs]                   # every string of two letters or more holds a '#'
    for group in same_text:
        for k in group[1:]:
            texts[k] = texts[group[0]]
    for group in same_seq:
        for k in group[1:]:
            seqs[k] = seqs[group[0]]
    records = {"struct_graph": [synthetic_atom_records(k, gen) for k in graph_sizes], "pocket": [synthetic_atom_records(k, gen) for k in pocket_sizes]}
    struct_file, pocket_file = {}, {}
    for k in range(n):
        if k not in missing_seq:
            struct_file[f"Q{k}"] = {"structure": {"0": {"A": {"residues": {"seq1": seqs[k].encode()}}}}}
        if k not in missing_struct:
            struct_file[f"G{k}"] = graph_entry(records["struct_graph"][k])
        if k not in missing_pocket:
            pocket_file[f"K{k}"] = graph_entry(records["pocket"][k])
    rows = [[f"r{k}", f"msa/{k}.a3m", texts[k], structs[k], f"G{k}", f"Q{k}", f"K{k}"] for k in range(n)]
    path = os.path.join(str(tmp_path), name)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name", "msa", "function", "foldseek", "structure", "sequence", "pocket"])
        w.writerows(rows)
    with open(os.path.join(str(tmp_path), "vocab.txt"), "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    cfg = {"dataset": {"csv_file_path": path, "data_dir": str(tmp_path), "max_sequence_length": 1024, "text_max_length": 512, "text_tokenizer": str(tmp_path),
                       "seq_tokenizer": "facebook/esm2_t33_650M_UR50D", "remove_hash": True, "msa_model_name_or_path": "unused.pt", "msa_depth": 50, "max_length": 1024},
           "dataloader": {"batch_size": 50, "shuffle": False, "num_workers": 4}, "output": {"csv_path": os.path.join(str(tmp_path), "out", "retrieval_metrics.csv")}}
    kept = [k for k in range(n) if k not in missing_pocket and k not in missing_struct and k not in missing_seq]
    return dict(cfg=cfg, struct_file=struct_file, pocket_file=pocket_file, rows=rows, records=records, seqs=seqs, texts=texts, structs=structs, kept=kept)
