"""Writes tests/golden/seqsim_collate.json: what the reference's own SequenceSimDataset (src/data/datasets/seqsim_dataset.py there) returns from
`collate_fn` on a small data directory, seeded with `random.seed`.  TEST INFRASTRUCTURE, run by hand where a checkout of the reference is at hand:

    python tests/golden/make_seqsim_golden.py <reference checkout>

The data directory and the local tokenizer directory (vocab.txt of the 33 ESM-2 tokens, tokenizer_config.json naming EsmTokenizer) are written to a
temporary directory; nothing is downloaded and no reference source is copied.  The fixture holds the files' contents, the seeds, the batches' indices and
the two id tensors per batch, plus the number of mutations that failed the assertion and were drawn again (at least one, or this script fails)."""
import importlib.util
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oneprot_amd.msa_data import MsaBatchConverter  # noqa: E402

SEQS = ["MKTAYIAKQRQISFVKSHFSRQ", "LAGVSERTIDPKQNFYMHWC", "MSSHEGGKKKALKQPKKQAKEMDEE"]
ALIGNED = [("MKTAYIAKQRQISFVKSHFSRQ", "MKTAYIAKQR-ISFVKSHF-RQ"), ("LAGVSERTIDPKQNFYMHWC", "LAG-SERTIDPKQNFYMHW-"), ("MSSHEGGKKKALKQPKKQAKEMDEE", "MSSHEGGKKKALKQ-KKQAKEMDEE"),
           ("MKTAYIAKQR", "MKTAYI-KQR"), ("LAGVSERTID", "LAGVSERTID")]


def mutations(rng, seq, n, wrong):
    """n mutation strings of `seq`, `wrong` of them naming a letter that does not stand at their position"""
    out = []
    for k in range(n):
        pos = rng.randrange(len(seq))
        letter = seq[pos] if k >= wrong else next(a for a in "ACDEFGHIKLMNPQRSTVWY" if a != seq[pos])
        out.append(f"{letter}{pos + 1}{rng.choice('ACDEFGHIKLMNPQRSTVWY')}")
    rng.shuffle(out)
    return out


def files():
    rng = random.Random(1881)
    return {"train_seqsim.txt": "\n".join(SEQS) + "\n",
            "clinvar_full_benign_mutations.json": json.dumps({s: mutations(rng, s, 6, 3) for s in SEQS}),
            "clinvar_full_pathogenic_mutations.json": json.dumps({s: mutations(rng, s, 6, 3) for s in SEQS}),
            "train_msa_seqsim.csv": "req_seq,aligned_seq\n" + "".join(f"{a},{b}\n" for a, b in ALIGNED)}


def main():
    ref = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_seqsim_dataset", os.path.join(ref, "src", "data", "datasets", "seqsim_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    content = files()
    with tempfile.TemporaryDirectory() as tmp:
        data_dir, tok_dir = os.path.join(tmp, "data"), os.path.join(tmp, "tok")
        os.makedirs(data_dir)
        os.makedirs(tok_dir)
        for name, text in content.items():
            with open(os.path.join(data_dir, name), "w") as f:
                f.write(text)
        with open(os.path.join(tok_dir, "vocab.txt"), "w") as f:
            f.write("\n".join(MsaBatchConverter.all_toks))
        with open(os.path.join(tok_dir, "tokenizer_config.json"), "w") as f:
            json.dump({"tokenizer_class": "EsmTokenizer"}, f)
        ds = mod.SequenceSimDataset(data_dir, "train", seq_tokenizer=tok_dir, max_length=20)
        redrawn = [0]
        apply = mod.SequenceSimDataset._apply_mutation

        def counting(sequence, mutation):
            try:
                return apply(sequence, mutation)
            except AssertionError:
                redrawn[0] += 1
                raise
        ds._apply_mutation = counting
        batches = []
        for seed, indices in ((0, [0, 1, 2]), (1, [3, 4]), (7, [4, 0, 2, 1])):
            random.seed(seed)
            a, b, modality, raw = ds.collate_fn([ds[i] for i in indices])
            assert modality == "seqsim" and raw is a
            batches.append({"seed": seed, "indices": indices, "input1": a.tolist(), "input2": b.tolist()})
        length = len(ds)
    assert redrawn[0] >= 1, "no mutation failed the assertion: the fixture would not pin the redraw"
    with open(os.path.join(HERE, "seqsim_collate.json"), "w") as f:
        json.dump({"files": content, "max_length": 20, "len": length, "redrawn": redrawn[0], "batches": batches}, f, separators=(",", ":"))
        f.write("\n")
    print(len(batches), "batches,", redrawn[0], "mutations drawn again")


if __name__ == "__main__":
    main()
