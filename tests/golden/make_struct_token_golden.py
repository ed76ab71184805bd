"""Writes tests/golden/struct_token_tokenizer.json: the ids of the structure tokenizer of ref src/data/datasets/struct_token_dataset.py:39-41 --
transformers.EsmTokenizer plus `add_tokens` of the 20 foldseek letters and '#' -- on structure strings with and without '#', and of the plain tokenizer
on upper-case sequences.  Run once on the CPU, where transformers is installed:

    python tests/golden/make_struct_token_golden.py

The tokenizer is built from a vocab.txt this script writes (the 33 ESM-2 tokens in id order), the way make_collect_golden.py builds its own; nothing is
downloaded."""
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oneprot_amd.msa_data import MsaBatchConverter  # noqa: E402
from oneprot_amd.token_data import NEW_TOKENS  # noqa: E402


def strings():
    rng = random.Random(1881)
    fold = "".join(NEW_TOKENS[:-1])
    run = lambda n, letters: "".join(rng.choice(letters) for _ in range(n))
    struct = ["dvvlcpp", "d#v#l", "#", "##", "#dpv", "dpv#", run(40, fold), run(40, fold + "#"), run(1021, fold), run(1022, fold), run(1023, fold), run(1500, fold + "#"),
              "", "dzv", "dbjv", "d v", "dVl", "DVL", "d<mask>v", "<mask>#", "d#<pad>"]
    seq = ["MKTAYIAKQR", "LAGVSERTIDPKQNFYMHWCXBUZO", run(1500, "LAGVSERTIDPKQNFYMHWC"), "MKJTA", ""]
    return struct, seq


def main():
    from transformers import EsmTokenizer
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vocab.txt")
        with open(path, "w") as f:
            f.write("\n".join(MsaBatchConverter.all_toks))
        struct_tok, seq_tok = EsmTokenizer(path), EsmTokenizer(path)
        struct_tok.add_tokens(NEW_TOKENS)
        struct, seq = strings()
        out = {"new_tokens": NEW_TOKENS, "new_token_ids": struct_tok.convert_tokens_to_ids(NEW_TOKENS),
               "struct": struct, "struct_ids": [struct_tok(s, truncation=True, max_length=1024)["input_ids"] for s in struct],
               "seq": seq, "seq_ids": [seq_tok(s, truncation=True, max_length=1024)["input_ids"] for s in seq]}
    with open(os.path.join(HERE, "struct_token_tokenizer.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(len(struct), "structure strings,", len(seq), "sequences; new ids", out["new_token_ids"][0], "..", out["new_token_ids"][-1])


if __name__ == "__main__":
    main()
