"""Writes tests/golden/esm_tokenizer.json: the ids transformers.EsmTokenizer gives about 40 strings, with truncation=True and max_length=1024 as the
reference's collect_embeddings.py calls it.  Run once on the CPU, where transformers is installed:

    python tests/golden/make_collect_golden.py

The tokenizer is built from a vocab.txt this script writes itself (the 33 ESM-2 tokens, one per line, in id order); nothing is downloaded.  The fixture
holds the strings and the ids and nothing else; tests/test_collect_cpu.py checks that every rule below is represented in it."""
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oneprot_amd.msa_data import LETTERS, MsaBatchConverter  # noqa: E402


def strings():
    rng = random.Random(1881)
    aa = "LAGVSERTIDPKQNFYMHWC"
    long = lambda n: "".join(rng.choice(aa) for _ in range(n))
    return [
        LETTERS,                                    # all 25 letters plus . and -
        "MKTAYIAKQR",
        "MKJTA", "MKJJTA", "MK*J TA", "JMKTA", "MKTAJ", "J", "JJJ", "*MK*", "MK1234TA", "M_K",      # out-of-vocabulary characters: single, runs, both ends
        "mkta", "MKta", "mKtA", "Mk Ta",            # lower case
        "M K", " MK ", "M\tK", "M \t K", "MK\n", "\tMKTA\t", "MK J J TA", " ", "J J",       # white space
        "MK<mask>TA", "<mask>", "<mask><mask>", "MK <mask> TA", "<cls>MK<eos>", "MK<pad>", "MK<unk>TA", "<null_1>M", "<mas", "MK<maskTA", "<<mask>>", "<MASK>",
        "a<mask>b", "M<K>T",
        "",                                         # the empty string
        long(1021), long(1022), long(1023), long(1500),
        "J" + long(1500), long(1021) + "JJ", long(1019) + " J J J J",
    ]


def main():
    from transformers import EsmTokenizer
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vocab.txt")
        with open(path, "w") as f:
            f.write("\n".join(MsaBatchConverter.all_toks))
        tok = EsmTokenizer(path)
        ss = strings()
        ids = [tok(s, truncation=True, max_length=1024)["input_ids"] for s in ss]
    with open(os.path.join(HERE, "esm_tokenizer.json"), "w") as f:
        json.dump({"strings": ss, "ids": ids}, f, separators=(",", ":"))
        f.write("\n")
    print(len(ss), "strings,", sum(map(len, ids)), "ids")


if __name__ == "__main__":
    main()
