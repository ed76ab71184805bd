"""Writes tests/golden/wordpiece.json: the ids `tokenizers.BertWordPieceTokenizer(vocab, lowercase=True)` -- and once lowercase=False -- gives the texts
below under truncation, on a vocabulary this script writes itself.  That tokenizer is what the reference's `AutoTokenizer.from_pretrained(text_tokenizer)`
resolves to for a BERT checkpoint (ref src/data/datasets/text_dataset.py:25,51).  Run once on the CPU, where `tokenizers` is installed:

    python tests/golden/make_wordpiece_golden.py

Nothing is downloaded.  (transformers' BERT class on a bare vocab file is not used: under transformers 5.15 it returned [UNK] for every word.)  The
fixture holds the vocabulary, the texts with their max_length and lowercase flag, and the ids; tests/test_text_data_cpu.py checks that every case the
list below is meant to hold is really in it, and that no text spells out a special token."""
import json
import os
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]",
         "the", "protein", "bind", "##ing", "##s", "kinase", "un", "##affect", "##able", "##ed", "a", "##a", "cafe", "resume", "i", "x", "ab", "##c",
         "σ", "##α", "##σ", "α", "蛋", "白", "ᄀ", "##ᅡ", "##ᆨ", "##\U0001f600", "\U00020000", "##\u0903",
         "!", ".", ",", "-", "(", ")", "#", "+", "$", "<", "—", "¡",
         "The", "İ", "Σ", "café", "각", "Protein", "##\u0301"]

SENTENCE = "the protein binding kinases"            # the, protein, bind, ##ing, kinase, ##s: 6 pieces


def cases():
    """(text, max_length, lowercase)"""
    low = [
        ("", 512), (" \t\n    ", 512),                         # empty, all white space
        ("ing", 512), ("the ing s", 512),                                 # only a ## piece
        ("bindingq", 512), ("unaffectableq the", 512), ("unaffectable", 512), ("unaffected binds", 512),      # the last position fails
        ("a" * 100, 512), ("a" * 101, 512), ("the " + "a" * 100 + " " + "a" * 101 + " the", 512), ("a" * 300, 512),
        ("!!!...", 512), ("(the)-,#protein.", 512), ("a+a$a", 512), ("the—protein ¡the!", 512), ("a\u226ea", 512),
        ("x蛋白ab", 512), ("蛋", 512), ("the一protein", 512), ("\U00020000x", 512), ("x\U0001f600", 512), ("x\U0001f600 \U0001f600", 512),
        ("각", 512), ("the 각 protein", 512), ("가", 512),
        ("café résumé", 512), ("cafe\u0301", 512), ("a\u0903", 512), ("a\u20dd", 512), ("CAFÉ The PROTEIN", 512),
        ("İ", 512), ("ΣΑΣ", 512), ("σας", 512),
        ("bind\x0bing bind\x0cing bind\u0085ing bind\u00ading bind\u200bing bind\x00ing bind\ufffding", 512), ("binding", 512), ("bind\u0378ing", 512),
        ("the protein bind\tthe\nprotein\rbind\u3000the", 512),
        (SENTENCE, 512), (SENTENCE, 9), (SENTENCE, 8), (SENTENCE, 7), (SENTENCE, 6), (SENTENCE, 5), (SENTENCE, 2), (SENTENCE, 3), ("", 2), ("", 3), ("ing", 3),
        ("a" * 100, 50), ("a" * 101 + " the", 3),
    ]
    cased = [("The protein", 512), ("the Protein PROTEIN", 512), ("İ Σ café cafe\u0301", 512), ("각", 512), ("ΣΑΣ", 512),
             ("x蛋白ab", 512), ("bind\u00ading", 512), (SENTENCE, 7), ("", 512)]
    return [(t, m, True) for t, m in low] + [(t, m, False) for t, m in cased]


def main():
    from tokenizers import BertWordPieceTokenizer
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vocab.txt")
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(VOCAB) + "\n")
        toks = {flag: BertWordPieceTokenizer(path, lowercase=flag) for flag in (True, False)}
        for text, max_length, lowercase in cases():
            tok = toks[lowercase]
            tok.enable_truncation(max_length=max_length)
            out.append({"text": text, "max_length": max_length, "lowercase": lowercase, "ids": tok.encode(text).ids})
    with open(os.path.join(HERE, "wordpiece.json"), "w") as f:
        json.dump({"vocab": VOCAB, "cases": out}, f, separators=(",", ":"))
        f.write("\n")
    print(len(out), "cases,", sum(len(c["ids"]) for c in out), "ids")


if __name__ == "__main__":
    main()
