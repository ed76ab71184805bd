"""The host side of the text input (oneprot_amd/text_data.py): the rule against tests/golden/wordpiece.json and, where `tokenizers` imports, against the
library itself on random strings; the fixture's coverage; the normalisation table against the five steps per character; the hash table; the header and
binding of the new entry point."""
import json
import os
import random
import re
import unicodedata

import numpy as np
import pytest
import torch

from oneprot_amd import hip, text_data
from oneprot_amd.text_data import (KIND_OTHER, KIND_SOLO, KIND_SPACE, MAX_EXPANSION, BertWordPieceTokenizer, is_cjk, norm_table, normalize_char,
                                   piece_key)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "wordpiece.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def toks(golden):
    return {flag: BertWordPieceTokenizer(golden["vocab"], lowercase=flag) for flag in (True, False)}


def test_host_rule_equals_the_fixture(golden, toks):
    assert len(golden["cases"]) >= 50
    for c in golden["cases"]:
        flat, off = toks[c["lowercase"]].encode_all([c["text"]], c["max_length"])
        assert off.tolist() == [0, len(c["ids"])] and flat.tolist() == c["ids"], (c["text"][:40], c["max_length"], c["lowercase"])
    # and as one batch per max_length, through the padded call
    for flag in (True, False):
        cs = [c for c in golden["cases"] if c["lowercase"] == flag and c["max_length"] == 512]
        out = toks[flag]([c["text"] for c in cs], max_length=512, device="cpu")
        assert out.dtype == torch.int64 and out.shape == (len(cs), max(len(c["ids"]) for c in cs))
        for row, c in zip(out.tolist(), cs):
            assert row[:len(c["ids"])] == c["ids"] and set(row[len(c["ids"]):]) <= {0}


def test_fixture_holds_every_case(golden, toks):
    """a vacuous fixture fails here: every case of the list is found by its own property, not by a label"""
    vocab = golden["vocab"]
    low = [c for c in golden["cases"] if c["lowercase"]]
    tok = toks[True]
    cls, sep, unk = tok.cls_id, tok.sep_id, tok.unk_id
    texts = [c["text"] for c in golden["cases"]]
    assert not any(s in t for t in texts for s in ("[CLS]", "[SEP]", "[UNK]", "[PAD]", "[MASK]")), "a literal special token is a known difference"
    assert any(c["lowercase"] is False for c in golden["cases"])
    body = lambda c: c["ids"][1:-1]
    assert all(c["ids"][0] == cls and c["ids"][-1] == sep for c in golden["cases"])
    assert any(c["text"] == "" and c["ids"] == [cls, sep] for c in low)
    assert any(c["text"] and c["text"].isspace() and c["ids"] == [cls, sep] for c in low)
    full = [c for c in low if c["max_length"] == 512]
    words_of = lambda c: tok.words(c["text"])
    # a word that exists only as a ## piece
    assert any(len(words_of(c)) == 1 and words_of(c)[0] not in tok.pieces[0] and words_of(c)[0] in tok.pieces[1] and body(c) == [unk] for c in full)

    def fails_late(word):
        """earlier pieces match, the last position does not"""
        start, n = 0, len(word)
        while start < n:
            table = tok.pieces[1 if start else 0]
            end = n
            while end > start and word[start:end] not in table:
                end -= 1
            if end == start:
                return start > 0 and n - start == 1
            start = end
        return False
    assert any(any(fails_late(w) for w in words_of(c)) and unk in body(c) for c in full)
    assert any(words_of(c) == ["a" * 100] and len(body(c)) == 100 and unk not in body(c) for c in full)
    assert any(words_of(c) == ["a" * 101] and body(c) == [unk] for c in full)
    punct = lambda ch: unicodedata.category(ch).startswith("P")
    assert any(len(c["text"]) >= 4 and all(punct(ch) for ch in c["text"]) and len(body(c)) == len(c["text"]) and unk not in body(c) for c in full)
    assert any(re.search(r"[a-z][\u4e00-\u9fff]|[\u4e00-\u9fff][a-z]", c["text"]) and unk not in body(c) for c in full)
    assert any(any(0xAC00 <= ord(ch) <= 0xD7A3 and len(unicodedata.normalize("NFD", ch)) == 3 for ch in c["text"]) and unk not in body(c) and len(body(c)) >= 3
               for c in full)
    assert any(any(unicodedata.category(ch) == "Mn" for ch in unicodedata.normalize("NFD", c["text"])) and unk not in body(c) and body(c) for c in full)
    assert any("İ" in c["text"] and body(c) == [vocab.index("i")] for c in full)
    assert any(c["text"] == "ΣΑΣ" and body(c) == [vocab.index("σ"), vocab.index("##α"), vocab.index("##σ")] for c in full)
    for ch in ("\x0b", "\x0c", "\u0085", "\u00ad", "\u200b", "\x00", "\ufffd"):              # dropped
        assert any(ch in c["text"] and unk not in body(c) for c in full), hex(ord(ch))
    for ch in ("\t", "\n", "\r", "\u3000"):                                                       # mapped to a space
        assert any(ch in c["text"] and unk not in body(c) for c in full), hex(ord(ch))
    assert any(any(ord(ch) > 0xFFFF for ch in c["text"]) and unk not in body(c) for c in full)
    assert any("\u0903" in c["text"] and vocab.index("##\u0903") in body(c) for c in full)          # an Mc sign is kept
    # truncation: a text of P pieces at max_length P + 3, P + 2 and P + 1, the last one cutting inside a word's pieces
    by_text = {}
    for c in low:
        by_text.setdefault(c["text"], {})[c["max_length"]] = c["ids"]
    found = False
    for text, runs in by_text.items():
        if 512 not in runs:
            continue
        whole = runs[512][1:-1]
        P = len(whole)
        if P >= 2 and all(P + d in runs for d in (1, 2, 3)):
            assert runs[P + 3] == runs[P + 2] == [cls] + whole + [sep] and runs[P + 1] == [cls] + whole[:-1] + [sep]
            assert vocab[whole[-1]].startswith("##"), "the cut does not fall inside a word's pieces"
            found = True
    assert found
    assert any(c["max_length"] == 2 and c["text"] and c["ids"] == [cls, sep] for c in low)
    assert any(c["max_length"] == 3 and len(c["ids"]) == 3 for c in low)


def _random_strings(rng, n):
    ranges = [(0x20, 0x7E), (0xA0, 0xFF), (0x100, 0x17F), (0x370, 0x3FF), (0x400, 0x4FF), (0x4E00, 0x4E80), (0xAC00, 0xAC80), (0x2000, 0x206F), (0x300, 0x36F)]
    weights = [12, 2, 2, 2, 2, 1, 1, 1, 1]
    out = []
    for _ in range(n):
        chars = []
        for _ in range(rng.randint(0, 60)):
            if rng.random() < 0.18:
                chars.append(" ")
            else:
                lo, hi = rng.choices(ranges, weights)[0]
                chars.append(chr(rng.randint(lo, hi)))
        out.append("".join(chars))
    return out


@pytest.mark.parametrize("lowercase", [True, False])
def test_random_strings_against_tokenizers(tmp_path, lowercase):
    tokenizers = pytest.importorskip("tokenizers")
    rng = random.Random(1881 + lowercase)
    strings = _random_strings(rng, 500)
    probe = BertWordPieceTokenizer(["[PAD]", "[UNK]", "[CLS]", "[SEP]"], lowercase=lowercase)
    pieces = set()
    for s in strings:
        for w in probe.words(s):
            if rng.random() < 0.75:                                # most words can be matched, whole or in two pieces
                k = rng.randint(1, len(w))
                pieces.add(w[:k])
                if k < len(w):
                    pieces.add("##" + w[k:])
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + sorted(pieces)
    path = tmp_path / "vocab.txt"
    path.write_text("\n".join(vocab) + "\n", encoding="utf-8")
    ours = BertWordPieceTokenizer(str(path), lowercase=lowercase)
    theirs = tokenizers.BertWordPieceTokenizer(str(path), lowercase=lowercase)
    words = unknown = 0
    for max_length in (512, 12):
        theirs.enable_truncation(max_length=max_length)
        flat, off = ours.encode_all(strings, max_length)
        for s, a, b in zip(strings, off[:-1], off[1:]):
            assert flat[a:b].tolist() == theirs.encode(s).ids, (s, max_length)
    for s in strings:
        for w in ours.words(s):
            words += 1
            unknown += ours.word_pieces(w) == [ours.unk_id]
    print(f"{words} words, {unknown} of them [UNK]")
    assert words > 1000 and 2 * unknown <= words, "the match would be trivial if most words were unknown"


def _five_steps(cp, lowercase):
    """the rule computed per character with unicodedata, written independently of normalize_char: [(code point, kind)]"""
    ch = chr(cp)
    if cp in (0, 0xFFFD):
        return []
    if ch not in "\t\n\r" and unicodedata.category(ch) in ("Cc", "Cf", "Co", "Cs"):
        return []
    white = cp in (9, 10, 13, 0x20, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000) or 0x2000 <= cp <= 0x200A
    if white:
        return [(0x20, KIND_SPACE)]
    s = ch
    if lowercase:
        s = "".join(c.lower() for c in unicodedata.normalize("NFD", s) if unicodedata.category(c) != "Mn")
    cjk = (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F or 0x2B740 <= cp <= 0x2B81F
           or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)
    out = []
    for c in s:
        solo = cjk or (ord(c) < 128 and not c.isalnum() and not c.isspace() and c.isprintable()) or unicodedata.category(c).startswith("P")
        out.append((ord(c), KIND_SOLO if solo else KIND_OTHER))
    return out


@pytest.mark.parametrize("lowercase", [True, False])
def test_normalisation_table_is_the_five_step_rule(lowercase):
    index, entries, pool = norm_table(lowercase)
    assert index.shape == (0x1100,) and entries.shape[1] == 256 and index.max() < entries.shape[0]

    def from_table(cp):
        e = int(entries[index[cp >> 8], cp & 255])
        count = (e >> 23) & 3
        if count <= 1:
            return [(e & 0x1FFFFF, (e >> 21) & 3)] * count
        return [(int(pool[(e & 0x1FFFFF) + k]) & 0x1FFFFF, (int(pool[(e & 0x1FFFFF) + k]) >> 21) & 3) for k in range(count)]
    rng = random.Random(7)
    sample = ([0xAC00, 0xAC01, 0xD7A3, 0xD800, 0xDFFF, 0xE000, 0xF900, 0xFA0E, 0xFAFF, 0xFB00, 0xFEFF, 0xFF21, 0xFFFD, 0xFFFF, 0x10000, 0x10400, 0x1D15E, 0x1D400, 0x1F600,
               0x20000, 0x2A6DF, 0x2A6E0, 0x2CEAF, 0x2CEB0, 0x2F800, 0x2FA1F, 0x30000, 0x3FFFF, 0xE0001, 0xE0100, 0xE01EF, 0xF0000, 0x10FFFD, 0x10FFFF]
              + [rng.randrange(0x3000, 0x110000) for _ in range(20000)])
    widest = 0
    for cp in list(range(0x3000)) + sample:
        got = from_table(cp)
        assert got == _five_steps(cp, lowercase), hex(cp)
        assert [(ord(c), k) for c, k in normalize_char(chr(cp), lowercase)] == got
        widest = max(widest, len(got))
    assert widest == (MAX_EXPANSION if lowercase else 1)
    if lowercase:
        assert from_table(0xAC01) == [(0x1100, KIND_OTHER), (0x1161, KIND_OTHER), (0x11A8, KIND_OTHER)]
        assert from_table(0x130) == [(ord("i"), KIND_OTHER)] and from_table(0x3A3) == [(0x3C3, KIND_OTHER)] and from_table(0x226E) == [(ord("<"), KIND_SOLO)]
    assert from_table(0x378) == [(0x378, KIND_OTHER)] and from_table(0xAD) == [] and from_table(0x2028) == [(0x20, KIND_SPACE)] and is_cjk(0x4E00)


def test_hash_table_holds_every_piece_once(golden, toks):
    tok = toks[True]
    slots, chars = tok.hash_table()
    cap = slots.shape[0]
    n = len(tok.pieces[0]) + len(tok.pieces[1])
    assert cap & (cap - 1) == 0 and cap >= 2 * n and int((slots[:, 3] >= 0).sum()) == n

    def find(piece, cont):
        key = piece_key(piece, cont)
        s = key & (cap - 1)
        while slots[s, 3] >= 0:
            k, at, meta, idx = (int(v) for v in slots[s])
            if k & 0xFFFFFFFF == key and meta == len(piece) | (cont << 16) and chars[at:at + len(piece)].tolist() == [ord(c) for c in piece]:
                return idx
            s = (s + 1) & (cap - 1)
        return -1
    for cont, table in enumerate(tok.pieces):
        for piece, idx in table.items():
            assert find(piece, cont) == idx
    assert find("ing", 0) == -1 and find("ing", 1) == golden["vocab"].index("##ing") and find("the", 1) == -1
    with pytest.raises(ValueError):
        BertWordPieceTokenizer(golden["vocab"], table_slots=len(golden["vocab"]) - 10).hash_table()


def test_vocab_sources_and_refusals(tmp_path, golden):
    (tmp_path / "vocab.txt").write_text("\n".join(golden["vocab"]) + "\n", encoding="utf-8")
    from_file = BertWordPieceTokenizer(str(tmp_path / "vocab.txt"))
    from_dir = BertWordPieceTokenizer(str(tmp_path))
    assert from_file.vocab == from_dir.vocab and from_dir.lowercase is True
    (tmp_path / "tokenizer_config.json").write_text(json.dumps({"do_lower_case": False}))
    assert BertWordPieceTokenizer(str(tmp_path)).lowercase is False
    with pytest.raises(ValueError, match="local path"):
        BertWordPieceTokenizer("allenai/scibert_scivocab_uncased")
    with pytest.raises(ValueError, match=r"\[UNK\]"):
        BertWordPieceTokenizer(["[CLS]", "[SEP]", "a"])
    with pytest.raises(ValueError, match="surrogate"):
        from_file.encode_all(["a\ud800b"])
    with pytest.raises(ValueError, match="surrogate"):
        from_file(["a\udfffb"], device="cpu")
    with pytest.raises(ValueError):
        from_file.encode_all(["a"], max_length=1)
    packed = from_file(["the protein", "binding"], max_length=16, device="cpu", packed=True)
    assert packed.pad_id == 0 and torch.equal(packed.to_padded(), from_file(["the protein", "binding"], max_length=16, device="cpu"))
    assert text_data.DEVICE_MIN_BYTES > 0


def test_header_declares_the_text_input():
    assert hip.ABI_VERSION == 7
    src = open(text_data.__file__).read()
    called = set(re.findall(r'"(oneprot_\w+)"', src))
    assert called == {"oneprot_wordpiece_encode"} and called <= set(hip._SIGS)
    header = open(hip.HEADER_PATH).read()
    assert re.search(r"\boneprot_wordpiece_encode\s*\(", header) and "text input" in header and "text_dataset.py:25,51" in header
    assert hip._PTR_DTYPES["oneprot_wordpiece_encode"] == "bliiiiiiil"
    restype, argtypes = hip._SIGS["oneprot_wordpiece_encode"]
    assert len(argtypes) == 23
    assert hip._consts["WORDPIECE_MAX_LENGTH"] == 65535 and hip._consts["WORDPIECE_MAX_TEXTS"] == 1 << 20
    build = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "build.sh")).read()
    assert "wordpiece.hip" in build
    kernel = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "wordpiece.hip")).read()
    assert "float" not in kernel and "atomic" not in kernel.replace("no atomics", "")
