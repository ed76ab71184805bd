"""csrc/wordpiece.hip against the host rule (BertWordPieceTokenizer.encode_all), id for id: the fixture's cases, batches past the CU count, texts of
several chunks with a character and a word across every chunk edge, a hash table small enough to collide, both layouts, run-to-run bytes, refusals."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from oneprot_amd import hip
from oneprot_amd.text_data import BertWordPieceTokenizer, piece_key

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wordpiece.json")
CHUNK = 256                       # bytes a work-group decodes per step (kChunk of csrc/wordpiece.hip)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def toks(golden):
    return {flag: BertWordPieceTokenizer(golden["vocab"], lowercase=flag) for flag in (True, False)}


def host(tok, texts, max_length):
    flat, off = tok.encode_all(texts, max_length)
    ids = np.full((len(texts), max_length), tok.pad_id, dtype=np.int64)
    lens = np.diff(off)
    ids[np.arange(max_length)[None, :] < lens[:, None]] = flat
    return ids, lens


def check(tok, texts, max_length):
    ids, lengths = tok.encode_device(texts, max_length, "cuda")
    want_ids, want_lens = host(tok, texts, max_length)
    assert lengths.cpu().tolist() == want_lens.tolist()
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    return ids, lengths


def test_fixture_in_batches_and_one_at_a_time(golden, toks):
    groups = {}
    for c in golden["cases"]:
        groups.setdefault((c["lowercase"], c["max_length"]), []).append(c)
    for (flag, ml), cs in groups.items():
        ids, lengths = check(toks[flag], [c["text"] for c in cs], ml)
        for row, n, c in zip(ids.cpu().tolist(), lengths.cpu().tolist(), cs):
            assert row[:n] == c["ids"]
    for c in golden["cases"]:
        ids, lengths = check(toks[c["lowercase"]], [c["text"]], c["max_length"])
        assert ids[0, :int(lengths[0])].cpu().tolist() == c["ids"]


def test_one_text_and_more_texts_than_cus(toks):
    tok = toks[True]
    check(tok, ["the protein binding kinases"], 16)
    words = ["the", "protein", "binding", "ing", "kinases", "蛋", "각", "!", "bindingq", "a" * 100, "a" * 101, ""]
    check(tok, [words[i % len(words)] for i in range(300)], 12)


def _fill_to(parts, target):
    """append 'the ' words and spaces until the text is `target` bytes long"""
    have = sum(len(p.encode("utf-8")) for p in parts)
    assert have <= target
    n = target - have
    parts.append("the " * (n // 4) + " " * (n % 4))


@pytest.mark.parametrize("shift", [1, 2])
def test_character_and_word_across_every_chunk_edge(toks, shift):
    tok = toks[True]
    texts = []
    for which in (0, 1):                                    # the 100-character word across the odd edges and the 3-byte character across the even ones, then swapped
        parts = []
        for edge in range(1, 7):
            if edge % 2 == which:
                _fill_to(parts, edge * CHUNK - 60)
                parts.append("a" * 100 + " ")
            else:
                _fill_to(parts, edge * CHUNK - shift)
                parts.append("蛋")
        raw = "".join(parts).encode("utf-8")
        for edge in range(1, 7):
            if edge % 2 == which:
                assert raw[edge * CHUNK - 60:edge * CHUNK + 40] == b"a" * 100
            else:
                assert raw[edge * CHUNK - shift:edge * CHUNK - shift + 3] == "蛋".encode("utf-8")
        texts.append("".join(parts))
    texts.append("the " * 70 + "a" * 101 + " the " + "a" * 300 + " protein " + "각" * 90 + " binding")        # 101 and 300 characters across edges; Hangul expands to 3
    texts.append("a" * 95 + "蛋" * 200 + "a" * 100)
    ids, lengths = check(tok, texts, 2048)
    assert int(lengths.max()) > 500
    check(tok, texts, 64)                                   # stops early, inside the first chunks
    check(tok, texts, 301)


def test_tiny_table_with_collisions():
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "ab", "##ab", "ba", "##ba", "a", "##a", "b", "##b", "abc", "##c", "cab"]
    tok = BertWordPieceTokenizer(vocab, table_slots=16)
    slots, _ = tok.hash_table()
    homes = [piece_key(p, cont) & 15 for cont, table in enumerate(tok.pieces) for p in table]
    assert len(set(homes)) < len(homes), "no two pieces share a home slot: the table is not small enough"
    occupied = {s for s in range(16) if slots[s, 3] >= 0}
    assert len(occupied) == len(homes) == 15 and len(tok.pieces[0]) + len(tok.pieces[1]) == 15
    strangers = ["".join(w) for n in (1, 2, 3) for w in itertools.product("abcd", repeat=n)]
    strangers = [w for w in strangers if w not in tok.pieces[0] and piece_key(w, 0) & 15 in occupied]
    assert len(strangers) >= 8
    texts = strangers + ["ab ba abc cab abab baab aabbc d ad da abcd", "cabcab", "c", "cc"] + [" ".join(strangers)]
    check(tok, texts, 64)


def test_padded_equals_packed_and_runs_repeat(toks):
    tok = toks[True]
    texts = ["the protein binding kinases", "", "café résumé 蛋白", "a" * 100 + " the", "unaffectable!"] * 3
    padded = tok(texts, max_length=32, device="cuda")
    packed = tok(texts, max_length=32, device="cuda", packed=True)
    want = tok(texts, max_length=32, device="cpu")
    assert padded.dtype == torch.int64 and torch.equal(padded.cpu(), want)
    assert packed.pad_id == 0 and torch.equal(packed.to_padded().cpu(), want)
    host_packed = tok(texts, max_length=32, device="cpu", packed=True)
    assert packed.lengths == host_packed.lengths and torch.equal(packed.ids.cpu(), host_packed.ids)
    a, la = tok.encode_device(texts, 32, "cuda")
    b, lb = tok.encode_device(texts, 32, "cuda")
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes()


def test_refusals_launch_nothing(toks):
    tok = toks[True]
    dev = torch.device("cuda")
    index, entries, pool, slots, chars = tok._device_tables(dev)
    raw = b"the protein"
    data = torch.tensor(list(raw), dtype=torch.uint8, device=dev)
    off = torch.tensor([0, 3, len(raw)], dtype=torch.int64)
    off_dev = off.to(dev)
    ML = 8
    ids = torch.full((2, ML), -7, dtype=torch.int32, device=dev)
    lengths = torch.full((2,), -7, dtype=torch.int32, device=dev)
    good = dict(off_host=off, n_bytes=len(raw), n=2, n_blocks=entries.shape[0], n_pool=pool.numel(), n_slots=slots.shape[0], n_chars=chars.numel(),
                max_piece=tok.max_piece_chars, ml=ML, cls=tok.cls_id, sep=tok.sep_id, unk=tok.unk_id, pad=tok.pad_id, slots=slots, ids=ids)

    def call(**kw):
        a = dict(good, **kw)
        hip.call("oneprot_wordpiece_encode", data, off_dev, index, entries, pool, a["slots"], chars, a["ids"], lengths, a["off_host"].data_ptr(), a["n_bytes"],
                 a["n"], a["n_blocks"], a["n_pool"], a["n_slots"], a["n_chars"], a["max_piece"], a["ml"], a["cls"], a["sep"], a["unk"], a["pad"])

    bad = [dict(n=0), dict(n=hip._consts["WORDPIECE_MAX_TEXTS"] + 1), dict(ml=1), dict(ml=hip._consts["WORDPIECE_MAX_LENGTH"] + 1), dict(n_bytes=len(raw) - 1),
           dict(n_bytes=-1), dict(off_host=torch.tensor([0, 5, 3], dtype=torch.int64)), dict(off_host=torch.tensor([-1, 3, 11], dtype=torch.int64)),
           dict(n_slots=slots.shape[0] - 1), dict(n_slots=1), dict(n_slots=0), dict(n_blocks=0), dict(n_blocks=0x1101), dict(n_pool=0), dict(n_chars=0),
           dict(max_piece=0), dict(max_piece=101), dict(cls=-1), dict(sep=-1), dict(unk=-1), dict(pad=-1), dict(slots=slots.view(-1)[1:]), dict(ids=None)]
    for kw in bad:
        with pytest.raises(hip.HipKernelError):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool((lengths == -7).all())
    call()
    want_ids, want_lens = host(tok, ["the", " protein"], ML)
    assert lengths.cpu().tolist() == want_lens.tolist() and np.array_equal(ids.cpu().numpy(), want_ids)
    with pytest.raises(ValueError, match="surrogate"):
        tok(["a\ud800b"], device="cuda")
