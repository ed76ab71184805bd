"""The MSA input path without a GPU (oneprot_amd/msa_data.py): the a3m reader, the exact selection rule on the host path against the reference's recorded
selections (tests/golden/msa_select.json, tie-free inputs) and against the restatement (tests/msa_select_ref.py), the token layouts, the collate."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests import msa_select_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_select.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_is_tie_free_and_not_vacuous(golden):
    per_mode = {"max": 0, "min": 0}
    for c in golden["cases"]:
        rows = R.to_bytes(c["seqs"])
        assert rows.shape[0] >= 20 and rows.shape[1] >= 100 and 4 <= c["num_seqs"] < rows.shape[0]
        _, _, tie_free = R.greedy(rows, c["num_seqs"], c["mode"])
        assert tie_free, "a fixture case with a tie at the top pins nothing"
        assert len(c["selected"]) == c["num_seqs"] and c["selected"][0] == 0
        per_mode[c["mode"]] += 1
    assert per_mode["max"] >= 6 and per_mode["min"] >= 6


def test_restatement_and_host_path_equal_the_reference_selections(golden):
    from oneprot_amd import msa_data as D
    for c in golden["cases"]:
        rows = R.to_bytes(c["seqs"])
        want, order, _ = R.greedy(rows, c["num_seqs"], c["mode"])
        assert want == c["selected"]
        idx, picks = D.select_host(rows, c["num_seqs"], c["mode"])
        assert idx == c["selected"] and picks == order
        msa = [(f"r{i}", s) for i, s in enumerate(c["seqs"])]
        got = D.greedy_select(msa, c["num_seqs"], mode=c["mode"], device="cpu")
        assert got == [msa[i] for i in c["selected"]]
        table = D.select_batch([rows], c["num_seqs"], c["mode"], "cpu")
        assert table.dtype == torch.int32 and table.tolist() == [c["selected"]]


@pytest.mark.parametrize("mode", ["max", "min"])
def test_host_path_equals_the_restatement_on_tie_heavy_inputs(mode):
    from oneprot_amd import msa_data as D
    cases = [R.draw(1, 40, 17, letters="AC"), R.draw(2, 33, 5, letters="AC"), ["ACDEFG"] * 9, R.draw(3, 12, 40) * 3, R.draw(4, 64, 33, kind="mutated"), ["A", "C"]]
    for seqs in cases:
        rows = R.to_bytes(seqs)
        for k in (1, 2, 7, len(seqs) - 1, len(seqs), len(seqs) + 1):
            if k < 1:
                continue
            want, order, _ = R.greedy(rows, k, mode)
            assert D.select_host(rows, k, mode) == (want, order)
    assert D.select_host(R.to_bytes(["ACDEFG"] * 9), 9, mode)[1] == list(range(9))          # every step a tie: the lowest index each time
    # a batch: each MSA at its own depth, -1 behind the picks
    arrays, ks = [R.to_bytes(c) for c in cases[:3]], [5, 40, 2]
    idx, order = D.select_batch(arrays, ks, mode, "cpu", want_order=True)
    assert tuple(idx.shape) == (3, 40)
    for b, (a, k) in enumerate(zip(arrays, ks)):
        want, picks, _ = R.greedy(a, k, mode)
        assert idx[b].tolist() == want + [-1] * (40 - len(want)) and order[b].tolist() == picks + [-1] * (40 - len(picks))


def test_greedy_select_edges_and_refusals():
    from oneprot_amd import msa_data as D
    msa = [(f"d{i}", s) for i, s in enumerate(R.draw(5, 10, 20))]
    assert D.greedy_select(msa, 10, device="cpu") is msa and D.greedy_select(msa, 11, device="cpu") is msa
    assert D.greedy_select(msa, 1, device="cpu") == msa[:1]
    with pytest.raises(AssertionError):
        D.greedy_select(msa, 3, mode="mean")
    with pytest.raises(ValueError):
        D.select_batch([np.zeros((3, 4), dtype=np.int64)], 2, "max", "cpu")
    with pytest.raises(ValueError):
        D.select_batch([np.zeros((3, 4), dtype=np.uint8)], 1025, "max", "cpu")
    with pytest.raises(ValueError):
        D.select_batch([np.zeros((3, 0), dtype=np.uint8)], 2, "max", "cpu")
    with pytest.raises(ValueError):
        D.select_batch([], 2, "max", "cpu")


def test_signatures_equal_the_reference(golden):
    from src.data.datasets.msa_dataset import MSADataset
    from src.data.utils import msa_utils

    def sig(fn):
        return [[p.name, None if p.default is inspect.Parameter.empty else p.default, p.default is not inspect.Parameter.empty]
                for p in inspect.signature(fn).parameters.values() if p.name != "self"]
    ours = sig(msa_utils.greedy_select)
    assert ours[:3] == golden["signatures"]["greedy_select"] and ours[3:] == [["device", None, True]]
    assert sig(MSADataset.__init__) == golden["signatures"]["MSADataset"]
    for name in ("filter_and_create_msa_file_list", "remove_insertions", "read_msa", "greedy_select"):
        assert callable(getattr(msa_utils, name))


A3M = """>query some description
ACDE
FGHIK
>hit1 e=1e-5
AC-EfgFG
HIK
>hit2
acdACDEF.*GH-K
"""


def test_reader(tmp_path):
    from oneprot_amd import msa_data as D
    assert D.remove_insertions("AbC.d*E-") == "ACE-"
    p = tmp_path / "fam.a3m"
    p.write_text(A3M)
    want = [("query some description", "ACDEFGHIK"), ("hit1 e=1e-5", "AC-EFGHIK"), ("hit2", "ACDEFGH-K")]
    assert D.read_msa(str(p)) == want
    assert D.read_msa(str(tmp_path / "fam")) == want                      # the `filename + '.a3m'` fallback
    with pytest.raises(OSError):
        D.read_msa(str(tmp_path / "absent"))
    bad = tmp_path / "bad.a3m"
    bad.write_text(">a\nACDE\n>b\nACD\n")
    with pytest.raises(ValueError, match="unequal"):
        D.read_msa(str(bad))
    lst = tmp_path / "train_msa.csv"
    lst.write_text("id,path\n7,/data/x/fam1.a3m,extra\n8,/data/x/fam2.a3m\n9,/data/x/other.txt\n")
    assert D.filter_and_create_msa_file_list(str(lst)) == ["/data/x/fam1.a3m", "/data/x/fam2.a3m"]


def test_token_table():
    from oneprot_amd import msa_data as D
    conv = D.MsaBatchConverter(max_length=1024)
    assert conv.byte_map.shape == (256,) and conv.byte_map.tolist() == [R.token_of(b) for b in range(256)]
    assert [conv.byte_map[ord(c)] for c in "LAGVSERTIDPKQNFYMHWCXBUZO.-"] == list(range(4, 31))
    assert conv.all_toks.index("<null_1>") == 31 and conv.all_toks.index("<mask>") == 32 and len(conv.all_toks) == 33
    assert (conv.cls_idx, conv.padding_idx, conv.eos_idx, conv.unk_idx, conv.mask_idx) == (0, 1, 2, 3, 32)
    assert conv.byte_map[ord("a")] == 3 and conv.byte_map[0] == 3 and conv.byte_map[255] == 3


@pytest.mark.parametrize("max_length", [8, 1024])
def test_host_tokens_and_truncations(max_length):
    from oneprot_amd import msa_data as D
    from oneprot_amd.packing import PackedMsa
    seqs = [R.draw(11, 6, 1030, letters=R.ALPHABET + "J?"), R.draw(12, 3, 5), R.draw(13, 9, 1022), R.draw(14, 2, 1021)]
    arrays = [R.to_bytes(s) for s in seqs]
    ks = [4, 5, 3, 2]
    conv = D.MsaBatchConverter(max_length=max_length)
    indices = D.select_batch(arrays, ks, "max", "cpu")
    picks = [R.greedy(a, k, "max")[0] for a, k in zip(arrays, ks)]
    blocks = [R.msa_tokens(a, p, max_length) for a, p in zip(arrays, picks)]
    assert blocks[0].shape == (4, min(1023, max_length)) and blocks[1].shape == (3, min(6, max_length))
    seq, tokens = conv.host(arrays, indices)
    assert tokens.dtype == torch.int64 and np.array_equal(tokens.numpy(), R.padded_batch(blocks))
    want_seq = R.padded_seqs([R.seq_tokens(a[0], max_length) for a in arrays])
    assert seq.dtype == torch.int64 and np.array_equal(seq.numpy(), want_seq)
    assert (seq[:, 0] == 0).all() and seq[0, min(1032, max_length) - 1] == 2                    # <eos> kept under truncation
    seq2, pk = conv.host(arrays, indices, packed=True)
    assert isinstance(pk, PackedMsa) and torch.equal(seq2, seq)
    ref = PackedMsa.from_padded(tokens)
    assert pk.shapes == ref.shapes == [b.shape for b in blocks]
    assert all(torch.equal(u, v) for u, v in zip(pk.unpack(), ref.unpack()))


def _write_family(tmp_path, name, seqs):
    p = tmp_path / name
    p.write_text("".join(f">s{i} of {name}\n{s}\n" for i, s in enumerate(seqs)))
    return str(p)


def test_dataset_and_collate_on_the_host_path(tmp_path):
    from oneprot_amd.packing import PackedMsa
    from src.data.datasets.msa_dataset import MSADataset
    fams = [R.draw(21, 5, 30), R.draw(22, 40, 64, kind="mutated"), R.draw(23, 25, 130)]
    files = [_write_family(tmp_path, f"fam{i}.a3m", s) for i, s in enumerate(fams)]
    (tmp_path / "train_msa.csv").write_text("".join(f"{i},{f}\n" for i, f in enumerate(files)))
    ds = MSADataset(str(tmp_path), "train", max_length=100, msa_depth=16, model_name_or_path="/nonexistent/model.pt")
    assert len(ds) == 3 and ds[1] == files[1] and ds.msa_padding_idx == 1 and ds.device is None and ds.packed_msa is False
    assert len(MSADataset(str(tmp_path), "train")) == 3
    (tmp_path / "val_msa.csv").write_text(f"0,{files[0]}\n")
    assert len(MSADataset(str(tmp_path), "val")) == 1000
    ds.device = "cpu"
    seq, msa, modality, sequences = ds.collate_fn(files)
    assert modality == "msa" and sequences == [f[0] for f in fams]
    arrays = [R.to_bytes(f) for f in fams]
    blocks = [R.msa_tokens(a, R.greedy(a, 16, "max")[0], 100) for a in arrays]
    assert tuple(msa.shape) == (3, 16, 100) and np.array_equal(msa.numpy(), R.padded_batch(blocks))
    assert np.array_equal(seq.numpy(), R.padded_seqs([R.seq_tokens(a[0], 100) for a in arrays]))
    ds.packed_msa = True
    seq2, pk, _, _ = ds.collate_fn(files)
    assert isinstance(pk, PackedMsa) and pk.shapes == [(5, 31), (16, 65), (16, 100)] and torch.equal(seq2, seq)
    assert all(np.array_equal(u.numpy(), v) for u, v in zip(pk.unpack(), blocks))


def test_new_symbols_in_the_header_and_the_library():
    from oneprot_amd import hip
    from ctypes import c_int, c_int64, c_size_t, c_void_p
    P, I, L64, SZ = c_void_p, c_int, c_int64, c_size_t
    assert hip._SIGS["oneprot_msa_select_workspace"] == (SZ, [I, I, L64, L64])
    assert hip._SIGS["oneprot_msa_select"] == (I, [P, P, P, P, P, P, SZ, L64, I, I, I, P])
    assert hip._SIGS["oneprot_msa_tokenize"] == (I, [P, P, P, P, P, P, P, P, L64, I, I, I, I, I, I, L64, I, I, I, P])
    assert hip._PTR_DTYPES["oneprot_msa_select"] == "blbiil" and hip._PTR_DTYPES["oneprot_msa_tokenize"] == "bliilill"
    assert hip.ABI_VERSION == 7
    if os.path.exists(hip.LIB_PATH):                                   # built: the symbols are in the library, and the size query runs without a GPU
        h = hip.lib()
        assert h.oneprot_msa_select_workspace(16, 50, 160000, 10000) >= 160000 * 4 + 16 * 50 * 4
        assert h.oneprot_msa_select_workspace(0, 50, 10, 10) == 0 and h.oneprot_msa_select_workspace(1, 1025, 10, 10) == 0
