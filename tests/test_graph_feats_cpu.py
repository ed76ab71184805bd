"""The batch featurisation of the pocket / struct_graph modalities without a GPU (oneprot_amd/graph_data.py: read_records, prepare_batch,
featurize_batch on the host path, synthetic_atom_records) and the declaration of its entry point (include/oneprot_hip.h)."""
import ctypes
import os
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from oneprot_amd import graph_data as G
from oneprot_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "struct_graph_feats.pt")
KEYS = ("x", "coords_ca", "coords_n", "coords_c", "bb_embs", "side_chain_embs", "batch", "ptr")
LETTERS = "ARNDCQEGHILKMFPSTWYVX"


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=True)["proteins"]


def golden_records(golden):
    return [(p["amino_types"], p["atom_amino_id"].numpy(), np.array(p["atom_names"], dtype="S"), p["atom_pos"].numpy()) for p in golden]


def mapping(records):
    """records as the structure file's nested layout"""
    return {f"P{k}": {"structure": {"0": {"A": {"residues": {"seq1": "".join(LETTERS[a] for a in r[0]).encode()},
                                                "polypeptide": {"atom_amino_id": r[1], "type": r[2], "xyz": r[3]}}}}} for k, r in enumerate(records)}


def same_batch(got, want):
    assert got.num_graphs == want.num_graphs
    for k in KEYS:
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), k


def legacy(records):
    file = mapping(records)
    return G.GraphBatch.from_data_list([G.protein_to_graph(k, file) for k in file])


def test_host_path_equals_protein_to_graph_and_from_data_list(golden):
    gen = torch.Generator().manual_seed(17)
    for records in (golden_records(golden), [G.synthetic_atom_records(n, gen) for n in (1, 2, 40, 90)]):
        same_batch(G.featurize_batch(records, device="cpu"), legacy(records))
    # fewer distinct ids than residues: the trailing residues are NaN rows (coordinates) with angle-0 features
    types, ids, names, pos = G.synthetic_atom_records(12, gen)
    short = (np.concatenate([types, [3, 7]]).astype(np.uint8), ids, names, pos)
    got = G.featurize_batch([short, golden_records(golden)[0]], device="cpu")
    same_batch(got, legacy([short, golden_records(golden)[0]]))
    assert torch.isnan(got.coords_ca[12:14]).all() and not torch.isnan(got.coords_ca[:12]).any()
    assert torch.equal(got.side_chain_embs[12:14], torch.tensor([[0.0] * 4 + [1.0] * 4] * 2))
    with pytest.raises(ValueError):
        G.featurize_batch([], device="cpu")
    with pytest.raises(ValueError):
        G.prepare_batch([])


def test_protein_to_graph_after_the_split_returns_the_golden(golden):
    file = mapping(golden_records(golden))
    for name, p in zip(file, golden):
        types, ids, names, pos = G.read_records(name, file, "non_pdb", "A")
        assert list(types) == p["amino_types"] and np.array_equal(ids, p["atom_amino_id"].numpy()) and np.array_equal(pos, p["atom_pos"].numpy())
        d = G.protein_to_graph(name, file, "non_pdb", "A")
        assert d.x[:, 0].tolist() == p["amino_types"] and d.x.dtype == torch.int64
        for got, want in ((d.coords_n, p["pos"][0]), (d.coords_ca, p["pos"][1]), (d.coords_c, p["pos"][2])):
            assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)) and torch.equal(torch.isnan(got), torch.isnan(want))
        for got, want in ((d.bb_embs, p["bb_embs"]), (d.side_chain_embs, p["side_chain_embs"])):
            assert torch.equal(got == 0, torch.nan_to_num(want) == 0) and torch.equal(got == 1, want == 1)
            assert float((got - torch.nan_to_num(want)).abs().max()) <= 1e-6
    with pytest.raises(KeyError):
        G.read_records("missing", file)
    bad = mapping(golden_records(golden)[:1])
    bad["P0"]["structure"]["0"]["A"]["residues"]["seq1"] = b"AB" + bad["P0"]["structure"]["0"]["A"]["residues"]["seq1"][2:]
    with pytest.raises(KeyError):                                                # 'B' is no key of res1int
        G.read_records("P0", bad)
    from src.data.utils import struct_graph_utils as U
    assert U.read_records is G.read_records and U.featurize_batch is G.featurize_batch


def test_name_codes():
    every = [n for group in G._ATOM_SETS for n in group]
    assert len(every) == 20 and max(len(n) for n in every) == 3
    codes = G.name_codes(np.array(every + [b"HD11", b"CG1xyz", b"CAx", b"NH12", b"OXT"], dtype="S"))
    assert codes.dtype == np.uint32
    for n, c in zip(every, codes[:20]):
        assert int(c) == int.from_bytes(n.ljust(4, b"\0"), "little"), n
    assert int(codes[20]) == int.from_bytes(b"HD11", "little") and int(codes[21]) == int.from_bytes(b"CG1x", "little")      # 4 bytes kept, 6 cut to 4
    assert len(set(codes.tolist())) == 25                                        # no other name falls on one of the 20
    assert np.array_equal(G.name_codes(np.array(["CA", "N"])), G.name_codes(np.array([b"CA", b"N"])))      # str names as bytes names


def test_residue_runs_for_ids_with_gaps_and_fewer_ids_than_residues():
    pos = np.arange(27, dtype=np.float64).reshape(9, 3)
    names = np.array([b"N", b"CA", b"C", b"CA", b"CA", b"CB", b"N", b"CA", b"CA"])
    a = ([0, 1, 2, 3, 4], np.array([5, 5, 5, 9, 40, 40, 41, 41]), names[:8], pos[:8])            # 4 distinct ids, 5 residues: residue 4 owns nothing
    b = ([6], np.array([-3]), names[8:], pos[8:])
    prep = G.prepare_batch([a, b])
    assert prep["res_atom_ptr"].tolist() == [0, 3, 4, 6, 8, 8, 9] and prep["graph_ptr"].tolist() == [0, 5, 6]
    assert prep["res_type"].tolist() == [0, 1, 2, 3, 4, 6] and prep["res_type"].dtype == np.uint8
    assert prep["atom_pos"].dtype == np.float32 and np.array_equal(prep["atom_pos"], pos.astype(np.float32))
    assert prep["res_atom_ptr"].dtype == prep["graph_ptr"].dtype == np.int64
    got = G.featurize_batch([a, b], device="cpu")
    assert torch.isnan(got.coords_ca[4]).all() and got.coords_ca[5].tolist() == [24.0, 25.0, 26.0]
    # a protein without any atom: every residue owns an empty run
    prep = G.prepare_batch([([1, 2], np.zeros(0, dtype=np.int64), np.zeros(0, dtype="S4"), np.zeros((0, 3))), b])
    assert prep["res_atom_ptr"].tolist() == [0, 0, 0, 1]


def test_shuffled_ids_take_the_stable_sort_and_keep_last_wins():
    gen = torch.Generator().manual_seed(5)
    types, ids, names, pos = G.synthetic_atom_records(30, gen)
    names = names.copy()
    names[np.flatnonzero(names == b"CB")[:5]] = b"CG"                            # residues with two atoms of one set: the later one must win
    perm = torch.randperm(len(ids), generator=gen).numpy()
    shuffled = (types, ids[perm], names[perm], pos[perm])
    other = G.synthetic_atom_records(7, gen)
    prep = G.prepare_batch([other, shuffled, other])
    a0, n0 = len(other[1]), len(other[0])
    _, rank = np.unique(shuffled[1], return_inverse=True)
    order = np.argsort(rank, kind="stable")
    assert np.array_equal(prep["atom_pos"][a0:a0 + len(perm)], shuffled[3][order])
    assert np.array_equal(prep["atom_name4"][a0:a0 + len(perm)], G.name_codes(shuffled[2][order]))
    assert np.array_equal(np.diff(prep["res_atom_ptr"])[n0:n0 + 30], np.bincount(rank, minlength=30))
    assert np.array_equal(prep["atom_pos"][:a0], other[3]) and np.array_equal(prep["atom_pos"][a0 + len(perm):], other[3])      # sorted proteins keep their order
    same_batch(G.featurize_batch([other, shuffled, other], device="cpu"), legacy([other, shuffled, other]))
    # the run's last atom of a set == numpy's last write
    want = G.get_atom_pos(*[shuffled[k] for k in (0, 2, 1, 3)])[4]
    ptr = prep["res_atom_ptr"][n0:n0 + 31]
    g_set = set(G.name_codes(np.array(G._ATOM_SETS[4])).tolist())
    for r in range(30):
        hits = [i for i in range(ptr[r], ptr[r + 1]) if int(prep["atom_name4"][i]) in g_set]
        if hits:
            assert np.array_equal(prep["atom_pos"][hits[-1]], want[r].numpy())
        else:
            assert torch.isnan(want[r]).all()


def test_more_ids_than_residues_raise_index_error():
    gen = torch.Generator().manual_seed(6)
    ok = G.synthetic_atom_records(5, gen)
    types, ids, names, pos = G.synthetic_atom_records(6, gen)
    over = (types[:5], ids, names, pos)
    for device in ("cpu", None):
        with pytest.raises(IndexError, match="protein 1"):
            G.featurize_batch([ok, over], device=device)
    with pytest.raises(IndexError):
        G.prepare_batch([ok, over])


def test_synthetic_atom_records_are_well_conditioned():
    gen = torch.Generator().manual_seed(9)
    n_torsions, kinds = 0, set()
    for n in (1, 2, 64, 300, 300):
        types, ids, names, pos = G.synthetic_atom_records(n, gen)
        assert types.dtype == np.uint8 and types.shape == (n,) and int(types.max()) <= 19
        assert ids.dtype == np.int64 and names.dtype == np.dtype("S4") and pos.dtype == np.float32 and pos.shape == (len(ids), 3) and names.shape == ids.shape
        assert (np.diff(ids) >= 0).all() and len(np.unique(ids)) == n
        places = torch.stack(G.get_atom_pos(types, names, ids, pos)).double().numpy()
        p0, p1, p2, p3 = G.record_torsions(places)[:4]
        cond = G.torsion_conditioning(p0, p1, p2, p3)
        real = ~np.isnan(cond)
        n_torsions += int(real.sum())
        if real.any():
            assert float(cond[real].min()) >= 0.05
        per_res = np.bincount(np.unique(ids, return_inverse=True)[1])
        kinds |= {"ca_only"} if (per_res == 1).any() else set()
        kinds |= {"bare"} if (per_res == 4).any() else set()
        if n >= 64:
            assert set(names.tolist()) >= {b"N", b"CA", b"C", b"O", b"CB", b"CG", b"CD1", b"NH1", b"OG1", b"SD"}
            assert (np.diff(np.unique(ids)) > 1).any()                            # gaps in the ids
    assert n_torsions > 2000 and kinds == {"ca_only", "bare"}


def test_header_declares_the_entry_point_and_the_binding_resolves_it():
    P, I, L64 = c_void_p, c_int, c_int64
    assert hip._SIGS["oneprot_graph_featurize"] == (I, [P] * 15 + [L64, L64, I, P])
    assert hip._PTR_DTYPES["oneprot_graph_featurize"] == "filbl" + "lfffffll" + "ll"      # atom_name4 as int32 words, res_type_bytes as bytes, the two host tables last
    assert "oneprot_graph_featurize" in hip.exported_symbols() and hip._consts["GRAPH_MAX_NODES"] == 1 << 26
    text = open(hip.HEADER_PATH).read()
    assert "src/data/utils/struct_graph_utils.py:31-144" in text
    if os.path.exists(hip.LIB_PATH):
        fn = getattr(ctypes.CDLL(hip.LIB_PATH), "oneprot_graph_featurize")
        fn.restype, fn.argtypes = hip._SIGS["oneprot_graph_featurize"]
        assert fn(*[None] * 15, 0, 1, 1, None) == -1                             # refused on the host before anything is touched
