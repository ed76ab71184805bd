"""The host input path of the pocket / struct_graph modalities (oneprot_amd/graph_data.py): the featurisation against the reference's recorded
results (tests/golden/struct_graph_feats.pt, written by tests/golden/make_struct_graph_feats_golden.py), the batch type, the structure-file layout as a
nested mapping, the dataset's augmentations by their properties, and the synthetic batches."""
import builtins
import os

import numpy as np
import pytest
import torch

from oneprot_amd import graph_data as G
from oneprot_amd.data import SyntheticPairs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "struct_graph_feats.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=True)["proteins"]


def _inputs(p):
    return p["amino_types"], np.array(p["atom_names"], dtype="S"), p["atom_amino_id"].numpy(), p["atom_pos"].numpy()


def test_featurisation_equals_the_reference(golden):
    assert sorted(len(p["amino_types"]) for p in golden) == [5, 8, 12, 17, 40]
    kinds = {k for p in golden for k in p["kinds"]}
    assert {"ca_only", "full", "backbone", "no_n"} <= kinds
    assert any((np.diff(np.unique(p["atom_amino_id"].numpy())) > 1).any() for p in golden)          # ids with gaps
    for p in golden:
        pos = G.get_atom_pos(*_inputs(p))
        assert len(pos) == 9
        for got, want in zip(pos, p["pos"]):                                                         # copies of fp32 inputs: exact, NaN pattern included
            assert got.dtype == torch.float32 and torch.equal(torch.isnan(got), torch.isnan(want))
            assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
        side, bb = G.calc_side_chain_embs(*pos), G.calc_bb_embs(torch.stack(pos[:3], dim=1))
        for got, want in ((side, p["side_chain_embs"]), (bb, p["bb_embs"])):
            assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want))
            assert torch.equal(got == 0, want == 0) and torch.equal(got == 1, want == 1)             # the angle-0 structure (missing atoms, padded ends)
            assert float((torch.nan_to_num(got) - torch.nan_to_num(want)).abs().max()) <= 1e-6
        full = p["kinds"].index("full")
        assert float(side[full, 4:].abs().min()) < 1.0 and not (side[full] == torch.tensor([0.0] * 4 + [1.0] * 4)).all()      # real torsions there
        ca_only = p["kinds"].index("ca_only")
        assert torch.equal(pos[0][ca_only], pos[1][ca_only]) and torch.equal(pos[2][ca_only], pos[1][ca_only])
        assert torch.equal(side[ca_only], torch.tensor([0.0] * 4 + [1.0] * 4))


def _mapping(golden, ids=("P0", "P1", "P2")):
    """the structure file as nested dicts of numpy arrays, the reference's layout"""
    letters = "ARNDCQEGHILKMFPSTWYVX"
    out = {}
    for name, p in zip(ids, golden):
        seq = "".join(letters[a] for a in p["amino_types"])
        out[name] = {"structure": {"0": {"A": {"residues": {"seq1": seq.encode()},
                                               "polypeptide": {"atom_amino_id": p["atom_amino_id"].numpy(), "type": np.array(p["atom_names"], dtype="S"),
                                                               "xyz": p["atom_pos"].numpy()}}}}}
    return out


def test_protein_to_graph_from_a_nested_mapping(golden):
    file = _mapping(golden)
    for name, p in zip(file, golden):
        d = G.protein_to_graph(name, file, "non_pdb", "A")
        n = len(p["amino_types"])
        assert d.x.shape == (n, 1) and d.x.dtype == torch.int64 and d.x[:, 0].tolist() == p["amino_types"]
        assert d.coords_ca.shape == d.coords_n.shape == d.coords_c.shape == (n, 3) and d.bb_embs.shape == (n, 6) and d.side_chain_embs.shape == (n, 8)
        assert torch.equal(d.coords_ca, p["pos"][1]) and not torch.isnan(d.bb_embs).any() and not torch.isnan(d.side_chain_embs).any()
        assert float((d.bb_embs - torch.nan_to_num(p["bb_embs"])).abs().max()) <= 1e-6
    two = {"Q": {"structure": {"0": {"A": file["P0"]["structure"]["0"]["A"], "B": file["P1"]["structure"]["0"]["A"]}}}}
    assert 20 not in golden[0]["amino_types"] + golden[1]["amino_types"]                             # 'X' would be dropped from the sequence on these branches
    both = G.protein_to_graph("Q", two, "pdb", "all")                                                # every chain of the entry, concatenated
    assert both.num_nodes == len(golden[0]["amino_types"]) + len(golden[1]["amino_types"])
    one = G.protein_to_graph("Q", two, "pdb", "B")
    assert torch.equal(one.coords_ca, golden[1]["pos"][1])
    with pytest.raises(KeyError):
        G.protein_to_graph("missing", file)


def test_a_path_without_h5py_is_refused(monkeypatch, tmp_path):
    real = builtins.__import__

    def no_h5py(name, *a, **k):
        if name == "h5py":
            raise ImportError("No module named 'h5py'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_h5py)
    with pytest.raises(ImportError, match="h5py is not importable"):
        G.protein_to_graph("P0", str(tmp_path / "seqstruc.h5"))


def test_graph_batch_offsets_and_device_move(golden):
    file = _mapping(golden)
    parts = [G.protein_to_graph(k, file) for k in file]
    b = G.GraphBatch.from_data_list(parts)
    sizes = [p.num_nodes for p in parts]
    assert b.num_graphs == 3 and b.num_nodes == sum(sizes) and b.ptr.tolist() == [0, sizes[0], sizes[0] + sizes[1], sum(sizes)]
    assert b.batch.dtype == torch.int64 and b.batch.tolist() == [g for g, n in enumerate(sizes) for _ in range(n)]
    assert b.x.shape == (b.num_nodes, 1) and b.x.dtype == torch.int64 and b.coords_ca.dtype == torch.float32
    assert torch.equal(b.coords_n[sizes[0]:sizes[0] + sizes[1]], parts[1].coords_n) and torch.equal(b.side_chain_embs[:sizes[0]], parts[0].side_chain_embs)
    moved = b.to("cpu")
    assert moved is not b and moved.num_graphs == 3 and torch.equal(moved.bb_embs, b.bb_embs)
    with pytest.raises(ValueError):
        G.GraphBatch.from_data_list([])
    bad = G.protein_to_graph("P0", file)
    bad.x = bad.x + 30
    with pytest.raises(ValueError, match="0..25"):
        G.GraphBatch.from_data_list([bad])


def _dataset(tmp_path, golden, split, **kw):
    (tmp_path / f"{split}_seqstruc.csv").write_text("P0,x\nP1,y\nP2,z\n")
    (tmp_path / f"{split}_pocket.csv").write_text("P0,x\nP1,y\n")
    ds = G.StructDataset(str(tmp_path), split, max_length=12, **kw)
    ds.h5_file = ds.h5_file_seq = _mapping(golden)
    return ds


def test_dataset_collate_and_augmentation_properties(tmp_path, golden):
    plain = _dataset(tmp_path, golden, "train")
    assert len(plain) == 3 and plain[1] == "P1" and len(_dataset(tmp_path, golden, "val")) == 1000
    ids = ["P0", "P1", "P2"]
    seq, ref, modality, sequences = plain.collate_fn(ids)
    assert modality == "struct_graph" and len(sequences) == 3 and isinstance(ref, G.GraphBatch)
    assert seq.dtype == torch.int64 and seq.shape == (3, 12) and (seq[:, 0] == 0).all()             # <cls> ... <eos>, truncated to max_length, pad 1
    assert seq[0].tolist()[:7] == [0] + [int(t) for t in G.tokenize_sequences([sequences[0]], 64)[0, 1:6]] + [2] and (seq[0, 7:] == 1).all()
    assert plain.collate_fn(ids, return_raw_sequences=True) == sequences
    assert _dataset(tmp_path, golden, "train", pocket=True).collate_fn(ids[:2])[2] == "pocket"
    # nothing changes outside split == 'train'
    val = _dataset(tmp_path, golden, "val", use_struct_mask=True, use_struct_coord_noise=True, use_struct_deform=True).collate_fn(ids)[1]
    for k in ("x", "coords_ca", "coords_n", "coords_c", "bb_embs"):
        assert torch.equal(getattr(val, k), getattr(ref, k)), k
    torch.manual_seed(0)
    np.random.seed(0)
    # the mask writes only 20s
    masked = 0
    for _ in range(8):
        got = _dataset(tmp_path, golden, "train", use_struct_mask=True).collate_fn(ids)[1]
        changed = got.x != ref.x
        assert (got.x[changed] == 20).all() and torch.equal(got.coords_ca, ref.coords_ca)
        masked += int(changed.sum())
    assert masked > 0
    # coordinate noise: N(0, 0.1) clipped to +-0.3, independently on CA / N / C
    got = _dataset(tmp_path, golden, "train", use_struct_coord_noise=True).collate_fn(ids)[1]
    deltas = [getattr(got, k) - getattr(ref, k) for k in ("coords_ca", "coords_n", "coords_c")]
    for d in deltas:
        assert float(d.abs().max()) <= 0.3 + 1e-5 and 0.05 < float(d.std()) < 0.15
    assert not torch.equal(deltas[0], deltas[1]) and torch.equal(got.x, ref.x)
    # deform: one [1, 3] scale per atom type in [0.9, 1.1]
    got = _dataset(tmp_path, golden, "train", use_struct_deform=True).collate_fn(ids)[1]
    for k in ("coords_ca", "coords_n", "coords_c"):
        a, b = getattr(got, k), getattr(ref, k)
        big = b.abs() > 1.0
        ratio = torch.where(big, a / b, torch.nan)
        lo, hi = np.nanmin(ratio.numpy(), axis=0), np.nanmax(ratio.numpy(), axis=0)
        assert (hi - lo < 1e-5).all() and (lo >= 0.9 - 1e-5).all() and (hi <= 1.1 + 1e-5).all()    # one factor per axis, inside the clip


def test_augment_clips_hold_at_the_extremes():
    """a generator stub that returns the extremes shows the clips themselves: noise beyond +-0.3 and scales beyond [0.9, 1.1] never reach the batch"""
    gen = torch.Generator().manual_seed(1)
    parts = [G.synthetic_protein(500, gen) for _ in range(4)]
    ref = G.GraphBatch.from_data_list(parts)
    got = G.augment_struct_batch(ref.clone(), False, True, False, generator=gen)
    d = got.coords_ca - ref.coords_ca
    assert float(d.abs().max()) <= 0.3 + 1e-5 and int((d.abs() >= 0.3 - 1e-5).sum()) > 0             # 6000 draws at 3 sigma: some sit on the clip
    got = G.augment_struct_batch(ref.clone(), True, False, False, rng=np.random.default_rng(3))
    assert set(got.x[got.x != ref.x].tolist()) <= {20}


def test_synthetic_pairs_yield_graph_batches():
    for modality in ("pocket", "struct_graph"):
        batches = list(SyntheticPairs(modality, 4, 16, 40, n_batches=2, ragged=True))
        again = list(SyntheticPairs(modality, 4, 16, 40, n_batches=2, ragged=True))
        assert len(batches) == 2
        for (seq, gb, name, raw), (_, gb2, _, _) in zip(batches, again):
            assert name == modality and raw is None and seq.shape == (4, 16) and isinstance(gb, G.GraphBatch) and gb.num_graphs == 4
            assert torch.equal(gb.coords_ca, gb2.coords_ca)                                          # seeded
            sizes = gb.ptr.diff().tolist()
            assert all(10 <= n <= 40 for n in sizes) and gb.bb_embs.shape == (gb.num_nodes, 6)
            ca, ptr = gb.coords_ca, gb.ptr.tolist()
            for a, b in zip(ptr[:-1], ptr[1:]):
                steps = (ca[a + 1:b] - ca[a:b - 1]).norm(dim=-1)
                assert float((steps - 3.8).abs().max()) < 1e-4
                assert float(((gb.coords_n[a:b] - ca[a:b]).norm(dim=-1) - 1.46).abs().max()) < 1e-4
                assert float(((gb.coords_c[a:b] - ca[a:b]).norm(dim=-1) - 1.52).abs().max()) < 1e-4
            assert int(gb.x.min()) >= 0 and int(gb.x.max()) <= 19 and not torch.isnan(gb.bb_embs).any()
    assert torch.equal(G.calc_bb_embs(torch.stack((gb.coords_n[:ptr[1]], ca[:ptr[1]], gb.coords_c[:ptr[1]]), dim=1)), gb.bb_embs[:ptr[1]])
