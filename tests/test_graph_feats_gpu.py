"""The batch featurisation of the pocket / struct_graph modalities on the device (csrc/graph_feats.hip through oneprot_amd.graph_data.featurize_batch)
against the pinned host functions, the reference's recorded results (tests/golden/struct_graph_feats.pt) and an fp64 restatement written here.

The gate of the features is not fixed in advance.  For every set of inputs, E is the largest error of the pinned HOST fp32 path against the fp64
restatement on the same fp32-rounded inputs, and the device is held to atol = max(4 E, 1e-6), rtol = 0: two fp32 evaluations of one formula each lie
within about E of fp64, hence within 2 E of each other; the other factor of 2 covers another libm.  No element is left out.  Every E and every device
error is printed before its assertion (-s).  Coordinates, x, batch and ptr are copies and must be exact."""
import os

import numpy as np
import pytest
import torch

from oneprot_amd import graph_data as G
from oneprot_amd import hip
from tests.gate import close, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "struct_graph_feats.pt")
LETTERS = "ARNDCQEGHILKMFPSTWYVX"
EXACT = ("x", "coords_ca", "coords_n", "coords_c", "batch", "ptr")
ANGLE0 = torch.tensor([0.0] * 4 + [1.0] * 4)


# ---- the fp64 restatement of get_atom_pos, compute_diherals, calc_side_chain_embs, calc_bb_embs ---------------------------------------------------------
def places64(record):
    """float64 [9, n, 3] from the fp32-rounded atom positions: per place the last atom of the residue (rank of its id) whose name is in the set"""
    types, ids, names, pos = record
    names = [bytes(a) if isinstance(a, (bytes, np.bytes_)) else str(a).encode() for a in np.asarray(names).tolist()]
    pos = np.asarray(pos).astype(np.float32).astype(np.float64).reshape(-1, 3)
    rank = {v: k for k, v in enumerate(sorted(set(np.asarray(ids).tolist())))}
    out = np.full((9, len(types), 3), np.nan)
    for i, (name, rid) in enumerate(zip(names, np.asarray(ids).tolist())):
        for k, group in enumerate(G._ATOM_SETS):
            if name in group:
                out[k, rank[rid]] = pos[i]
    for k in (0, 2):
        out[k] = np.where(np.isnan(out[k]), out[1], out[k])
    return out


def dihedral64(v1, v2, v3):
    with np.errstate(invalid="ignore", divide="ignore"):
        n1, n2 = np.cross(v1, v2), np.cross(v2, v3)
        a = (n1 * n2).sum(-1) + 0.0                                      # torch's sums start from +0: three -0 give +0, and atan2(0, +0) is 0 where atan2(0, -0) is pi
        b = np.nan_to_num((np.cross(n1, n2) * v2).sum(-1) / np.sqrt((v2 * v2).sum(-1)))
        return np.nan_to_num(np.arctan2(b, a))


def feats64(record):
    """(bb [n, 6], side [n, 8]) in float64"""
    p = places64(record)
    n = p.shape[1]
    chain = [p[k] for k in (0, 1, 3, 4, 5, 6, 7)]
    v = [b - a for a, b in zip(chain[:-1], chain[1:])]
    ang = np.stack([dihedral64(v[k], v[k + 1], v[k + 2]) for k in range(4)], 1)
    side = np.concatenate([np.sin(ang), np.cos(ang)], 1)
    X = np.stack([p[0], p[1], p[2]], 1).reshape(3 * n, 3)
    d = X[1:] - X[:-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        U = np.nan_to_num(d / np.sqrt((d * d).sum(-1, keepdims=True)))
    a = np.zeros(3 * n)
    a[1:3 * n - 2] = dihedral64(U[:-2], U[1:-1], U[2:])
    a = a.reshape(n, 3)
    return np.concatenate([np.cos(a), np.sin(a)], 1), side


def gate_of(records, label):
    """(bb64, side64, atol, host batch): the restatement over the batch, the gate max(4 E, 1e-6) from the host path's own error, the host batch"""
    host = G.featurize_batch(records, device="cpu")
    parts = [feats64(r) for r in records]
    bb, side = (torch.from_numpy(np.concatenate([p[k] for p in parts])) for k in (0, 1))
    E = max(float((host.bb_embs.double() - bb).abs().max()), float((host.side_chain_embs.double() - side).abs().max()))
    print(f"{label}: E (host fp32 vs fp64) = {E:.3e}, gate atol = {max(4 * E, 1e-6):.3e}")
    return bb, side, max(4 * E, 1e-6), host


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b, msg=""):
    for k in EXACT + ("bb_embs", "side_chain_embs"):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), f"{msg} {k}"


def check_against_host(records, label):
    """the device batch against the host batch of the same records: copies exact (NaN pattern included), features inside the gate, the angle-0 pattern equal"""
    bb, side, atol, host = gate_of(records, label)
    got = G.featurize_batch(records, device=DEV)
    assert got.num_graphs == host.num_graphs
    for k in EXACT:
        a, b = getattr(got, k).cpu(), getattr(host, k)
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), f"{label} {k}"
    for k, ref in (("bb_embs", bb), ("side_chain_embs", side)):
        g, h = getattr(got, k).cpu(), getattr(host, k)
        assert g.dtype == torch.float32 and g.shape == h.shape
        print(f"{label} {k}: device vs fp64 {close(g, ref, 0, atol, f'{label} {k} vs fp64'):.3e}, device vs host {close(g, h, 0, atol, f'{label} {k} vs host'):.3e}")
        exact = (ref == 0) | (ref == 1)                                  # the restatement is exact only where the nan_to_num chain made the angle 0
        assert torch.equal(g[exact].double(), ref[exact]) and torch.equal(h[exact].double(), ref[exact]), f"{label} {k}: angle 0 is not exactly (0, 1)"
    return got, host, atol


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=True)["proteins"]


def golden_records(golden):
    return [(p["amino_types"], p["atom_amino_id"].numpy(), np.array(p["atom_names"], dtype="S"), p["atom_pos"].numpy()) for p in golden]


def mapping(records):
    return {f"P{k}": {"structure": {"0": {"A": {"residues": {"seq1": "".join(LETTERS[a] for a in r[0]).encode()},
                                                "polypeptide": {"atom_amino_id": r[1], "type": r[2], "xyz": r[3]}}}}} for k, r in enumerate(records)}


def test_golden_proteins_as_one_batch(golden):
    records = golden_records(golden)
    got, host, atol = check_against_host(records, "golden")
    sizes = [len(p["amino_types"]) for p in golden]
    assert got.ptr.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist() and got.batch.tolist() == [g for g, n in enumerate(sizes) for _ in range(n)]
    assert got.x[:, 0].tolist() == [a for p in golden for a in p["amino_types"]] and got.x.shape == (sum(sizes), 1)
    for k, name in enumerate(("coords_n", "coords_ca", "coords_c")):                                       # the recorded pos_n, pos_ca, pos_c: bit-equal
        want = torch.cat([p["pos"][k] for p in golden])
        g = getattr(got, name).cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(want)) and torch.equal(bits(torch.nan_to_num(g)), bits(torch.nan_to_num(want))), name
    for name in ("bb_embs", "side_chain_embs"):
        want = torch.nan_to_num(torch.cat([p[name] for p in golden]))
        g = getattr(got, name).cpu()
        print(f"golden {name}: device vs recorded {close(g, want, 0, atol, name):.3e}")
    want = torch.cat([p["side_chain_embs"] for p in golden])
    zero = (want[:, :4] == 0) & (want[:, 4:] == 1)                                                         # recorded angle exactly 0 -> exactly (0, 1)
    g = got.side_chain_embs.cpu()
    assert int(zero.sum()) > 50 and (g[:, :4][zero] == 0).all() and (g[:, 4:][zero] == 1).all()
    want = torch.cat([p["bb_embs"] for p in golden])
    zero = (want[:, :3] == 1) & (want[:, 3:] == 0)
    g = got.bb_embs.cpu()
    assert int(zero.sum()) >= 3 * len(golden) and (g[:, :3][zero] == 1).all() and (g[:, 3:][zero] == 0).all()


def test_graph_boundaries_alone_in_the_batch_and_reversed():
    gen = torch.Generator().manual_seed(23)
    sizes = (1, 2, 3, 63, 64, 65, 257)                                                                     # across a wave, across a work-group, a single residue
    records = [G.synthetic_atom_records(n, gen) for n in sizes]
    got, _, _ = check_against_host(records, "boundaries")
    ptr = got.ptr.tolist()
    bb = got.bb_embs.cpu()
    for a, b in zip(ptr[:-1], ptr[1:]):
        assert bb[a, 0] == 1 and bb[a, 3] == 0, "phi of a protein's first residue is angle 0"
        assert bb[b - 1, 1] == 1 and bb[b - 1, 2] == 1 and bb[b - 1, 4] == 0 and bb[b - 1, 5] == 0, "psi and omega of its last residue are angle 0"
    back = G.featurize_batch(records[::-1], device=DEV)
    rptr = back.ptr.tolist()
    for g, r in enumerate(records):
        alone = G.featurize_batch([r], device=DEV)
        rg = len(records) - 1 - g
        for k in ("x", "coords_ca", "coords_n", "coords_c", "bb_embs", "side_chain_embs"):
            assert torch.equal(bits(getattr(alone, k)), bits(getattr(got, k)[ptr[g]:ptr[g + 1]])), f"protein {g} alone vs in the batch: {k}"
            assert torch.equal(bits(getattr(alone, k)), bits(getattr(back, k)[rptr[rg]:rptr[rg + 1]])), f"protein {g} alone vs in the reversed batch: {k}"
        assert alone.ptr.tolist() == [0, sizes[g]] and not alone.batch.any()


def _odd_records():
    gen = torch.Generator().manual_seed(31)
    rnd = lambda *s: torch.randn(*s, generator=gen).numpy() * 3.0      # noqa: E731
    # a residue of 130 atoms with three CG (the last one wins) between two ordinary ones
    types, ids, names, pos = G.synthetic_atom_records(3, gen)
    mid = int(np.unique(ids)[1])
    keep = ids != mid
    big_names = [b"N", b"CA", b"C", b"O", b"CB", b"CG"] + [b"HX%d" % k for k in range(60)] + [b"CG", b"CD"] + [b"HY%d" % k for k in range(59)] + [b"CG", b"CE", b"NZ"]
    assert len(big_names) == 130
    first = int(np.flatnonzero(~keep)[0])
    big = (types,
           np.concatenate([ids[:first], np.full(130, mid), ids[keep][first:]]),
           np.concatenate([names[:first], np.array(big_names, dtype="S4"), names[keep][first:]]),
           np.concatenate([pos[:first], pos[first] + rnd(130, 3), pos[keep][first:]]).astype(np.float32))
    no_atom = (np.array([3], dtype=np.uint8), np.zeros(0, dtype=np.int64), np.zeros(0, dtype="S4"), np.zeros((0, 3), dtype=np.float32))      # one residue, no atom at all
    t5 = G.synthetic_atom_records(5, gen)
    tail = (np.concatenate([t5[0], [7, 9]]).astype(np.uint8),) + t5[1:]                                    # the last two residues own no atom
    # a residue whose atoms are all of no set (its places are all NaN) and one with N and C missing, which take CA
    t4 = G.synthetic_atom_records(4, gen)
    u = np.unique(t4[1])
    n4 = t4[2].copy()
    n4[t4[1] == u[1]] = b"H"
    sel = (t4[1] == u[2]) & np.isin(n4, [b"N", b"C"])
    no_nc = (t4[0], t4[1][~sel], n4[~sel], t4[3][~sel])
    t40 = G.synthetic_atom_records(40, gen)
    perm = torch.randperm(len(t40[1]), generator=gen).numpy()
    shuffled = (t40[0], t40[1][perm], t40[2][perm], t40[3][perm])                                          # the stable-sort fallback
    return [big, no_atom, tail, no_nc, shuffled]


def test_runs_of_atoms_against_the_host_path():
    records = _odd_records()
    got, host, _ = check_against_host(records, "runs")
    ptr = host.ptr.tolist()
    big = records[0]
    cg = np.flatnonzero((big[2] == b"CG") & (big[1] == np.unique(big[1])[1]))
    assert len(cg) == 3 and int((big[1] == np.unique(big[1])[1]).sum()) == 130
    places = G.get_atom_pos(big[0], big[2], big[1], big[3])
    assert torch.equal(places[4][1], torch.from_numpy(big[3][cg[-1]]))                                     # the host's last write is the third CG ...
    assert torch.isnan(got.coords_ca[ptr[1]]).all() and torch.equal(got.side_chain_embs[ptr[1]].cpu(), ANGLE0)      # the residue without atoms
    assert torch.isnan(got.coords_ca[ptr[3] - 2:ptr[3]]).all() and not torch.isnan(got.coords_ca[ptr[2]:ptr[3] - 2]).any()
    assert torch.isnan(got.coords_ca[ptr[3] + 1]).all()                                                    # atoms, none of a set
    r = ptr[3] + 2
    assert torch.equal(got.coords_n[r], got.coords_ca[r]) and torch.equal(got.coords_c[r], got.coords_ca[r]) and not torch.isnan(got.coords_ca[r]).any()
    # ... and decides the device's torsions: with the first CG instead, the host's own side chain row is another one
    moved = (big[0], big[1], big[2].copy(), big[3])
    moved[2][cg[1:]] = b"HZ"
    other = G.featurize_batch([moved], device="cpu").side_chain_embs[1]
    assert float((other - host.side_chain_embs[1]).abs().max()) > 1e-2


@pytest.mark.parametrize("shift", [0.0, 150.0])
def test_accuracy_against_fp64(shift):
    gen = torch.Generator().manual_seed(41)
    records = [G.synthetic_atom_records(300, gen) for _ in range(4)]
    records = [(t, i, n, (p + np.float32(shift)).astype(np.float32)) for t, i, n, p in records]
    check_against_host(records, f"accuracy shift {shift:g}")


def test_two_calls_give_the_same_bits():
    gen = torch.Generator().manual_seed(43)
    records = [G.synthetic_atom_records(n, gen) for n in (70, 1, 300)]
    a, b = G.featurize_batch(records, device=DEV), G.featurize_batch(records, device=DEV)
    same_bits(a, b, "second call")
    assert a.coords_ca.data_ptr() != b.coords_ca.data_ptr() and a.x.device == torch.device(DEV)


def _dataset(tmp_path, file, device, **kw):
    (tmp_path / "train_seqstruc.csv").write_text("".join(f"{k},x\n" for k in file))
    ds = G.StructDataset(str(tmp_path), "train", max_length=48, **kw)
    ds.h5_file = ds.h5_file_seq = file
    ds.device = device
    return ds


def test_dataset_on_the_device_equals_the_host_dataset(tmp_path, golden):
    gen = torch.Generator().manual_seed(47)
    records = golden_records(golden)[:3] + [G.synthetic_atom_records(n, gen) for n in (30, 64)]
    file = mapping(records)
    ids = list(file) + ["absent"]                                                                           # the per-id KeyError skip stays
    _, _, atol, _ = gate_of(records, "dataset")
    for kw in ({}, dict(use_struct_mask=True, use_struct_coord_noise=True, use_struct_deform=True)):
        out = []
        for device in (None, DEV):
            np.random.seed(3)
            torch.manual_seed(3)
            out.append(_dataset(tmp_path, file, device, **kw).collate_fn(ids))
        (seq_h, host, mod_h, raw_h), (seq_d, got, mod_d, raw_d) = out
        assert mod_h == mod_d == "struct_graph" and raw_h == raw_d and len(raw_d) == 5
        assert seq_d.device == torch.device(DEV) and torch.equal(seq_d.cpu(), seq_h) and isinstance(got, G.GraphBatch) and got.num_graphs == 5
        for k in EXACT:
            a, b = getattr(got, k), getattr(host, k)
            assert a.device == torch.device(DEV) and torch.equal(torch.isnan(a.cpu()), torch.isnan(b)) and torch.equal(torch.nan_to_num(a.cpu()), torch.nan_to_num(b)), (kw, k)
        for k in ("bb_embs", "side_chain_embs"):
            close(getattr(got, k).cpu(), getattr(host, k), 0, atol, f"dataset {k}")
        if kw:
            plain = G.featurize_batch(records, device="cpu")
            assert int((host.x != plain.x).sum()) > 0 and not torch.equal(torch.nan_to_num(host.coords_ca), torch.nan_to_num(plain.coords_ca))      # the augmentations did act
    assert _dataset(tmp_path, file, DEV).collate_fn(ids, return_raw_sequences=True) == raw_h


def _raw_call(fn, tensors, host_res, host_graph, A, N, Gn):
    return fn(*[None if t is None else t.data_ptr() for t in tensors], host_res.ctypes.data if host_res is not None else None,
              host_graph.ctypes.data if host_graph is not None else None, A, N, Gn, torch.cuda.current_stream().cuda_stream)


def test_refusals_launch_nothing():
    with pytest.raises(ValueError):
        G.featurize_batch([], device=DEV)
    fn = getattr(hip.lib(), "oneprot_graph_featurize")
    gen = torch.Generator().manual_seed(53)
    prep = G.prepare_batch([G.synthetic_atom_records(n, gen) for n in (6, 9)])
    A, N, Gn = len(prep["atom_name4"]), 15, 2
    ins = [torch.from_numpy(prep["atom_pos"]).to(DEV), torch.from_numpy(prep["atom_name4"].view(np.int32)).to(DEV), torch.from_numpy(prep["res_atom_ptr"]).to(DEV),
           torch.from_numpy(prep["res_type"]).to(DEV), torch.from_numpy(prep["graph_ptr"]).to(DEV)]
    outs = [torch.full(s, -7, dtype=d, device=DEV) for s, d in (((N, 1), torch.int64), ((N, 3), torch.float32), ((N, 3), torch.float32), ((N, 3), torch.float32),
                                                                  ((N, 6), torch.float32), ((N, 8), torch.float32), ((N,), torch.int64), ((Gn + 1,), torch.int64))]
    res, graph = prep["res_atom_ptr"], prep["graph_ptr"]

    def changed(table, at, value):
        t = table.copy()
        t[at] = value
        return t
    bad = [(res, graph, A, 0, Gn), (res, graph, A, N, 0), (res, graph, A, N, -1),
           (changed(res, 4, res[3] - 1), graph, A, N, Gn),                                                 # decreases
           (changed(res, N, A - 1), graph, A, N, Gn), (changed(res, N, A + 1), graph, A, N, Gn),           # does not end at A
           (changed(res, 0, -1), graph, A, N, Gn),                                                         # leaves its range
           (res, changed(graph, 1, N + 1), A, N, Gn), (res, changed(graph, 2, N - 1), A, N, Gn),           # decreases / does not end at N
           (res, changed(graph, 0, 1), A, N, Gn), (res, graph, A + 1, N, Gn), (res, graph, A, N + 1, Gn)]
    for case in bad:
        assert _raw_call(fn, ins + outs, *case) == -1, case[2:]
    for k in range(13):
        tensors = list(ins + outs)
        tensors[k] = None
        assert _raw_call(fn, tensors, res, graph, A, N, Gn) == -1, f"NULL pointer {k}"
    assert _raw_call(fn, ins + outs, None, graph, A, N, Gn) == -1 and _raw_call(fn, ins + outs, res, None, A, N, Gn) == -1
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs), "a refused call wrote something"
    assert _raw_call(fn, ins + outs, res, graph, A, N, Gn) == 0                                            # the same arguments, untouched, are accepted
    torch.cuda.synchronize()
    assert outs[7].tolist() == graph.tolist() and not bool((outs[0] == -7).any())


def test_device_batch_through_the_tower_forward_and_backward():
    from oneprot_amd import pronet as P
    from tests import pronet_ref as R
    gen = torch.Generator().manual_seed(59)
    records = [G.synthetic_atom_records(n, gen) for n in (1, 2, 33, 70)]
    host = G.featurize_batch(records, device="cpu")
    got = G.featurize_batch(records, device=DEV)
    torch.manual_seed(21)
    tower = P.ProNet(level="backbone", num_blocks=2, hidden_channels=64, out_channels=8).to(DEV).eval()      # the smallest built width
    cfg = dict(num_blocks=2, num_radial=6, num_pos_emb=16, cutoff=10.0, max_num_neighbors=32, int_emb_layers=3, out_layers=2)
    cot = torch.randn(4, 8, generator=gen)
    sd = {k: v.detach().cpu() for k, v in tower.state_dict().items()}

    def restated(dtype):
        p = {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items()}
        out = R.forward(p, host, dtype=dtype, aug=None, **cfg)
        (out * cot.to(dtype)).sum().backward()
        return {"output": out.detach(), **{k: v.grad for k, v in p.items()}}

    def run(batch):
        tower.zero_grad(set_to_none=True)
        out = tower(batch)
        (out * cot.to(DEV)).sum().backward()
        return {"output": out.detach(), **{k: v.grad.clone() for k, v in tower.named_parameters()}}
    r64, r32 = restated(torch.float64), restated(torch.float32)
    a, b = run(got), run(host.to(DEV))
    assert set(a) == set(r64) and a["output"].shape == (4, 8)
    worst = 0.0
    for k in r64:                                                                                          # tests/test_pronet_gpu.py's rule: 4 x the fp32 restatement's own error, per tensor
        e32, e = rel_l2(r32[k], r64[k]), rel_l2(a[k], b[k])
        worst = max(worst, e / max(e32, 1e-30))
        assert e <= 4.0 * e32, f"{k}: device-path batch vs host-path batch {e:.3e}, fp32 restatement vs fp64 {e32:.3e}"
    print(f"tower: worst (device-path vs host-path batch) / (fp32 restatement's error) over {len(r64)} tensors: {worst:.3f}")
