"""Ragged MSA batches without a device: the host type oneprot_amd.packing.PackedMsa (layout, round trips, refusals, geometry tables), the ragged group
planner, the new entry points in the header and the binding, and -- in fp64 with tests/msa_ref.py alone -- the fact the feature rests on: the published
forward of an MSA's own R_b x L_b block, with the row scale of the padded row count, is the padded forward on that block."""
import math
import os
import re

import pytest
import torch

from tests import msa_ref as MR
from tests.msa_cases import _tower, _write_fair_esm_file

F64 = torch.float64
RAGGED_SYMBOLS = ("oneprot_msa_embed_ragged_fwd", "oneprot_msa_row_scores_ragged", "oneprot_msa_row_context_ragged_workspace", "oneprot_msa_row_context_ragged",
                  "oneprot_msa_row_context_ragged_dropout", "oneprot_msa_col_attn_ragged", "oneprot_msa_col_attn_ragged_dropout")


def _padded():
    """[3, 4, 9]: MSA 0 full with an interior hole and a shorter row 0; MSA 1 two rows of six columns with a hole; MSA 2 one row of three"""
    g = torch.Generator().manual_seed(0)
    t = torch.randint(4, 30, (3, 4, 9), generator=g)
    t[:, :, 0] = 0
    t[0, 0, 7:] = 1                 # row 0 shorter than the rows below it: still 9 columns (row 3 holds a token in column 8)
    t[0, 2, 4] = 1                  # an interior hole
    t[1, :, 6:] = 1
    t[1, 2:] = 1
    t[1, 1, 2] = 1
    t[2, :, 3:] = 1
    t[2, 1:] = 1
    return t


# ---------------------------------------------------------------------------------------------------------------- the host type
def test_from_padded_cuts_only_trailing_all_pad_rows_and_columns():
    from oneprot_amd.packing import PackedMsa, batch_size, PAD_MULTIPLE
    t = _padded()
    pk = PackedMsa.from_padded(t)
    assert pk.shapes == [(4, 9), (2, 6), (1, 3)] and pk.padded_shape == (4, 9) and pk.pad_id == 1
    assert len(pk) == 3 and batch_size(pk) == 3 and batch_size(t) == 3
    assert pk.cu_tokens.dtype == torch.int32 and pk.cu_tokens.tolist() == [0, 36, 48, 51]
    assert pk.T_pad == 256 and pk.T_pad % PAD_MULTIPLE == 0 and pk.n_tokens == 51
    assert pk.ids.dtype == torch.int64 and bool((pk.ids[51:] == 1).all())
    blocks = pk.unpack()
    assert torch.equal(blocks[0], t[0]) and torch.equal(blocks[1], t[1, :2, :6]) and torch.equal(blocks[2], t[2, :1, :3])
    assert int(blocks[0][2, 4]) == 1 and int(blocks[1][1, 2]) == 1 and bool((blocks[0][0, 7:] == 1).all())      # interior pads are kept
    assert torch.equal(pk.to_padded(), t)                                                                          # the round trip
    # t = cu_tokens[b] + r * L_b + l
    assert int(pk.ids[36 + 1 * 6 + 3]) == int(t[1, 1, 3])


def test_from_list_unpack_round_trip_and_padded_shape():
    from oneprot_amd.packing import PackedMsa
    g = torch.Generator().manual_seed(1)
    msas = [torch.randint(4, 30, (r, l), generator=g, dtype=torch.int32) for r, l in ((3, 7), (1, 300), (5, 2))]
    pk = PackedMsa.from_list(msas)
    assert pk.padded_shape == (5, 300) and pk.shapes == [(3, 7), (1, 300), (5, 2)] and pk.T_pad == 512 and pk.cu_tokens.tolist() == [0, 21, 321, 331]
    for a, b in zip(pk.unpack(), msas):
        assert torch.equal(a, b.long())
    x = torch.arange(pk.T_pad * 2, dtype=torch.float32).view(pk.T_pad, 2)
    views = pk.unpack(x)
    assert [tuple(v.shape) for v in views] == [(3, 7, 2), (1, 300, 2), (5, 2, 2)]
    assert views[1].data_ptr() == x[21:].data_ptr()                         # views, not copies
    assert PackedMsa.from_list(msas, padded_shape=(8, 512)).padded_shape == (8, 512)
    assert tuple(PackedMsa.from_list(msas, padded_shape=(8, 512)).to_padded().shape) == (3, 8, 512)
    moved = pk.to("cpu")
    assert moved is not pk and torch.equal(moved.ids, pk.ids) and moved.shapes == pk.shapes and moved._tables == {}


def test_refusals_of_the_type():
    from oneprot_amd import hip
    from oneprot_amd.packing import PackedMsa
    ok = torch.full((2, 4), 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="holds no token"):
        PackedMsa.from_padded(torch.stack([torch.full((2, 4), 5), torch.ones(2, 4, dtype=torch.int64)]))
    with pytest.raises(ValueError, match="holds no token"):
        PackedMsa.from_list([ok, torch.zeros(0, 4, dtype=torch.int64)])
    with pytest.raises(ValueError, match=str(hip.MSA_MAX_ROWS)):
        PackedMsa.from_list([torch.full((hip.MSA_MAX_ROWS + 1, 2), 5, dtype=torch.int64)])
    with pytest.raises(ValueError, match=str(hip.MSA_MAX_LEN)):
        PackedMsa.from_list([torch.full((1, hip.MSA_MAX_LEN + 1), 5, dtype=torch.int64)])
    with pytest.raises(ValueError, match="integers"):
        PackedMsa.from_list([ok.float()])
    with pytest.raises(ValueError, match="integers"):
        PackedMsa.from_padded(torch.full((1, 2, 4), 5.0))
    with pytest.raises(ValueError, match="smaller than the largest block"):
        PackedMsa.from_list([ok], padded_shape=(1, 4))
    with pytest.raises(ValueError, match="smaller than the largest block"):
        PackedMsa.from_list([ok], padded_shape=(2, 3))
    with pytest.raises(ValueError, match="multiple of 256"):
        PackedMsa(torch.ones(100, dtype=torch.int64), torch.tensor([0, 8], dtype=torch.int32), [(2, 4)])


def test_geometry_tables_are_cached_and_longest_first():
    from oneprot_amd.packing import PackedMsa
    pk = PackedMsa.from_padded(_padded())
    H = 2
    (g,) = pk.tables(H)
    assert pk.tables(H)[0] is g                                             # built once per batch and device
    assert (g["n"], g["b_first"], g["max_R"], g["max_L"]) == (3, 0, 4, 9)
    assert g["sum_l_lp"] == 9 * 32 + 6 * 32 + 3 * 32 and g["sum_r_lp"] == 4 * 32 + 2 * 32 + 1 * 32 and g["s_elems"] == H * (81 + 36 + 9)
    rows = g["geo"].tolist()
    assert g["geo"].dtype == torch.int64 and tuple(g["geo"].shape) == (3, 8)
    assert [r[:3] for r in rows] == [[0, 4, 9], [36, 2, 6], [48, 1, 3]] and [r[6] for r in rows] == [0, 1, 2]
    assert [r[3] for r in rows] == [0, H * 81, H * (81 + 36)]               # score maps back to back
    assert rows[0][4] == 0 and rows[0][5] == H * g["sum_l_lp"]              # P of every MSA, then every Vt
    two = pk.tables(H, [(0, 1), (1, 3)])
    assert [t["b_first"] for t in two] == [0, 1] and two[1]["geo"].tolist()[0][:3] == [36, 2, 6] and two[1]["geo"].tolist()[0][6] == 0
    # longest first whatever the stream's order
    rev = PackedMsa.from_list([m for m in reversed(pk.unpack())], padded_shape=pk.padded_shape)
    assert [r[1:3] for r in rev.tables(H)[0]["geo"].tolist()] == [[4, 9], [2, 6], [1, 3]]
    assert [r[6] for r in rev.tables(H)[0]["geo"].tolist()] == [2, 1, 0]
    assert pk.row_lens().tolist() == [9, 6, 3]
    idx, cu, n0 = pk.row0()
    assert n0 == 18 and idx.numel() == 256 and cu.tolist() == [0, 9, 15, 18] and idx[:18].tolist() == list(range(9)) + list(range(36, 42)) + [48, 49, 50]


def test_ragged_group_planner_is_pure_and_splits_under_a_tiny_budget(monkeypatch):
    from oneprot_amd.msa import plan_groups_ragged
    shapes = [(4, 9), (2, 6), (1, 3), (3, 9)]
    assert plan_groups_ragged(shapes, 2, budget=1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert plan_groups_ragged(shapes, 2, budget=1 << 30) == [(0, 4)]
    per = [4 * 2 * l * l for _, l in shapes]
    assert plan_groups_ragged(shapes, 2, budget=per[0] + per[1]) == [(0, 2), (2, 4)]
    assert plan_groups_ragged(shapes, 2, budget=per[0] + per[1]) == plan_groups_ragged(list(shapes), 2, budget=per[0] + per[1])
    monkeypatch.setenv("ONEPROT_MSA_SCORE_BYTES", "1")
    assert len(plan_groups_ragged(shapes, 2)) == 4
    monkeypatch.delenv("ONEPROT_MSA_SCORE_BYTES")
    assert plan_groups_ragged(shapes, 2) == [(0, 4)]


def test_new_symbols_are_declared_and_bound():
    from oneprot_amd import hip
    txt = re.sub(r"/\*.*?\*/", "", open(hip.HEADER_PATH).read(), flags=re.S)
    for name in RAGGED_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in hip._SIGS, name
    assert hip._PTR_DTYPES["oneprot_msa_row_scores_ragged"] == "hffl" and hip._PTR_DTYPES["oneprot_msa_embed_ragged_fwd"].startswith("lii")
    assert hip.ABI_VERSION == 7


def test_encoder_refuses_packed_tokens_and_a_cpu_packed_msa(tmp_path):
    from oneprot_amd import hip
    from oneprot_amd.packing import PackedMsa, PackedTokens
    from src.models.components.msa_encoder import MsaEncoder
    path = os.path.join(str(tmp_path), "tiny.pt")
    _write_fair_esm_file(path, _tower())
    enc = MsaEncoder(path, output_dim=32, proj_type="linear", use_all_msa=True)
    with pytest.raises(NotImplementedError, match="packed token streams"):
        enc(PackedTokens.from_padded(torch.tensor([[0, 5, 2, 1]]), pad_id=1))
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        enc(PackedMsa.from_padded(_padded()))
    with pytest.raises(ValueError, match="max_positions"):
        enc(PackedMsa.from_list([torch.full((1, 161), 5, dtype=torch.int64)]))
    with pytest.raises(ValueError, match="pad id"):
        enc(PackedMsa.from_padded(_padded().clamp(min=2), pad_id=0))


def test_synthetic_pairs_pack_the_msa_side_on_request():
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.packing import PackedMsa
    seq, mod, name, _ = next(iter(SyntheticPairs("msa", 4, 32, 48, msa_depth=5, ragged=True)))
    seq2, pk, name2, _ = next(iter(SyntheticPairs("msa", 4, 32, 48, msa_depth=5, ragged=True, packed_msa=True)))
    assert isinstance(mod, torch.Tensor) and isinstance(pk, PackedMsa) and name == name2 == "msa" and torch.equal(seq, seq2)
    assert pk.padded_shape == (5, 48) and torch.equal(pk.to_padded(), mod)


# ---------------------------------------------------------------------------------------------------------------- the fact the cut rests on, fp64
def _forward_block(tok, sd, H, R_padded):
    """MR.forward of one block [1, R_b, L_b] with the two numbers of the padded batch it was cut from: the row scale hd^-1/2 / sqrt(R_padded) (MR.row_scores
    takes R from the tensor, so its scores are rescaled by sqrt(R_b / R_padded)), and the column attention's one-row shortcut decided by R_padded."""
    Rb = tok.shape[1]
    n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    pad = tok.eq(MR.PAD)
    x = MR.embed(tok, sd)
    for i in range(n_layers):
        q, k, v = MR.qkv_proj(x, sd, i, "row_self_attention").chunk(3, dim=-1)
        S = MR.row_scores(q, k, pad, H) * (math.sqrt(Rb) / math.sqrt(R_padded))
        x = MR.attn_out(x, MR.row_context(S, v, pad, H), sd, i, "row_self_attention")
        q, k, v = MR.qkv_proj(x, sd, i, "column_self_attention").chunk(3, dim=-1)
        x = MR.attn_out(x, MR.col_context(q, k, v, pad, H, general=R_padded > 1), sd, i, "column_self_attention")
        x = MR.ffn(x, sd, i)
    return MR._ln(x, sd, "emb_layer_norm_after")


@pytest.mark.parametrize("one_row", [False, True])
def test_forward_of_a_block_with_the_padded_row_scale_is_the_padded_forward_on_that_block(one_row):
    from oneprot_amd.packing import PackedMsa
    tr = _tower()
    with torch.no_grad():
        tr.flat.normal_(0.0, 0.08)
    sd = {k: v.detach().to(F64) for k, v in tr.state_dict().items() if v.is_floating_point()}
    t = _padded()[:, :1, :].contiguous() if one_row else _padded()
    pk = PackedMsa.from_padded(t)
    full = MR.forward(t, sd, 2)
    for b, blk in enumerate(pk.unpack()):
        Rb, Lb = blk.shape
        got = _forward_block(blk[None], sd, 2, pk.padded_shape[0])[0]
        ref = full[b, :Rb, :Lb]
        live = blk.ne(1)                                                    # a padded position inside a block attends a -10000-biased row in both: compare the tokens
        err = float((got - ref)[live].abs().max())
        print(f"MSA {b} ({Rb} x {Lb} of {tuple(t.shape[1:])}): max |block - padded| = {err:.3e} of {float(ref.abs().max()):.3e}")
        assert err < 1e-9, (b, err)
