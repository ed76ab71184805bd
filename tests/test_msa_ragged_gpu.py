"""Ragged MSA batches on the GPU: the seven oneprot_msa_*_ragged entry points and the tower / encoder / module on a PackedMsa.

Each ragged call is checked twice on a stream cut from a padded batch: against the fp64 restatement tests/msa_ref.py of the PADDED batch, sliced to the
block, at the tolerances of tests/test_msa_gpu.py (fp32 rtol 1e-4, atol 1e-3 * sqrt(R) for the scores; bf16 rtol 2^-7, atol 2e-2; the embedding 1e-5), and
bit for bit against its padded twin run on that padded batch with the same inputs and the same scale.  A NaN or Inf anywhere fails, tail rows included.
The fp64 references run on the device too (MR is plain torch) and are computed once per stream."""
import functools
import math
import os
import warnings

import pytest
import torch

from tests import msa_ref as MR
from tests.gate import close
from tests.msa_cases import ARCH, DEV, F64, _checkpoint, _ids, _key_bias, _tokens

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- helpers
def _index(pk):
    """(flat positions of the padded batch, stream rows) of every position of every block"""
    R, L = pk.padded_shape
    c, pi, si = pk.offsets(), [], []
    for b, (rb, lb) in enumerate(pk.shapes):
        r, l = torch.meshgrid(torch.arange(rb), torch.arange(lb), indexing="ij")
        pi.append(((b * R + r) * L + l).reshape(-1))
        si.append((c[b] + r * lb + l).reshape(-1))
    return torch.cat(pi), torch.cat(si)


def _to_stream(pk, padded_rows, fill=0.0):
    """rows of a padded [B * R * L, ...] tensor at the blocks' positions -> the stream [T_pad, ...]"""
    pi, si = _index(pk)
    out = torch.full((pk.T_pad,) + tuple(padded_rows.shape[1:]), fill, dtype=padded_rows.dtype, device=padded_rows.device)
    out[si.to(padded_rows.device)] = padded_rows[pi.to(padded_rows.device)]
    return out


def _row_padded(qkv, ids, H, scale, drop=None):
    """the padded twins on the padded batch: S [B, H, L, L], ctx [B, R, L, H * 64]; drop = (b_first, p, seed, stream id)"""
    from oneprot_amd import hip
    B, R, L = ids.shape
    kb = _key_bias(ids)
    S = torch.empty(B, H, L, L, dtype=torch.float32, device=DEV)
    ctx = torch.empty(B * R * L, H * 64, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_msa_row_scores", qkv, kb, S, B, R, L, H, 64, scale)
    ws = torch.empty(hip.query("oneprot_msa_row_context_workspace", B, R, L, H), dtype=torch.uint8, device=DEV)
    if drop is None:
        hip.call("oneprot_msa_row_context", S, qkv, kb, ctx, ws, ws.numel(), B, R, L, H, 64)
    else:
        hip.call("oneprot_msa_row_context_dropout", S, qkv, kb, ctx, ws, ws.numel(), B, R, L, H, 64, *drop)
    torch.cuda.synchronize()
    return S, ctx.view(B, R, L, H * 64)


def _row_ragged(pk, qkv, H, scale, groups=None, drop=None, b_off=0):
    """the ragged calls on the stream, group by group -> (per-MSA S [H, L_b, L_b] clones, ctx stream [T_pad, H * 64])"""
    from oneprot_amd import hip
    kb = torch.empty(pk.T_pad, dtype=torch.float32, device=DEV)
    hip.call("oneprot_key_padding_bias", pk.ids, kb, pk.T_pad, pk.pad_id)
    ctx = torch.full((pk.T_pad, H * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    S_of = [None] * len(pk)
    for g in pk.tables(H, groups):
        S = torch.full((g["s_elems"],), float("nan"), dtype=torch.float32, device=DEV)
        ws = torch.empty(hip.query("oneprot_msa_row_context_ragged_workspace", g["sum_l_lp"], g["sum_r_lp"], H), dtype=torch.uint8, device=DEV)
        assert ws.numel() == 2 * H * (g["sum_l_lp"] + 64 * g["sum_r_lp"])
        hip.call("oneprot_msa_row_scores_ragged", qkv, kb, S, g["geo"], g["n"], g["max_L"], H, 64, scale)
        geom = (g["geo"], g["n"], g["max_R"], g["max_L"], g["sum_l_lp"], g["sum_r_lp"], H, 64, pk.n_tokens, pk.T_pad)
        if drop is None:
            hip.call("oneprot_msa_row_context_ragged", S, qkv, kb, ctx, ws, ws.numel(), *geom)
        else:
            hip.call("oneprot_msa_row_context_ragged_dropout", S, qkv, kb, ctx, ws, ws.numel(), *geom, b_off + g["b_first"], *drop)
        torch.cuda.synchronize()
        for row in g["geo"].tolist():
            l = row[2]
            S_of[g["b_first"] + row[6]] = S[row[3]:row[3] + H * l * l].view(H, l, l).clone()
    return S_of, ctx


def _col_ragged(pk, qkv, H, drop=None):
    from oneprot_amd import hip
    kb = torch.empty(pk.T_pad, dtype=torch.float32, device=DEV)
    hip.call("oneprot_key_padding_bias", pk.ids, kb, pk.T_pad, pk.pad_id)
    ctx = torch.full((pk.T_pad, H * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    (g,) = pk.tables(H)
    geom = (g["geo"], g["n"], g["max_R"], g["max_L"], H, 64, 64 ** -0.5, pk.n_tokens, pk.T_pad)
    if drop is None:
        hip.call("oneprot_msa_col_attn_ragged", qkv, kb, ctx, *geom)
    else:
        hip.call("oneprot_msa_col_attn_ragged_dropout", qkv, kb, ctx, *geom, pk.padded_shape[1], *drop)
    torch.cuda.synchronize()
    return ctx


def _col_padded(qkv, ids, H, drop=None):
    from oneprot_amd import hip
    B, R, L = ids.shape
    ctx = torch.empty(B * R * L, H * 64, dtype=torch.bfloat16, device=DEV)
    if drop is None:
        hip.call("oneprot_msa_col_attn", qkv, _key_bias(ids), ctx, B, R, L, H, 64, 64 ** -0.5)
    else:
        hip.call("oneprot_msa_col_attn_dropout", qkv, _key_bias(ids), ctx, B, R, L, H, 64, 64 ** -0.5, *drop)
    torch.cuda.synchronize()
    return ctx.view(B, R, L, H * 64)


def _tail_is_zero(pk, ctx):
    assert torch.isfinite(ctx[:pk.n_tokens].float()).all(), "non-finite ctx inside the blocks"
    assert bool((ctx[pk.n_tokens:] == 0).all()), "tail rows of ctx are not 0"


# ---------------------------------------------------------------------------------------------------------------- row attention
ROW_BLOCKS = [(1, 5), (3, 33), (2, 20), (50, 70), (5, 130), (3, 97), (2, 257)]
ROW_HOLES = ((1, 2, 7),) + tuple((3, 0, l) for l in (66, 67, 68, 69))       # a hole at (r = 2, l = 7) of MSA 1; row 0 of MSA 3 shorter than its other rows


@functools.lru_cache(maxsize=None)
def _row_stream(which):
    """(padded ids, PackedMsa on the device, padded qkv bf16 on the device, H, scale, padded-twin S and ctx, fp64 S and ctx) -- computed once"""
    from oneprot_amd.packing import PackedMsa
    blocks, H, holes = (ROW_BLOCKS, 2, ROW_HOLES) if which == "mixed" else ([(3, 1024)], 1, ())
    B, R, L = len(blocks), max(r for r, _ in blocks), max(l for _, l in blocks)
    ids = _ids(B, R, L, [l for _, l in blocks], [r for r, _ in blocks], holes)
    pk = PackedMsa.from_padded(ids).to(DEV)
    assert pk.shapes == blocks and pk.padded_shape == (R, L)
    g = torch.Generator().manual_seed(77 + L)
    qkv = torch.randn(B * R * L, 3 * H * 64, generator=g).to(torch.bfloat16).to(DEV)
    scale = 64 ** -0.5 / math.sqrt(R)                                       # the padded row count
    S_pad, ctx_pad = _row_padded(qkv, ids, H, scale)
    q, k, v = qkv.to(F64).view(B, R, L, 3, H * 64).unbind(3)
    pad = ids.eq(1).to(DEV)
    S64 = MR.row_scores(q, k, pad, H)
    c64 = MR.row_context(S64, v, pad, H)
    return ids, pk, qkv, H, scale, S_pad, ctx_pad, S64, c64


def _check_row(pk, S_of, ctx, ref, order=None, fp64=True):
    """per MSA: S and ctx against fp64 (sliced to the block) and bit-equal to the padded twin; order[i] = the padded batch's MSA behind stream MSA i"""
    ids, pk0, _, H, _, S_pad, ctx_pad, S64, c64 = ref
    R = pk0.padded_shape[0]
    _tail_is_zero(pk, ctx)
    for i, blk in enumerate(pk.unpack(ctx)):
        b = i if order is None else order[i]
        rb, lb = pk.shapes[i]
        assert torch.isfinite(S_of[i]).all()
        assert torch.equal(S_of[i], S_pad[b, :, :lb, :lb]), f"S of MSA {b} {rb}x{lb} differs from the padded kernel's"
        assert torch.equal(blk, ctx_pad[b, :rb, :lb]), f"row ctx of MSA {b} {rb}x{lb} differs from the padded kernel's"
        if fp64:
            close(S_of[i], S64[b, :, :lb, :lb], 1e-4, 1e-3 * math.sqrt(R), f"ragged S, MSA {b} {rb}x{lb}")
            close(blk, c64[b, :rb, :lb], 2 ** -7, 2e-2, f"ragged row ctx, MSA {b} {rb}x{lb}")


@pytest.mark.parametrize("which", ["mixed", "L1024"])
def test_row_attention_ragged_vs_fp64_and_bit_equal_to_padded(which):
    ref = _row_stream(which)
    _, pk, qkv, H, scale = ref[:5]
    S_of, ctx = _row_ragged(pk, _to_stream(pk, qkv), H, scale)
    _check_row(pk, S_of, ctx, ref)


def test_row_attention_ragged_in_any_order_and_under_grouping():
    from oneprot_amd.msa import plan_groups_ragged
    from oneprot_amd.packing import PackedMsa
    ref = _row_stream("mixed")
    _, pk, qkv, H, scale = ref[:5]
    order = [4, 0, 6, 2, 3, 1, 5]
    blocks = pk.unpack()
    perm = PackedMsa.from_list([blocks[b] for b in order], padded_shape=pk.padded_shape)
    qs = pk.unpack(_to_stream(pk, qkv))
    qperm = torch.zeros(perm.T_pad, qkv.shape[1], dtype=qkv.dtype, device=DEV)
    qperm[:perm.n_tokens] = torch.cat([qs[b].reshape(-1, qkv.shape[1]) for b in order])
    S_of, ctx = _row_ragged(perm, qperm, H, scale)
    _check_row(perm, S_of, ctx, ref, order=order, fp64=False)
    groups = plan_groups_ragged(pk.shapes, H, budget=1)
    assert groups == [(b, b + 1) for b in range(len(pk))]
    S_of, ctx = _row_ragged(pk, _to_stream(pk, qkv), H, scale, groups=groups)
    _check_row(pk, S_of, ctx, ref, fp64=False)
    S_of, ctx = _row_ragged(pk, _to_stream(pk, qkv), H, scale, groups=[(0, 3), (3, 4), (4, 7)])
    _check_row(pk, S_of, ctx, ref, fp64=False)


# ---------------------------------------------------------------------------------------------------------------- column attention
COL_BLOCKS = [(1, 33), (2, 1), (17, 33), (33, 1), (50, 33), (128, 33), (1, 1), (2, 33)]


@functools.lru_cache(maxsize=None)
def _col_stream():
    from oneprot_amd.packing import PackedMsa
    H, B, R, L = 2, len(COL_BLOCKS), 128, 33
    ids = _ids(B, R, L, [l for _, l in COL_BLOCKS], [r for r, _ in COL_BLOCKS], ((4, 7, 3), (0, 0, 9)))      # a hole; the ONE key of a one-row MSA masked
    ids[2, :, 5] = 1                                                        # one column with every key masked, inside its block
    pk = PackedMsa.from_padded(ids).to(DEV)
    assert pk.shapes == COL_BLOCKS
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * R * L, 3 * H * 64, generator=g).to(torch.bfloat16).to(DEV)
    return ids, pk, qkv, H


def test_col_attention_ragged_vs_fp64_and_bit_equal_to_padded():
    ids, pk, qkv, H = _col_stream()
    B, R, L = ids.shape
    ctx = _col_ragged(pk, _to_stream(pk, qkv), H)
    _tail_is_zero(pk, ctx)
    ctx_pad = _col_padded(qkv, ids, H)
    pad = ids.eq(1).to(DEV)
    q, k, v = qkv.to(F64).view(B, R, L, 3, H * 64).unbind(3)
    c64 = MR.col_context(q, k, v, pad, H, general=True)
    live = (~pad).any(dim=1)                                                # [B, L]: columns with at least one key
    assert not bool(live[2, 5]) and not bool(live[0, 9])
    for b, blk in enumerate(pk.unpack(ctx)):
        rb, lb = pk.shapes[b]
        valid = ~pad[b, :rb, :lb]
        assert torch.equal(blk[valid], ctx_pad[b, :rb, :lb][valid]), f"col ctx of MSA {b} {rb}x{lb} differs from the padded kernel's"
        sel = live[b, None, :lb, None].expand(rb, lb, H * 64)
        zero64, zero32 = torch.zeros((), dtype=F64, device=DEV), torch.zeros((), device=DEV)
        close(torch.where(sel, blk.float(), zero32), torch.where(sel, c64[b, :rb, :lb], zero64), 2 ** -7, 2e-2, f"ragged col ctx, MSA {b} {rb}x{lb}")
        assert bool((blk[:, ~live[b, :lb]] == 0).all())                     # every key masked: 0


# ---------------------------------------------------------------------------------------------------------------- embedding
def test_embed_ragged_bit_equal_to_padded_and_vs_fp64():
    from oneprot_amd import hip
    from oneprot_amd.packing import PackedMsa
    B, R, L, d, V, max_pos, rows_tab = 3, 5, 70, 128, 33, 80, 8
    g = torch.Generator().manual_seed(3)
    tok = _tokens(B, R, L, [70, 33, 9], [5, 3, 1], 4)
    tok[0, 1, 9] = tok[0, 1, 10] = tok[0, 2, 31] = tok[1, 2, 4] = tok[1, 0, 30] = 1      # interior padding: the positions behind it do not count it
    pk = PackedMsa.from_padded(tok).to(DEV)
    assert pk.shapes == [(5, 70), (3, 33), (1, 9)]
    sd = {"embed_tokens.weight": torch.randn(V, d, generator=g) * 0.05, "embed_positions.weight": torch.randn(max_pos + 2, d, generator=g) * 0.05,
          "msa_position_embedding": torch.randn(1, rows_tab, 1, d, generator=g) * 0.05, "emb_layer_norm_before.weight": 1 + 0.1 * torch.randn(d, generator=g),
          "emb_layer_norm_before.bias": 0.1 * torch.randn(d, generator=g)}
    a = [sd[k].to(DEV).contiguous() for k in sd]
    xp = torch.full((B * R * L, d), float("nan"), device=DEV)
    hip.call("oneprot_msa_embed_fwd", tok.to(DEV), *a, xp, B, R, L, d, V, max_pos + 2, rows_tab, 1, 1e-5)
    x = torch.full((pk.T_pad, d), float("nan"), device=DEV)
    hip.call("oneprot_msa_embed_ragged_fwd", pk.ids, pk.cu_tokens, pk.row_lens(), *a, x, len(pk), pk.T_pad, 5, 70, d, V, max_pos + 2, rows_tab, 1, 1e-5)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and bool((x[pk.n_tokens:] == 0).all())
    ref = MR.embed(tok, {k: v.to(F64) for k, v in sd.items()})
    for b, blk in enumerate(pk.unpack(x)):
        rb, lb = pk.shapes[b]
        assert torch.equal(blk, xp.view(B, R, L, d)[b, :rb, :lb]), f"embedding of MSA {b} differs from the padded kernel's"
        close(blk, ref[b, :rb, :lb], 1e-5, 1e-5, f"ragged embed, MSA {b}")
        assert bool((blk[pk.unpack()[b].eq(1)] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- tower / encoder
E2E = [((3, 5, 70), [70, 44, 9], [5, 3, 1]), ((2, 1, 40), [33, 20], [1, 1])]


def _padded_twin_captures(tr, pk, tok, stages, captures):
    """What the padded kernels give on the padded batch from the very operands the packed run's attentions read (its `stages` taps "row.qkv" / "col.qkv",
    scattered to the padded layout; zeros elsewhere: those positions are padding -- q counts as 0 there and the keys are masked).  The full padded forward
    is no bit-level twin: its GEMMs run on B * R * L rows, the stream's on T_pad, and the NT GEMM picks its kernel by M % 256 (csrc/gemm_nt.hip)."""
    B, R, L = tok.shape
    H = tr.H
    pi, si = _index(pk)
    pi, si = pi.to(DEV), si.to(DEV)
    n = 0
    for (kind, layer, ctx) in captures:
        taps = [t for (name, i, t) in stages if name == kind + ".qkv" and i == layer]
        if not taps:                                                        # R = 1: the column block is two GEMMs, no attention kernel
            assert kind == "col" and R == 1
            continue
        qkv = torch.zeros(B * R * L, taps[0].shape[1], dtype=torch.bfloat16, device=DEV)
        qkv[pi] = taps[0][si]
        twin = _row_padded(qkv, tok, H, 64 ** -0.5 / math.sqrt(R))[1] if kind == "row" else _col_padded(qkv, tok, H)
        valid = tok.ne(1).to(DEV).view(-1)[pi]
        assert torch.equal(ctx[si][valid], twin.reshape(B * R * L, -1)[pi][valid]), f"{kind} attention of layer {layer}: packed != padded kernels on the same operands"
        n += 1
    return n


@pytest.mark.parametrize("pooling,proj", [("mean", "linear"), ("cls", "mlp")])
@pytest.mark.parametrize("use_all_msa", [True, False])
@pytest.mark.parametrize("shape,lens,rows", E2E, ids=[str(c[0]) for c in E2E])
def test_msa_encoder_on_a_packed_msa_vs_restatement(tmp_path, shape, lens, rows, use_all_msa, pooling, proj):
    from oneprot_amd.packing import PackedMsa
    from src.models.components.msa_encoder import MsaEncoder
    scale = proj == "mlp"
    enc = MsaEncoder(_checkpoint(tmp_path), output_dim=64, pooling_type=pooling, proj_type=proj, use_logit_scale=scale, use_all_msa=use_all_msa)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    enc = enc.to(DEV)
    tr = enc.transformer
    tok = _tokens(*shape, lens, rows, 9)
    pk = PackedMsa.from_padded(tok).to(DEV)
    assert pk.shapes == [(r, l) for r, l in zip(rows, lens)] and pk.padded_shape == shape[1:]
    with torch.no_grad():
        feats = enc(pk).cpu()
        tr.capture, tr.stages = [], []
        stream = tr(pk)["representations"][2]
        captures, stages, tr.capture, tr.stages = tr.capture, tr.stages, None, None
        feats_pad = enc(tok.to(DEV)).cpu()
        hidden_pad = tr(tok.to(DEV))["representations"][2]
    assert tuple(stream.shape) == (pk.T_pad, 128) and torch.isfinite(stream).all() and torch.isfinite(feats).all()      # tail rows included
    assert len(captures) == 4 and all(torch.isfinite(c.float()).all() for _, _, c in captures)
    ref_h, ref_f = MR.encoder_features(tok, sd, 2, use_all_msa, pooling)
    err = diff = 0.0
    for b, blk in enumerate(pk.unpack(stream)):
        rb, lb = pk.shapes[b]
        m = tok[b, :rb, :lb].ne(1).unsqueeze(-1).to(F64)
        err = max(err, float(((blk.cpu().to(F64) - ref_h[b, :rb, :lb]) * m).abs().max()))
        diff = max(diff, float(((blk - hidden_pad[b, :rb, :lb]).cpu().to(F64) * m).abs().max()))
    cs = torch.nn.functional.cosine_similarity(feats.to(F64), ref_f, dim=-1)
    print(f"hidden max err {err:.3e} of {float(ref_h.abs().max()):.3e}; cosine {float(cs.min()):.6f}; largest difference to the padded HIP forward: "
          f"hidden {diff:.3e}, features {float((feats - feats_pad).abs().max()):.3e}")
    assert err < 0.05 * ref_h.abs().max()
    assert cs.min() > 0.999, cs
    assert abs(feats.norm(dim=-1) - (1 / 0.07 if scale else 1.0)).max() < 1e-3
    assert _padded_twin_captures(tr, pk, tok, stages, captures) == (2 if shape[1] == 1 else 4)
    # hidden_and_pooled hands the representation back in the packed form
    hid, pooled = enc.hidden_and_pooled(pk)
    close = lambda u, v: torch.allclose(u, v, rtol=1e-4, atol=1e-4)        # two fp32 LayerNorm kernels (fused with the pooling / alone) on unit-scale rows: a few ulp apart
    assert tuple(pooled.shape) == (len(pk), 128)
    if use_all_msa:
        assert close(hid[:pk.n_tokens], stream[:pk.n_tokens])
    else:
        assert [tuple(h.shape) for h in hid] == [(l, 128) for l in lens]
        assert close(hid[1], pk.unpack(stream)[1][0])


def test_packed_tower_grouping_leaves_the_stream_bit_identical(tmp_path, monkeypatch):
    from oneprot_amd.msa import MsaTransformer
    from oneprot_amd.packing import PackedMsa
    tr = MsaTransformer.from_pretrained(_checkpoint(tmp_path)).to(DEV)
    pk = PackedMsa.from_padded(_tokens(3, 4, 50, [50, 31, 45], [4, 2, 3], 2)).to(DEV)
    outs = []
    for budget in (None, "1"):
        if budget is None:
            monkeypatch.delenv("ONEPROT_MSA_SCORE_BYTES", raising=False)
        else:
            monkeypatch.setenv("ONEPROT_MSA_SCORE_BYTES", budget)
        x, _ = tr.run_layers(pk)
        torch.cuda.synchronize()
        outs.append(x.clone())
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()


# ---------------------------------------------------------------------------------------------------------------- dropout
SEED, STREAM = 1234, (3 << 60) | 77


@pytest.mark.parametrize("b_off", [0, 3])
def test_ragged_row_dropout_is_the_padded_twins_mask(b_off):
    ids, pk, qkv, H, scale, _, ctx_pad0, _, _ = _row_stream("mixed")
    qs = _to_stream(pk, qkv)
    _, ctx_pad = _row_padded(qkv, ids, H, scale, drop=(b_off, 0.5, SEED, STREAM))
    _, ctx = _row_ragged(pk, qs, H, scale, groups=[(0, 2), (2, 7)], drop=(0.5, SEED, STREAM), b_off=b_off)      # b_first = b_off + the group's first MSA
    _tail_is_zero(pk, ctx)
    differs = False
    for b, blk in enumerate(pk.unpack(ctx)):
        rb, lb = pk.shapes[b]
        assert torch.equal(blk, ctx_pad[b, :rb, :lb]), f"dropped row ctx of MSA {b} differs from the padded twin's"
        differs |= not torch.equal(blk, ctx_pad0[b, :rb, :lb])
    assert differs
    _, ctx0 = _row_ragged(pk, qs, H, scale, drop=(0.0, SEED, STREAM))
    _, ctxu = _row_ragged(pk, qs, H, scale)
    assert torch.equal(ctx0, ctxu)


def test_ragged_col_dropout_is_the_padded_twins_mask():
    ids, pk, qkv, H = _col_stream()
    qs = _to_stream(pk, qkv)
    ctx_pad = _col_padded(qkv, ids, H, drop=(0.5, SEED, STREAM))
    ctx = _col_ragged(pk, qs, H, drop=(0.5, SEED, STREAM))
    _tail_is_zero(pk, ctx)
    und = _col_ragged(pk, qs, H)
    pad = ids.eq(1).to(DEV)
    for b, blk in enumerate(pk.unpack(ctx)):
        rb, lb = pk.shapes[b]
        valid = ~pad[b, :rb, :lb]
        assert torch.equal(blk[valid], ctx_pad[b, :rb, :lb][valid]), f"dropped col ctx of MSA {b} differs from the padded twin's"
    assert not torch.equal(ctx, und)
    assert torch.equal(_col_ragged(pk, qs, H, drop=(0.0, SEED, STREAM)), und)


def test_packed_tower_with_dropout_is_deterministic_finite_and_different(tmp_path):
    from oneprot_amd.msa import MsaTransformer
    from oneprot_amd.packing import PackedMsa
    tr = MsaTransformer.from_pretrained(_checkpoint(tmp_path)).to(DEV)
    pk = PackedMsa.from_padded(_tokens(3, 5, 70, [70, 44, 9], [5, 3, 1], 9)).to(DEV)
    tr.set_rng_state({"_drop_seed": SEED, "_drop_calls": 0})
    state = tr.rng_state()
    a, _ = tr.run_layers(pk, drop=True)
    a = a.clone()
    assert tr.rng_state()["_drop_calls"] == 1
    b, _ = tr.run_layers(pk, drop=True)                                     # the next call id: another draw
    b = b.clone()
    tr.set_rng_state(state)
    c, _ = tr.run_layers(pk, drop=True)
    plain, _ = tr.run_layers(pk)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert torch.equal(a, c) and not torch.equal(a, b) and not torch.equal(a, plain)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_ragged_entry_points_refuse_bad_tables_and_sizes_without_a_launch():
    from oneprot_amd import hip
    from oneprot_amd.msa import MsaTransformer, config_from_args
    from oneprot_amd.packing import PackedMsa
    h = hip.lib()
    H = 1
    pk = PackedMsa.from_list([torch.full((2, 8), 5, dtype=torch.int64), torch.full((1, 3), 5, dtype=torch.int64)]).to(DEV)
    (g,) = pk.tables(H)
    T = pk.T_pad
    qkv = torch.zeros(T, 192, dtype=torch.bfloat16, device=DEV)
    kb = torch.zeros(T, device=DEV)
    mark = 7.0
    ctx = torch.full((T, 64), mark, dtype=torch.bfloat16, device=DEV)
    S = torch.full((g["s_elems"],), mark, device=DEV)
    nbytes = hip.query("oneprot_msa_row_context_ragged_workspace", g["sum_l_lp"], g["sum_r_lp"], H)
    assert nbytes == 2 * (g["sum_l_lp"] + 64 * g["sum_r_lp"])
    assert hip.query("oneprot_msa_row_context_ragged_workspace", 0, 32, 1) == 0 and hip.query("oneprot_msa_row_context_ragged_workspace", 33, 32, 1) == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()
    geo = p(g["geo"])
    scores = lambda geo_, n, max_L, H_, hd: h.oneprot_msa_row_scores_ragged(p(qkv), p(kb), p(S), geo_, n, max_L, H_, hd, 0.125, None)
    assert scores(None, 2, 8, 1, 64) == -1 and scores(geo + 8, 2, 8, 1, 64) == -1                  # no table; a table off its 16-byte alignment
    assert scores(geo, 0, 8, 1, 64) == -1 and scores(geo, 2, hip.MSA_MAX_LEN + 1, 1, 64) == -1 and scores(geo, 2, 8, 1, 32) == -1 and scores(geo, 65536, 8, 1, 64) == -1
    rctx = lambda geo_, nb, max_R, Tn, Tp: h.oneprot_msa_row_context_ragged(p(S), p(qkv), p(kb), p(ctx), p(ws), nb, geo_, 2, max_R, 8, g["sum_l_lp"], g["sum_r_lp"],
                                                                              1, 64, Tn, Tp, None)
    assert rctx(None, nbytes, 2, 19, T) == -1 and rctx(geo, nbytes - 1, 2, 19, T) == -1 and rctx(geo, nbytes, 0, 19, T) == -1
    assert rctx(geo, nbytes, 2, 0, T) == -1 and rctx(geo, nbytes, 2, T + 1, T) == -1               # the token count against T_pad
    assert h.oneprot_msa_row_context_ragged_dropout(p(S), p(qkv), p(kb), p(ctx), p(ws), nbytes, geo, 2, 2, 8, g["sum_l_lp"], g["sum_r_lp"], 1, 64, 19, T, 0, 1.0, 1, 1,
                                                    None) == -1              # p = 1
    assert h.oneprot_msa_row_context_ragged_dropout(p(S), p(qkv), p(kb), p(ctx), p(ws), nbytes, geo, 2, 2, 8, g["sum_l_lp"], g["sum_r_lp"], 1, 64, 19, T, -1, 0.5, 1, 1,
                                                    None) == -1              # b_first < 0
    col = lambda geo_, max_R, max_L, hd: h.oneprot_msa_col_attn_ragged(p(qkv), p(kb), p(ctx), geo_, 2, max_R, max_L, 1, hd, 0.125, 19, T, None)
    assert col(None, 2, 8, 64) == -1 and col(geo, hip.MSA_MAX_ROWS + 1, 8, 64) == -1 and col(geo, 2, 0, 64) == -1 and col(geo, 2, 8, 48) == -1
    cdrop = lambda l_stride, prob: h.oneprot_msa_col_attn_ragged_dropout(p(qkv), p(kb), p(ctx), geo, 2, 2, 8, 1, 64, 0.125, 19, T, l_stride, prob, 1, 1, None)
    assert cdrop(7, 0.5) == -1 and cdrop(hip.MSA_MAX_LEN + 1, 0.5) == -1 and cdrop(8, float("nan")) == -1      # a stride shorter than the longest row
    x = torch.full((T, 64), mark, device=DEV)
    tabs = [torch.zeros(40, 64, device=DEV) for _ in range(3)] + [torch.ones(64, device=DEV), torch.zeros(64, device=DEV)]
    emb = lambda cu, n, max_R, max_L, n_pos, n_rows: h.oneprot_msa_embed_ragged_fwd(p(pk.ids), cu, p(pk.row_lens()), *[p(t) for t in tabs], p(x), n, T, max_R, max_L, 64, 33,
                                                                                     n_pos, n_rows, 1, 1e-5, None)
    assert emb(None, 2, 2, 8, 40, 40) == -1 and emb(p(pk.cu_tokens), 0, 2, 8, 40, 40) == -1
    assert emb(p(pk.cu_tokens), 2, 2, 8, 9, 40) == -1 and emb(p(pk.cu_tokens), 2, 2, 8, 40, 1) == -1          # position table / row table too short
    torch.cuda.synchronize()
    assert bool((ctx == mark).all()) and bool((S == mark).all()) and bool((x == mark).all())                    # nothing was launched
    tr = MsaTransformer(config_from_args(ARCH))
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        tr.run_layers(pk.to("cpu"))


# ---------------------------------------------------------------------------------------------------------------- module
def test_module_steps_with_a_packed_msa_batch(tmp_path):
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    warnings.filterwarnings("ignore", message=".*no weight file.*")
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.optim import FusedAdam
    from oneprot_amd.packing import PackedMsa
    from src.models.components.msa_encoder import MsaEncoder
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.oneprot_module import OneProtLitModule
    torch.manual_seed(0)
    seq = SequenceEncoder("facebook/esm2_t6_8M_UR50D", output_dim=64, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
    msa = MsaEncoder(_checkpoint(tmp_path), output_dim=64, pooling_type="mean", proj_type="mlp", use_logit_scale=True, use_all_msa=True)
    module = OneProtLitModule(components={"sequence": seq, "msa": msa}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP").to(DEV)
    before = msa.transformer.flat.detach().clone()
    batch = next(iter(SyntheticPairs("msa", 4, 32, 48, msa_depth=5, ragged=True, packed_msa=True, device=DEV)))
    padded = next(iter(SyntheticPairs("msa", 4, 32, 48, msa_depth=5, ragged=True, device=DEV)))
    assert isinstance(batch[1], PackedMsa) and batch[1].is_cuda and torch.equal(batch[1].to_padded(), padded[1])
    module.eval()
    with torch.no_grad():
        cs = torch.nn.functional.cosine_similarity(module(batch[1], "msa"), module(padded[1], "msa"), dim=-1)
    print(f"packed against padded features of the same batch: cosine {float(cs.min()):.6f}")
    assert cs.min() > 0.999
    module.train()
    assert not msa.transformer.training
    loss = module.training_step({"msa": batch}, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    g = seq.transformer.flat.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0
    assert all(p.grad is None for p in msa.transformer.parameters())
    assert torch.equal(msa.transformer.flat.detach(), before)
    assert any(p.grad is not None for p in msa.proj.parameters())
    module.eval()
    module.validation_step(batch, 0)
    assert module.metrics["val_msa"].global_count() > 0
