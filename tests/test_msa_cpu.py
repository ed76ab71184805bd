"""The MSA modality without a device: the fp64 restatement (tests/msa_ref.py) checked against itself, the public surface, the state-dict keys, the
fair-esm file loader, the refusals, the group planner and the synthetic batches."""
import inspect
import math
import os

import pytest
import torch

from tests import msa_cases as MC
from tests import msa_ref as MR
from tests.msa_cases import _tower, _write_fair_esm_file

F64 = torch.float64


def _qkv(B, R, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, R, L, D, generator=g, dtype=F64) for _ in range(3))


# ---------------------------------------------------------------------------------------------------------------- the restatement against itself
def test_tied_scores_einsum_equals_loop_over_rows():
    q, k, _ = _qkv(2, 3, 7, 128, 0)
    pad = torch.zeros(2, 3, 7, dtype=torch.bool)
    pad[1, :, 5:] = True
    pad[0, 2, 3] = True
    a, b = MR.row_scores(q, k, pad, 2), MR.row_scores_loop(q, k, pad, 2)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    assert float(a[0, :, 3].abs().max()) > 0 and float(MR.row_scores(q[:, 2:], k[:, 2:], pad[:, 2:], 2)[0, :, 3].abs().max()) == 0      # q zeroed at the pad


def test_column_shortcut_equals_general_formula_at_one_row():
    q, k, v = _qkv(2, 1, 6, 128, 1)
    pad = torch.zeros(2, 1, 6, dtype=torch.bool)
    assert torch.allclose(MR.col_context(q, k, v, pad, 2), MR.col_context(q, k, v, pad, 2, general=True), rtol=1e-12, atol=1e-12)


def test_positions_skip_interior_padding():
    row = torch.tensor([[0, 5, 1, 1, 6, 7, 1]])
    assert MR.positions(row).tolist() == [[2, 3, 1, 1, 4, 5, 1]]


def test_row_scale_uses_the_padded_row_count():
    """appending a fully padded row changes the tied row attention (the published scale is hd^-1/2 / sqrt(R) with R the padded depth)"""
    tr = _tower()
    sd = {k: v.detach() for k, v in tr.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    tok = torch.randint(4, 30, (1, 2, 9), generator=g)
    tok[:, :, 0] = 0
    more = torch.cat([tok, torch.ones(1, 1, 9, dtype=torch.int64)], dim=1)
    a, b = MR.forward(tok, sd, 2), MR.forward(more, sd, 2)[:, :2]
    assert torch.isfinite(b).all() and float((a - b).abs().max()) > 1e-6
    q, k, _ = _qkv(1, 3, 9, 128, 5)
    q[:, 2] = 0
    pad2, pad3 = torch.zeros(1, 2, 9, dtype=torch.bool), torch.zeros(1, 3, 9, dtype=torch.bool)
    assert torch.allclose(MR.row_scores(q, k, pad3, 2) * math.sqrt(3), MR.row_scores(q[:, :2], k[:, :2], pad2, 2) * math.sqrt(2), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("R", [3, 1])
def test_stage_helpers_chained_reproduce_forward(R):
    """qkv_proj -> row / column context -> attn_out, ffn: the helpers of the per-stage tower test, chained in fp64, are MR.forward (R = 1: the column shortcut)"""
    tr = _tower()
    with torch.no_grad():
        tr.flat.normal_(0.0, 0.08)
    sd = {k: v.detach().to(F64) for k, v in tr.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    tok = torch.randint(4, 30, (2, R, 11), generator=g)
    tok[:, :, 0] = 0
    tok[1, :, 8:] = 1
    tok[0, R - 1, 4] = 1
    pad = tok.eq(1)
    x = MR.embed(tok, sd)
    for i in range(2):
        q, k, v = MR.qkv_proj(x, sd, i, "row_self_attention").chunk(3, dim=-1)
        x = MR.attn_out(x, MR.row_context(MR.row_scores(q, k, pad, 2), v, pad, 2), sd, i, "row_self_attention")
        q, k, v = MR.qkv_proj(x, sd, i, "column_self_attention").chunk(3, dim=-1)
        x = MR.attn_out(x, MR.col_context(q, k, v, pad, 2), sd, i, "column_self_attention")
        x = MR.ffn(x, sd, i)
    x = MR._ln(x, sd, "emb_layer_norm_after")
    ref = MR.forward(tok, sd, 2)
    assert torch.allclose(x, ref, rtol=1e-12, atol=1e-12) and float(ref.abs().max()) > 0.1


def test_ffn_gate_of_the_grouped_stage_test_is_the_measured_one(tmp_path):
    """tests/test_msa_edges_gpu.py runs the FFN stage of its grouped tower test at four times the reference's own difference (bf16-rounded LayerNorm and GELU
    outputs against exact ones): that figure, recomputed here from the same file of weights and the same tokens"""
    from oneprot_amd.msa import MsaTransformer
    tr = MsaTransformer.from_pretrained(MC._checkpoint(tmp_path))
    shape, lens, rows, seed = MC.GROUPED
    diff = MR.ffn_rounding_self_difference(MC._tokens(*shape, lens, rows, seed), tr.state_dict(), tr.H, MC.bf)
    assert len(diff) == 2 and diff[0] > diff[1] and 0.995 * MC.FFN_SELF_DIFFERENCE_GROUPED < diff[0] <= MC.FFN_SELF_DIFFERENCE_GROUPED


# ---------------------------------------------------------------------------------------------------------------- surface
def test_msa_encoder_signature_is_the_reference_one():
    from src.models.components.msa_encoder import MsaEncoder
    from oneprot_amd.encoders import BaseEncoder
    assert issubclass(MsaEncoder, BaseEncoder)
    sig = inspect.signature(MsaEncoder.__init__)
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    E = inspect.Parameter.empty
    assert got == [("model_name_or_path", E), ("output_dim", E), ("pooling_type", "mean"), ("proj_type", None), ("use_logit_scale", False),
                   ("learnable_logit_scale", False), ("use_all_msa", False)]


def _published_keys(n_layers):
    keys = ["embed_tokens.weight", "embed_positions.weight", "msa_position_embedding"]
    keys += [f"emb_layer_norm_{w}.{p}" for w in ("before", "after") for p in ("weight", "bias")]
    for i in range(n_layers):
        for blk in ("row_self_attention", "column_self_attention"):
            keys += [f"layers.{i}.{blk}.layer.{n}_proj.{p}" for n in ("q", "k", "v", "out") for p in ("weight", "bias")]
        for blk in ("row_self_attention", "column_self_attention", "feed_forward_layer"):
            keys += [f"layers.{i}.{blk}.layer_norm.{p}" for p in ("weight", "bias")]
        keys += [f"layers.{i}.feed_forward_layer.layer.{n}.{p}" for n in ("fc1", "fc2") for p in ("weight", "bias")]
    return keys


def test_state_dict_keys_and_strict_round_trip():
    tr = _tower()
    sd = tr.state_dict()
    extras = {k for k in sd if k.startswith(("lm_head.", "contact_head."))}
    assert set(sd) - extras == set(_published_keys(2))
    assert extras and "flat" not in sd
    assert tuple(sd["msa_position_embedding"].shape) == (1, 1024, 1, 128) and tuple(sd["embed_positions.weight"].shape) == (160 + 1 + 1, 128)
    with torch.no_grad():
        tr.flat.normal_()
    other = _tower()
    res = other.load_state_dict({k: v.clone() for k, v in tr.state_dict().items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(other.flat, tr.flat)
    assert not any(p.requires_grad for p in other.parameters()) and not other.training
    other.train()
    assert not other.training                                            # frozen, eval only


def test_loader_reads_a_fair_esm_file_and_swaps_row_and_column(tmp_path):
    from oneprot_amd.msa import MsaTransformer
    tr = _tower()
    with torch.no_grad():
        tr.flat.normal_()
    path = os.path.join(str(tmp_path), "tiny.pt")
    _write_fair_esm_file(path, tr)
    on_disk = torch.load(path, weights_only=False)["model"]
    assert "encoder.layers.0.column_self_attention.layer.q_proj.weight" in on_disk
    assert torch.equal(on_disk["encoder.layers.0.column_self_attention.layer.q_proj.weight"], tr.view("layers.0.row_self_attention.layer.q_proj.weight"))
    got = MsaTransformer.from_pretrained(path)
    assert (got.n_layers, got.d, got.f, got.H, got.config.max_positions) == (2, 128, 256, 2, 160)
    assert torch.equal(got.view("layers.0.row_self_attention.layer.q_proj.weight"), tr.view("layers.0.row_self_attention.layer.q_proj.weight"))
    assert torch.equal(got.flat, tr.flat)


# ---------------------------------------------------------------------------------------------------------------- refusals (no device)
def test_refusals_before_the_device(tmp_path, monkeypatch):
    from oneprot_amd import hip
    from oneprot_amd.packing import PackedTokens
    from src.models.components.msa_encoder import MsaEncoder
    monkeypatch.delenv("ONEPROT_ALLOW_RANDOM_INIT", raising=False)
    with pytest.raises(OSError, match="ONEPROT_ALLOW_RANDOM_INIT=1"):
        MsaEncoder(os.path.join(str(tmp_path), "absent.pt"), output_dim=32)
    path = os.path.join(str(tmp_path), "tiny.pt")
    _write_fair_esm_file(path, _tower())
    enc = MsaEncoder(path, output_dim=32, proj_type="linear", use_all_msa=True)
    assert enc.d_model == 128 and "use_all_msa=True" in repr(enc)
    with pytest.raises(NotImplementedError, match="packed token streams"):
        enc(PackedTokens.from_padded(torch.tensor([[0, 5, 2, 1]]), pad_id=1))
    with pytest.raises(ValueError, match="max_positions"):
        enc(torch.zeros(1, 2, 161, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match=str(hip.MSA_MAX_ROWS)):
        enc(torch.zeros(1, hip.MSA_MAX_ROWS + 1, 8, dtype=torch.int64))
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        enc(torch.zeros(1, 2, 8, dtype=torch.int64))


def test_random_init_switch_builds_the_published_architecture(monkeypatch):
    from oneprot_amd.msa import MsaTransformer
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    with pytest.warns(UserWarning, match="random initialisation"):
        tr = MsaTransformer.from_pretrained("/nowhere/esm_msa1b_t12_100M_UR50S.pt")
    assert (tr.n_layers, tr.d, tr.f, tr.H, tr.config.max_positions) == (12, 768, 3072, 12, 1024)


# ---------------------------------------------------------------------------------------------------------------- group planner
@pytest.mark.parametrize("B,R,L,H,budget", [(16, 50, 512, 12, 1 << 30), (5, 3, 100, 2, 4 * 2 * 100 * 100 * 2), (7, 2, 64, 12, 1), (1, 1, 8, 1, 1 << 30)])
def test_group_planner(B, R, L, H, budget):
    from oneprot_amd.msa import plan_groups
    groups = plan_groups(B, R, L, H, budget)
    assert groups == plan_groups(B, R, L, H, budget)
    assert [b for b0, b1 in groups for b in range(b0, b1)] == list(range(B))
    per = 4 * H * L * L
    for b0, b1 in groups:
        assert b1 > b0 and ((b1 - b0) * per <= budget or b1 - b0 == 1)
    if budget < per:
        assert all(b1 - b0 == 1 for b0, b1 in groups)


def test_group_planner_reads_the_environment(monkeypatch):
    from oneprot_amd.msa import plan_groups
    monkeypatch.setenv("ONEPROT_MSA_SCORE_BYTES", "1")
    assert len(plan_groups(3, 2, 16, 2)) == 3
    monkeypatch.delenv("ONEPROT_MSA_SCORE_BYTES")
    assert plan_groups(3, 2, 16, 2) == [(0, 3)]


# ---------------------------------------------------------------------------------------------------------------- synthetic batches
def test_synthetic_msa_batches():
    from oneprot_amd.data import SyntheticPairs
    mk = lambda **kw: list(SyntheticPairs("msa", 6, 24, 40, n_batches=2, msa_depth=7, seed=5, **kw))
    a, b = mk(ragged=True), mk(ragged=True)
    assert len(a) == 2
    for (s1, m1, n1, r1), (s2, m2, _, _) in zip(a, b):
        assert n1 == "msa" and r1 is None and torch.equal(s1, s2) and torch.equal(m1, m2)
        assert tuple(s1.shape) == (6, 24) and tuple(m1.shape) == (6, 7, 40) and m1.dtype == torch.int64
        assert int(m1.min()) >= 0 and int(m1.max()) < 33
        pad = m1.eq(1)
        for x in range(6):
            rows = int((~pad[x]).any(dim=1).sum())
            n = int((~pad[x, 0]).sum())
            assert rows >= 1 and bool((m1[x, :rows, 0] == 0).all())
            assert bool(pad[x, rows:].all()) and bool(pad[x, :, n:].all()) and not bool(pad[x, :rows, :n].any())
    assert any(bool(m.eq(1)[x].all(dim=1).any()) for _, m, _, _ in a for x in range(6))     # some MSA is shallower than msa_depth
    full = mk()[0][1]
    assert not bool(full.eq(1).any())
    assert not torch.equal(mk(ragged=True)[0][1], list(SyntheticPairs("msa", 6, 24, 40, msa_depth=7, seed=6, ragged=True))[0][1])
    # the other modalities are untouched by the new argument
    x = list(SyntheticPairs("struct_token", 3, 16, seed=1))[0]
    y = list(SyntheticPairs("struct_token", 3, 16, seed=1, msa_depth=9))[0]
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
