"""The MSA tower on the GPU: the four oneprot_msa_* entry points against the fp64 restatement tests/msa_ref.py on bf16-rounded randn inputs handed
identically to both, batch independence and grouping bit for bit, MsaEncoder end to end, and one training sub-step of OneProtLitModule with the frozen tower.

Tolerances are the project's (tests/test_gemm_small_shapes_gpu.py): fp32 outputs rtol 1e-4, atol 1e-3 * sqrt(K / 64) -- K = R * 64 for the tied scores --;
bf16 outputs rtol 2^-7, atol 2e-2, which covers the bf16 rounding of the probabilities (their rows sum to 1: at most about 2^-9 * max|v|).  A NaN or Inf
anywhere fails, padded positions included.  Parity with fair-esm itself is unpinned (see tests/msa_ref.py)."""
import functools
import math
import os
import warnings

import pytest
import torch

from tests import msa_ref as MR

from tests.gate import close
from tests.msa_cases import DEV, E2E, F64, ROW_CASES, _checkpoint, _col, _ids, _qkv, _row, _split, _tokens

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,lens,rows,holes", ROW_CASES, ids=[str(c[0]) for c in ROW_CASES])
def test_row_scores_and_context_vs_fp64(shape, lens, rows, holes):
    B, R, L, H = shape
    ids = _ids(B, R, L, lens, rows, holes)
    qkv = _qkv(B, R, L, H, 11 + L)
    S, ctx = _row(qkv, ids, H)
    pad = ids.eq(1)
    q, k, v = _split(qkv, B, R, L, H)
    S64 = MR.row_scores(q, k, pad, H)
    close(S, S64, 1e-4, 1e-3 * math.sqrt(R), f"S {shape}")
    c64 = MR.row_context(S64, v, pad, H)
    close(ctx.view(B, R, L, H * 64), c64, 2 ** -7, 2e-2, f"row ctx {shape}")


@pytest.mark.parametrize("L", [1, 33])
@pytest.mark.parametrize("R", [2, 3, 16, 17, 31, 32, 33, 50, 64, 65, 96, 97, 127, 128])       # every edge of R rounded up to 16 (query tiles) and to 32 (LDS fill, P.V trips)
def test_col_attn_vs_fp64(R, L):
    B, H = 2, 2
    ids = _ids(B, R, L, [L, L], [R - R // 3, max(R // 2, 1)])             # trailing rows fully padded
    ids[1, :, L - 1] = 1                                                  # one column with every key masked
    qkv = _qkv(B, R, L, H, 100 * R + L)
    ctx = _col(qkv, ids, H).view(B, R, L, H * 64)
    assert torch.isfinite(ctx).all()
    pad = ids.eq(1)
    q, k, v = _split(qkv, B, R, L, H)
    c64 = MR.col_context(q, k, v, pad, H, general=True)
    live = (~pad).any(dim=1)                                              # [B, L]: columns with at least one key
    assert not bool(live[1, L - 1])
    sel = live[:, None, :, None].expand_as(c64)
    close(torch.where(sel.to(DEV), ctx.float(), torch.zeros((), device=DEV)), torch.where(sel, c64, torch.zeros((), dtype=F64)), 2 ** -7, 2e-2, f"col ctx R={R} L={L}")


def test_col_attn_refuses_more_than_128_rows():
    from oneprot_amd import hip
    qkv = torch.zeros(129, 192, dtype=torch.bfloat16, device=DEV)
    kb = torch.zeros(129, device=DEV)
    ctx = torch.zeros(129, 64, dtype=torch.bfloat16, device=DEV)
    assert hip.lib().oneprot_msa_col_attn(qkv.data_ptr(), kb.data_ptr(), ctx.data_ptr(), 1, 129, 1, 1, 64, 0.125, None) == -1
    assert hip.lib().oneprot_msa_col_attn(qkv.data_ptr(), kb.data_ptr(), ctx.data_ptr(), 1, 64, 1, 1, 32, 0.125, None) == -1      # hd 64 only


def test_msa_zero_alone_equals_msa_zero_in_a_batch():
    B, R, L, H = 3, 5, 70, 2
    ids = _ids(B, R, L, [70, 41, 64], [5, 3, 4])
    qkv = _qkv(B, R, L, H, 5)
    S3, r3 = _row(qkv, ids, H)
    c3 = _col(qkv, ids, H)
    n = R * L
    S1, r1 = _row(qkv[:n].contiguous(), ids[:1], H)
    c1 = _col(qkv[:n].contiguous(), ids[:1], H)
    assert torch.equal(S3[:1], S1) and torch.equal(r3[:n], r1) and torch.equal(c3[:n], c1)


def test_embed_vs_fp64():
    from oneprot_amd import hip
    B, R, L, d, V, max_pos, rows_tab = 2, 3, 33, 128, 33, 40, 8
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(4, 30, (B, R, L), generator=g)
    tok[:, :, 0] = 0
    tok[1, :, 20:] = 1
    tok[1, 2] = 1
    tok[0, 1, 9] = tok[0, 1, 10] = tok[0, 2, 31] = 1                      # interior padding: the positions behind it do not count it
    sd = {"embed_tokens.weight": torch.randn(V, d, generator=g) * 0.05, "embed_positions.weight": torch.randn(max_pos + 2, d, generator=g) * 0.05,
          "msa_position_embedding": torch.randn(1, rows_tab, 1, d, generator=g) * 0.05, "emb_layer_norm_before.weight": 1 + 0.1 * torch.randn(d, generator=g),
          "emb_layer_norm_before.bias": 0.1 * torch.randn(d, generator=g)}
    x = torch.full((B * R * L, d), float("nan"), device=DEV)
    a = [sd[k].to(DEV).contiguous() for k in sd]
    hip.call("oneprot_msa_embed_fwd", tok.to(DEV), *a, x, B, R, L, d, V, max_pos + 2, rows_tab, 1, 1e-5)
    torch.cuda.synchronize()
    ref = MR.embed(tok, {k: v.to(F64) for k, v in sd.items()})
    close(x.view(B, R, L, d), ref, 1e-5, 1e-5, "msa embed")
    assert bool((x.view(B, R, L, d)[tok.eq(1).to(DEV)] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- tower / encoder
@pytest.mark.parametrize("pooling,proj", [("mean", "linear"), ("cls", "mlp")])
@pytest.mark.parametrize("use_all_msa", [True, False])
@pytest.mark.parametrize("shape,lens,rows", E2E, ids=[str(c[0]) for c in E2E])
def test_msa_encoder_vs_restatement(tmp_path, shape, lens, rows, use_all_msa, pooling, proj):
    from src.models.components.msa_encoder import MsaEncoder
    scale = proj == "mlp"
    enc = MsaEncoder(_checkpoint(tmp_path), output_dim=64, pooling_type=pooling, proj_type=proj, use_logit_scale=scale, use_all_msa=use_all_msa)
    assert enc.d_model == 128 and not enc.transformer.training
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    enc = enc.to(DEV)
    tok = _tokens(*shape, lens, rows, 9)
    with torch.no_grad():
        feats = enc(tok.to(DEV)).cpu()
        hidden = enc.transformer(tok.to(DEV))["representations"][2].cpu()
    assert torch.isfinite(hidden).all() and torch.isfinite(feats).all()
    ref_h, ref_f = MR.encoder_features(tok, sd, 2, use_all_msa, pooling)
    mask = tok.ne(1).unsqueeze(-1).to(F64)
    err = ((hidden.to(F64) - ref_h) * mask).abs().max()
    cs = torch.nn.functional.cosine_similarity(feats.to(F64), ref_f, dim=-1)
    print(f"hidden max err {float(err):.3e} of {float(ref_h.abs().max()):.3e}; cosine {float(cs.min()):.6f}")
    assert err < 0.05 * ref_h.abs().max()
    assert cs.min() > 0.999, cs
    assert abs(feats.norm(dim=-1) - (1 / 0.07 if scale else 1.0)).max() < 1e-3


def test_grouping_leaves_attention_outputs_bit_identical(tmp_path, monkeypatch):
    from oneprot_amd.msa import MsaTransformer, plan_groups
    tr = MsaTransformer.from_pretrained(_checkpoint(tmp_path)).to(DEV)
    tok = _tokens(3, 4, 50, [50, 31, 45], [4, 2, 3], 2).to(DEV)
    outs = []
    for budget in (None, "1"):
        if budget is None:
            monkeypatch.delenv("ONEPROT_MSA_SCORE_BYTES", raising=False)
        else:
            monkeypatch.setenv("ONEPROT_MSA_SCORE_BYTES", budget)
        assert len(plan_groups(3, 4, 50, 2)) == (1 if budget is None else 3)
        tr.capture = []
        x, _ = tr.run_layers(tok)
        torch.cuda.synchronize()
        outs.append((tr.capture, x.clone()))
        tr.capture = None
    assert len(outs[0][0]) == 4
    for (ka, ia, a), (kb_, ib, b) in zip(outs[0][0], outs[1][0]):
        assert (ka, ia) == (kb_, ib) and torch.equal(a, b), (ka, ia)
    assert torch.equal(outs[0][1], outs[1][1])


def test_module_training_step_with_frozen_msa_tower(tmp_path):
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    warnings.filterwarnings("ignore", message=".*no weight file.*")
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.optim import FusedAdam
    from src.models.components.msa_encoder import MsaEncoder
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.oneprot_module import OneProtLitModule
    torch.manual_seed(0)
    seq = SequenceEncoder("facebook/esm2_t6_8M_UR50D", output_dim=64, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
    msa = MsaEncoder(_checkpoint(tmp_path), output_dim=64, pooling_type="mean", proj_type="mlp", use_logit_scale=True, use_all_msa=True)
    module = OneProtLitModule(components={"sequence": seq, "msa": msa}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP").to(DEV)
    assert hasattr(msa.transformer, "_rng_uid")
    before = msa.transformer.flat.detach().clone()
    batch = next(iter(SyntheticPairs("msa", 4, 32, 48, msa_depth=5, ragged=True, device=DEV)))
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
