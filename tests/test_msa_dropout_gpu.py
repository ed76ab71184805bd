"""The MSA tower's train-mode dropout on the GPU: oneprot_msa_row_context_dropout and oneprot_msa_col_attn_dropout against the fp64 restatement handed
the masks rebuilt on the host (tests/msa_dropout_ref.py, tests/philox_ref.py), the tower with every site's mask rebuilt, determinism and the stream state,
and the proof that nothing moves while the switch is off.

Tolerances are those of tests/test_msa_gpu.py: bf16 outputs rtol 2^-7, atol 2e-2; any non-finite value fails, padded positions included.  Every comparison
with a masked reference carries a guard against a vacuous pass: the masked reference must differ from the unmasked one by more than the tolerance at half
of the unpadded elements at least (the tower test: by more than its gate), or a kernel that ignores its mask would pass too.  The inputs are those of
tests/test_msa_gpu.py (bf16-rounded randn), except for the two long row cases (L = 257, 1024), where q is scaled by LONG_Q_GAIN = 4: a softmax of unit-variance
scores over several hundred keys is so flat that dropping a tenth of it moves a context value by less than the tolerance (L = 1024: about 0.017 against 0.02;
the guard's share is 0.49 at L = 257 and 0.17 at L = 1024 for p = 0.1), which says nothing about the kernel.  With the gain the shares are 0.77 and 0.72.
Shares of the reference alone, computed without a device: row cases 0.59 - 0.77 at p = 0.1 and 0.88 - 0.97 at p = 0.5; column cases 0.64 - 0.86 and
0.90 - 0.98 (R = 33 and the L = 1 cases included: none needed another stream id).
Parity with fair-esm itself is unpinned (see tests/msa_ref.py)."""
import functools
import math
import os
import warnings

import pytest
import torch

from tests import msa_dropout_ref as DR
from tests import msa_ref as MR
from tests import msa_cases as MC
from tests.gate import close
from tests.msa_cases import DEV, F64

pytestmark = pytest.mark.gpu
RTOL, ATOL = 2 ** -7, 2e-2
SEED = 0x1234567
UID = 7                                                   # a tower id for the stream ids of the kernel tests
LONG_Q_GAIN = 4.0


def _stream(local):
    return (3 << 60) | (UID << 44) | local


def _qkv(B, R, L, H, seed, q_gain=1.0):
    """test_msa_gpu._qkv (the same numbers at gain 1) with q scaled by q_gain before the one rounding to bf16"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * R * L, 3 * H * 64, generator=g)
    x[:, :H * 64] *= q_gain
    return x.to(torch.bfloat16)


def _moved_share(masked, plain, pad):
    """share of the unpadded elements [B, R, L, :] at which the masked reference leaves the tolerance band of the unmasked one"""
    moved = (masked - plain).abs() > ATOL + RTOL * plain.abs()
    live = (~pad)[..., None].expand_as(moved)
    return float(moved[live].double().mean())


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the row kernel
ROW_CASES = [c for c in MC.ROW_CASES if c[0] != (1, 1, 5, 1)]


def _row_inputs(shape, lens, rows, holes):
    B, R, L, H = shape
    return MC._ids(B, R, L, lens, rows, holes), _qkv(B, R, L, H, 11 + L, LONG_Q_GAIN if L > 130 else 1.0)


def _row_refs(ids, qkv, H, p, stream):
    """(fp64 context with the host mask, fp64 context without a mask)"""
    B, R, L = ids.shape
    pad = ids.eq(1)
    q, k, v = MC._split(qkv, B, R, L, H)
    S64 = MR.row_scores(q, k, pad, H)
    return DR.row_context(S64, v, pad, H, DR.row_mask(B, H, L, p, SEED, stream)), MR.row_context(S64, v, pad, H)


def _row_drop(qkv, ids, H, p, stream, b_first=0, S=None):
    from oneprot_amd import hip
    B, R, L = ids.shape
    kb, qd = MC._key_bias(ids), qkv.to(DEV)
    if S is None:
        S = torch.empty(B, H, L, L, dtype=torch.float32, device=DEV)
        hip.call("oneprot_msa_row_scores", qd, kb, S, B, R, L, H, 64, 64 ** -0.5 / math.sqrt(R))
    ctx = torch.empty(B * R * L, H * 64, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(hip.query("oneprot_msa_row_context_workspace", B, R, L, H), dtype=torch.uint8, device=DEV)
    hip.call("oneprot_msa_row_context_dropout", S, qd, kb, ctx, ws, ws.numel(), B, R, L, H, 64, b_first, p, SEED, stream)
    torch.cuda.synchronize()
    return S, ctx


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape,lens,rows,holes", ROW_CASES, ids=[str(c[0]) for c in ROW_CASES])
def test_row_context_dropout_vs_fp64_with_the_host_mask(shape, lens, rows, holes, p):
    B, R, L, H = shape
    ids, qkv = _row_inputs(shape, lens, rows, holes)
    c_drop, c_eval = _row_refs(ids, qkv, H, p, _stream(5))
    share = _moved_share(c_drop, c_eval, ids.eq(1))
    print(f"row {shape} p={p}: the mask moves {share:.2f} of the unpadded elements out of the tolerance")
    assert share >= 0.5
    _, ctx = _row_drop(qkv, ids, H, p, _stream(5))
    close(ctx.view(B, R, L, H * 64), c_drop, RTOL, ATOL, f"row ctx dropout {shape} p={p}")


def test_row_b_first_places_the_mask_in_the_batch():
    shape, lens, rows, holes = MC.ROW_CASES[1]            # (2, 3, 33, 2)
    B, R, L, H = shape
    ids, qkv = _row_inputs(shape, lens, rows, holes)
    _, both = _row_drop(qkv, ids, H, 0.1, _stream(5))
    n = R * L
    one = lambda b_first: _row_drop(qkv[n:].contiguous(), ids[1:], H, 0.1, _stream(5), b_first=b_first)[1]
    assert torch.equal(one(1), both[n:])
    assert not torch.equal(one(0), both[n:])


# ---------------------------------------------------------------------------------------------------------------- 3: the column kernel
COL_STREAM = {}                                           # (R, L, p) -> stream id where the default's guard share falls short of 0.5 (none does)


def _col_inputs(R, L):
    B, H = 2, 2
    ids = MC._ids(B, R, L, [L, L], [R - R // 3, max(R // 2, 1)])          # the padding of test_col_attn_vs_fp64: trailing rows fully padded
    ids[1, :, L - 1] = 1                                                  # one column with every key masked
    return ids, _qkv(B, R, L, H, 100 * R + L)


def _col_refs(ids, qkv, H, p, stream):
    B, R, L = ids.shape
    pad = ids.eq(1)
    q, k, v = MC._split(qkv, B, R, L, H)
    return DR.col_context(q, k, v, pad, H, DR.col_mask(B, H, L, R, p, SEED, stream), general=True), MR.col_context(q, k, v, pad, H, general=True)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("L", [1, 33])
@pytest.mark.parametrize("R", [2, 17, 33, 50, 128])
def test_col_attn_dropout_vs_fp64_with_the_host_mask(R, L, p):
    from oneprot_amd import hip
    B, H = 2, 2
    ids, qkv = _col_inputs(R, L)
    stream = COL_STREAM.get((R, L, p), _stream(6))
    c_drop, c_eval = _col_refs(ids, qkv, H, p, stream)
    pad = ids.eq(1)
    live = (~pad).any(dim=1)                                              # [B, L]: columns with at least one key
    assert not bool(live[1, L - 1])
    share = _moved_share(c_drop, c_eval, pad)
    print(f"col R={R} L={L} p={p}: the mask moves {share:.2f} of the unpadded elements out of the tolerance")
    assert share >= 0.5
    ctx = torch.empty(B * R * L, H * 64, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_msa_col_attn_dropout", qkv.to(DEV), MC._key_bias(ids), ctx, B, R, L, H, 64, 64 ** -0.5, p, SEED, stream)
    torch.cuda.synchronize()
    ctx = ctx.view(B, R, L, H * 64)
    assert torch.isfinite(ctx).all()
    sel = live[:, None, :, None].expand_as(c_drop)
    close(torch.where(sel.to(DEV), ctx.float(), torch.zeros((), device=DEV)), torch.where(sel, c_drop, torch.zeros((), dtype=F64)), RTOL, ATOL,
          f"col ctx dropout R={R} L={L} p={p}")


# ---------------------------------------------------------------------------------------------------------------- 4: p = 0 and the refusals
def test_p_zero_equals_the_undropped_calls_and_bad_arguments_are_refused():
    from oneprot_amd import hip
    shape, lens, rows, holes = MC.ROW_CASES[1]
    B, R, L, H = shape
    ids, qkv = _row_inputs(shape, lens, rows, holes)
    S, plain = MC._row(qkv, ids, H)
    for p in (0.0, 2.0 ** -18):                           # below 2^-17: thr16 = 0, no dropout at all
        assert torch.equal(_row_drop(qkv, ids, H, p, _stream(5), S=S)[1], plain)
    ids_c, qkv_c = _col_inputs(17, 33)
    kb, qd = MC._key_bias(ids_c), qkv_c.to(DEV)
    got = torch.empty(2 * 17 * 33, 128, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_msa_col_attn_dropout", qd, kb, got, 2, 17, 33, 2, 64, 0.125, 0.0, SEED, _stream(6))
    torch.cuda.synchronize()
    assert torch.equal(got, MC._col(qkv_c, ids_c, 2))
    # refusals, each before any launch: the outputs keep their contents
    h = hip.lib()
    kbr, qr = MC._key_bias(ids), qkv.to(DEV)
    ctx = torch.full((B * R * L, H * 64), 3.0, dtype=torch.bfloat16, device=DEV)
    ws = torch.full((hip.query("oneprot_msa_row_context_workspace", B, R, L, H),), 7, dtype=torch.uint8, device=DEV)
    row = lambda p, b_first, B_=B: h.oneprot_msa_row_context_dropout(S.data_ptr(), qr.data_ptr(), kbr.data_ptr(), ctx.data_ptr(), ws.data_ptr(), ws.numel(), B_, R, L,
                                                                     H, 64, b_first, p, SEED, _stream(5), None)
    for p in (-0.1, float("nan"), 1.0, 1.5):
        assert row(p, 0) == -1, p
    assert row(0.1, -1) == -1
    assert row(0.1, 65535 // H - B + 1) == -1 and row(0.0, 65535 // H - B + 1) == -1      # (b_first + B) * H > 65535
    col = lambda p, R_: h.oneprot_msa_col_attn_dropout(qd.data_ptr(), kb.data_ptr(), got.data_ptr(), 2, R_, 33, 2, 64, 0.125, p, SEED, _stream(6), None)
    before = got.clone()
    for p in (-0.1, float("nan"), 1.0):
        assert col(p, 17) == -1, p
    assert col(0.1, 1) == -1 and col(0.1, 129) == -1      # R = 1 is the host's shortcut: no probabilities to drop
    torch.cuda.synchronize()
    assert bool((ctx == 3.0).all()) and bool((ws == 7).all()) and torch.equal(got, before)


# ---------------------------------------------------------------------------------------------------------------- 5: the tower
def _encoder(tmp_path, use_all_msa=True, pooling="mean", proj="linear"):
    from src.models.components.msa_encoder import MsaEncoder
    enc = MsaEncoder(MC._checkpoint(tmp_path), output_dim=64, pooling_type=pooling, proj_type=proj, use_all_msa=use_all_msa)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    return enc.to(DEV), sd


def _masks(tr, call, shape, seed):
    return DR.tower_masks(functools.partial(tr._drop_stream, call), shape, tr.d, tr.f, tr.H, tr.n_layers, tr._drop_probs(), seed)


@pytest.mark.parametrize("shape,lens,rows", MC.E2E, ids=[str(c[0]) for c in MC.E2E])
def test_tower_dropout_vs_restatement_with_every_mask_rebuilt(tmp_path, shape, lens, rows):
    """The gates of test_msa_encoder_vs_restatement.  The encoder's features are taken from row 0 / position 0 (cls): a mean over every token would average
    the dropout away and the guard on the features could not tell a tower that ignores its masks."""
    enc, sd = _encoder(tmp_path, use_all_msa=False, pooling="cls")
    tr = enc.transformer
    tok = MC._tokens(*shape, lens, rows, 9)
    tr.set_rng_state({"_drop_seed": SEED, "_drop_calls": 0})
    enc.train_dropout = True
    enc.train()
    assert enc.training and not tr.training
    with torch.no_grad():
        feats = enc(tok.to(DEV)).cpu()                                                    # call 0
        hidden = tr(tok.to(DEV), drop=True)["representations"][2].cpu()                   # call 1
    assert tr.rng_state()["_drop_calls"] == 2
    assert torch.isfinite(hidden).all() and torch.isfinite(feats).all()
    tr_sd = {k[len("transformer."):]: v for k, v in sd.items() if k.startswith("transformer.")}
    _, ref_f = DR.encoder_features(tok, sd, 2, False, "cls", _masks(tr, 0, shape, SEED))
    masks = _masks(tr, 1, shape, SEED)
    ref_h = DR.forward(tok, tr_sd, 2, masks)
    eval_h, eval_f = MR.encoder_features(tok, sd, 2, False, "cls")
    mask = tok.ne(1).unsqueeze(-1).to(F64)
    gate = 0.05 * ref_h.abs().max()
    cos = lambda a, b: torch.nn.functional.cosine_similarity(a.to(F64), b, dim=-1)
    moved, cs_moved = ((ref_h - eval_h) * mask).abs().max(), cos(ref_f, eval_f)
    err, cs = ((hidden.to(F64) - ref_h) * mask).abs().max(), cos(feats, ref_f)
    print(f"{shape}: hidden max err {float(err):.3e} (gate {float(gate):.3e}; the masks move the reference by {float(moved):.3e}); "
          f"cosine {float(cs.min()):.6f} (dropped vs eval reference {float(cs_moved.max()):.6f})")
    assert moved > gate and cs_moved.max() < 0.999       # a tower that ignored its masks would fail both gates below
    if shape[1] == 1:
        # one row: the column block is out_proj(v_proj(x)) with no probability mask (the masks hold none for site 2) but WITH its residual dropout
        assert not any(site == 2 for _, site in masks)
        no3 = {k: v for k, v in masks.items() if k[1] != 3}
        assert ((DR.forward(tok, tr_sd, 2, no3) - ref_h) * mask).abs().max() > 2 * gate
    assert err < gate
    assert cs.min() > 0.999, cs


# ---------------------------------------------------------------------------------------------------------------- 6: determinism and state
def test_same_seed_and_call_repeat_bit_for_bit_and_the_state_restores(tmp_path, monkeypatch):
    from oneprot_amd.msa import MsaTransformer, plan_groups
    tr = MsaTransformer.from_pretrained(MC._checkpoint(tmp_path)).to(DEV)
    tok = MC._tokens(3, 4, 50, [50, 31, 45], [4, 2, 3], 2).to(DEV)
    monkeypatch.delenv("ONEPROT_MSA_SCORE_BYTES", raising=False)

    def run():
        x, _ = tr.run_layers(tok, drop=True)
        torch.cuda.synchronize()
        return x.clone()

    tr.set_rng_state({"_drop_seed": SEED, "_drop_calls": 0})
    a0 = run()
    state = tr.rng_state()
    assert state["_drop_seed"] == SEED and state["_drop_calls"] == 1
    a1 = run()
    assert torch.isfinite(a0).all() and not torch.equal(a0, a1)                           # the next call draws other masks
    tr.set_rng_state({"_drop_seed": SEED, "_drop_calls": 0})
    assert torch.equal(run(), a0)                                                         # same seed, same call id
    tr.set_rng_state(state)
    assert torch.equal(run(), a1)                                                         # the state taken after call 0 reproduces call 1
    tr.set_rng_state({"_drop_seed": SEED + 1, "_drop_calls": 0})
    assert not torch.equal(run(), a0)
    # grouping: one MSA per group (b_first = 0, 1, 2 through the host) against all three in one call
    assert len(plan_groups(3, 4, 50, 2)) == 1
    monkeypatch.setenv("ONEPROT_MSA_SCORE_BYTES", "1")
    assert len(plan_groups(3, 4, 50, 2)) == 3
    tr.set_rng_state({"_drop_seed": SEED, "_drop_calls": 0})
    assert torch.equal(run(), a0)


# ---------------------------------------------------------------------------------------------------------------- 7: nothing moves by default
def test_default_is_untouched_and_the_switch_needs_train_mode(tmp_path, monkeypatch):
    monkeypatch.delenv("ONEPROT_MSA_DROPOUT", raising=False)
    enc, _ = _encoder(tmp_path)
    tr = enc.transformer
    tok = MC._tokens(2, 5, 70, [70, 44], [5, 3], 9).to(DEV)
    pooled = lambda: enc.hidden_and_pooled(tok, want_hidden=False)[1].clone()
    enc.train()
    assert enc.training and not tr.training
    off_train = pooled()
    enc.eval()
    off_eval = pooled()
    assert torch.equal(off_train, off_eval) and tr.rng_state() == {}                      # no call id was drawn
    with torch.no_grad():
        x, _ = tr.run_layers(tok)
        y, _ = tr.run_layers(tok, drop=False)
    assert torch.equal(x, y)
    for on in ("env", "attr"):
        if on == "env":
            monkeypatch.setenv("ONEPROT_MSA_DROPOUT", "1")
        else:
            monkeypatch.delenv("ONEPROT_MSA_DROPOUT")
            enc.train_dropout = True
        enc.train()
        assert not tr.training
        a, b = pooled(), pooled()
        assert torch.isfinite(a).all() and not torch.equal(a, b) and not torch.equal(a, off_eval)
        enc.eval()
        assert torch.equal(pooled(), off_eval) and not tr.training
    enc.train_dropout = False
    enc.train()
    assert torch.equal(pooled(), off_eval)


def test_module_training_step_with_the_switch_on(tmp_path):
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    warnings.filterwarnings("ignore", message=".*no weight file.*")
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.optim import FusedAdam
    from src.models.components.msa_encoder import MsaEncoder
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.oneprot_module import OneProtLitModule
    torch.manual_seed(0)
    seq = SequenceEncoder("facebook/esm2_t6_8M_UR50D", output_dim=64, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
    msa = MsaEncoder(MC._checkpoint(tmp_path), output_dim=64, pooling_type="mean", proj_type="mlp", use_logit_scale=True, use_all_msa=True)
    msa.train_dropout = True
    module = OneProtLitModule(components={"sequence": seq, "msa": msa}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP").to(DEV)
    before = msa.transformer.flat.detach().clone()
    batch = next(iter(SyntheticPairs("msa", 4, 32, 48, msa_depth=5, ragged=True, device=DEV)))
    module.train()
    assert msa.training and not msa.transformer.training
    loss = module.training_step({"msa": batch}, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert msa.transformer.rng_state()["_drop_calls"] >= 1                                # the step ran the dropped forward
    assert all(p.grad is None for p in msa.transformer.parameters())
    assert torch.equal(msa.transformer.flat.detach(), before)
    assert any(p.grad is not None for p in msa.proj.parameters())
    ck = {}
    module.on_save_checkpoint(ck)
    assert ck["oneprot_amd_dropout_rng"]["msa"]["_drop_calls"] == msa.transformer.rng_state()["_drop_calls"]
