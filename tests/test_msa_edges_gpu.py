"""The MSA kernels (csrc/msa.hip) at every edge and the tower (oneprot_amd/msa.py) stage by stage, against the fp64 restatement tests/msa_ref.py on the bf16-rounded
inputs the kernels read.  tests/test_msa_gpu.py, written with the kernels, stops at H = 2, d = 128, randn scores, L off every tile edge and a 5 % end-to-end gate.

  1 edges: row attention at L on, one below and one above every tile size (16 / 32 / 64 / 128 / 256), at L = 1024 with its last key live and at the published
    12 heads (QKV row pitch 2304); column attention at 12 heads (its R edges are in test_msa_gpu.test_col_attn_vs_fp64); the embedding past column 64, at
    d = 100 / 768 / 2048 and with the position table exactly as long as needed; every refusal of the entry points on the host.
  2 scores of a trained tower: q multiplied by 60 to 100, |S| beyond 150 (asserted), a softmax that is close to one-hot.
  3 masks as equalities, no reference: +-1000 planted where the result must not depend on it, torch.equal on the output.
  4 the tower stage by stage: embedding, QKV, attention, out-projection, FFN, each against fp64 from that stage's OWN captured input (MsaTransformer.stages), so
    that drift cannot hide a stage's error.  The 5 % gate of test_msa_encoder_vs_restatement is the drift budget, not the correctness check.

Gates are the module's (tests/test_gemm_small_shapes_gpu.py): fp32 outputs rtol 1e-4, atol 1e-3 * sqrt(K / 64) -- K = R * 64 for the tied scores, d for the
out-projection, f for the FFN --; bf16 outputs rtol 2^-7, atol 2e-2; the embedding 1e-5 / 1e-5; per element, a non-finite value anywhere fails.
Parity with fair-esm itself is still unpinned (tests/msa_ref.py).

One FFN gate is the measured one, by the rule that a correct tower may miss the fp32 gate of that stage only through bf16 tie flips and that the allowance is then four
times the reference's own difference, never a guess.  The 2-layer d = 128 model (f = 256: atol 2.0e-3) on the (3, 4, 50) batch of test_tower_stages_one_msa_per_group
missed it: 2.155e-3 at one element of 76 800 in layer 0, 2.426e-3 in layer 1.  The tower's LayerNorm is fp32, the reference's fp64; of 76 800 LayerNorm outputs one or two lie
so close to a bf16 tie that the two round apart, and one flip (2^-7 of a value near 3) moves a whole token row of the FFN output.  Measured on the CPU, same weights and
tokens (MR.ffn_rounding_self_difference: bf16-rounded LayerNorm and GELU outputs against exact ones): 9.44e-3 (layer 0), 7.52e-3 (layer 1); that test alone runs its FFN
stage at atol 4 * 9.44e-3, rtol 1e-4 as everywhere.  The other two tower tests keep the plain gate: (1, 1, 40) measured 1.08e-3 / 3.9e-4 against 2.0e-3, the published
width 5.63e-3 against 6.93e-3.

Mutations these tests were run against (one at a time, on a copy of the tree, value / in-bounds index changes only; "before" = tests/test_msa_gpu.py as it
was before this file, 35 tests, plus the twelve R values its column sweep gained here; "new" = this file):
  1 k_msa_row_pv and k_msa_col_attn: the ctx store's head offset h * 64 -> (h & 1) * 64
      before: nothing (H <= 2 everywhere); new: both published-head-count row cases, the 12-head column case, the 12-head near-one-hot row and column
      cases, the published-width tower at "layer 0 row ctx" (172530 / 184320 elements off)
  2 k_msa_row_softmax and k_msa_col_attn: no max subtraction (m = 0 after the reduction)
      before: nothing (randn scores); new: all eight near-one-hot cases (non-finite ctx)
  3 k_msa_embed: the count loop bound j <= l -> j <= min(l, 63)
      before: not the kernel test (L = 33), but the four end-to-end cases at L = 70; new: the embedding at L = 65 (400 / 39000 off), 130 and 1024; L = 64 passes, as it must
  4 msa.py: row_scale from the number of non-empty rows of MSA 0 instead of the padded R
      before: nothing (MSA 0 is full in every tower test); new: the grouped tower at "layer 0 row ctx" (26819 / 76800 off, max err 0.585)
  5 k_msa_row_softmax: j < L -> j < L && j < 1023
      before: nothing (the L = 1024 case masks keys 1000 .. 1023); new: the longest row.  With plain randn inputs that test caught it at 8 of 131072 elements
      only (max err 2.98e-2 against 2e-2: one key of 1024 carries little), so it now makes the last key the heavy one (k times 8): 39099 / 131072 off, max err 3.17
"""
import math

import pytest
import torch

from tests import msa_ref as MR
from tests.gate import close
from tests.msa_cases import DEV, F64, FFN_SELF_DIFFERENCE_GROUPED, GROUPED, _checkpoint, _col, _ids, _qkv, _row, _split, _tokens, bf

pytestmark = pytest.mark.gpu
BF16_GATE = (2 ** -7, 2e-2)


def f32_gate(K):
    return 1e-4, 1e-3 * math.sqrt(K / 64)


def _check_row(shape, ids, qkv):
    """S and ctx of the two row entry points against fp64, every head and every position; -> the reference S"""
    B, R, L, H = shape
    S, ctx = _row(qkv, ids, H)
    pad = ids.eq(1)
    assert not bool(pad[:, 0].all(dim=1).any())                          # row 0 holds a key in every MSA: excluded and -10000-biased keys are the same thing
    q, k, v = _split(qkv, B, R, L, H)
    S64 = MR.row_scores(q, k, pad, H)
    close(S, S64, *f32_gate(R * 64), f"S {shape}")
    close(ctx.view(B, R, L, H * 64), MR.row_context(S64, v, pad, H), *BF16_GATE, f"row ctx {shape}")
    return S64


def _check_col(shape, ids, qkv):
    """ctx of the column attention against fp64 at every position of every column that has a key"""
    B, R, L, H = shape
    ctx = _col(qkv, ids, H).view(B, R, L, H * 64)
    assert torch.isfinite(ctx).all()
    pad = ids.eq(1)
    q, k, v = _split(qkv, B, R, L, H)
    c64 = MR.col_context(q, k, v, pad, H, general=True)
    sel = (~pad).any(dim=1)[:, None, :, None].expand_as(c64)
    zero = torch.zeros((), dtype=F64)
    close(torch.where(sel, ctx.cpu().to(F64), zero), torch.where(sel, c64, zero), *BF16_GATE, f"col ctx {shape}")
    return q, k


# ---------------------------------------------------------------------------------------------------------------- 1. kernel edges
@pytest.mark.parametrize("L", [1, 16, 17, 31, 32, 63, 64, 65, 127, 128, 129, 255, 256])
def test_row_attention_at_every_tile_edge(L):
    """16 = MFMA tile, 32 = Lp and the P . V trip, 64 = a wave's quadrant / the softmax stride / the P . V query block, 128 = the score tile: L on each,
    one below, one above.  MSA 0 is full length (the last key is live), MSA 1 ends off every tile edge."""
    ids = _ids(2, 2, L, [L, L - min(5, L - 1)], [2, 2])
    _check_row((2, 2, L, 1), ids, _qkv(2, 2, L, 1, 300 + L))


def test_row_attention_longest_row_all_keys_live():
    """k of the last column times 8 (exact in bf16): key 1023 takes most of the probability of about half of the queries, so a softmax that drops it cannot pass"""
    from oneprot_amd import hip
    L = hip.MSA_MAX_LEN
    assert L == 1024
    qkv = _qkv(1, 2, L, 1, 77)
    qkv.view(2, L, 3, 64)[:, L - 1, 1] *= 8
    _check_row((1, 2, L, 1), _ids(1, 2, L, [L], [2]), qkv)


HEAD_CASES = [((2, 3, 33, 12), [33, 20], [3, 2], ((0, 2, 7),)), ((1, 5, 130, 12), [130], [3], ((0, 2, 7), (0, 0, 129)))]


@pytest.mark.parametrize("shape,lens,rows,holes", HEAD_CASES, ids=[str(c[0]) for c in HEAD_CASES])
def test_row_attention_published_head_count(shape, lens, rows, holes):
    B, R, L, H = shape
    _check_row(shape, _ids(B, R, L, lens, rows, holes), _qkv(B, R, L, H, 500 + L))


def test_col_attn_published_head_count():
    shape = B, R, L, H = 3, 17, 5, 12
    ids = _ids(B, R, L, [L] * B, [17, 9, 2])
    ids[1, :, L - 1] = 1                                                  # one column with every key masked
    _check_col(shape, ids, _qkv(B, R, L, H, 41))


EMBED_CASES = [(64, 128, 9), (65, 100, 9), (130, 768, 9), (1024, 2048, 0)]   # (L, d, spare rows of the position table)


@pytest.mark.parametrize("L,d,spare", EMBED_CASES, ids=[f"L{c[0]}-d{c[1]}" for c in EMBED_CASES])
def test_embed_edges(L, d, spare):
    """the per-row position count takes its second trip from column 64 on; d off a multiple of 64, at the published 768 and at the kernel's limit 64 * EMB_MAXV;
    the last case needs every row of its position table (n_pos = L + pad + 1)"""
    from oneprot_amd import hip
    B, R, V, rows_tab, n_pos = 2, 3, 33, 8, L + 2 + spare
    g = torch.Generator().manual_seed(L + d)
    tok = torch.randint(4, 30, (B, R, L), generator=g)
    tok[:, :, 0] = 0
    for r, c in ((1, 9), (1, 10), (1, 40), (2, 63), (1, 66), (1, 67), (2, 65), (1, 100)):      # interior padding on both sides of column 64 where L reaches
        if c < L - 1:
            tok[0, r, c] = 1
    tok[1, 0, L - 7:] = 1
    tok[1, 1, 3] = 1
    tok[1, 2] = 1                                                         # a fully padded row
    assert int(MR.positions(tok).max()) == L + 1 and (L < 65 or bool(tok[:, :, 64:].ne(1).any()))
    sd = {"embed_tokens.weight": torch.randn(V, d, generator=g) * 0.05, "embed_positions.weight": torch.randn(n_pos, d, generator=g) * 0.05,
          "msa_position_embedding": torch.randn(1, rows_tab, 1, d, generator=g) * 0.05, "emb_layer_norm_before.weight": 1 + 0.1 * torch.randn(d, generator=g),
          "emb_layer_norm_before.bias": 0.1 * torch.randn(d, generator=g)}
    x = torch.full((B * R * L, d), float("nan"), device=DEV)
    hip.call("oneprot_msa_embed_fwd", tok.to(DEV), *[sd[k].to(DEV).contiguous() for k in sd], x, B, R, L, d, V, n_pos, rows_tab, 1, 1e-5)
    torch.cuda.synchronize()
    x = x.view(B, R, L, d).cpu()
    close(x, MR.embed(tok, {k: v.to(F64) for k, v in sd.items()}), 1e-5, 1e-5, f"msa embed L={L} d={d}")
    assert bool((x[tok.eq(1)] == 0).all())


def test_refusals_on_the_host():
    """every shape, alignment and size refusal of the five entry points, through the bare library: the refused calls launch nothing (their buffers are still as
    large as they would have needed); the same calls with nothing wrong are then taken, so that each -1 is due to the one altered argument"""
    from oneprot_amd import hip
    h = hip.lib()
    f32, b16 = torch.float32, torch.bfloat16
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=DEV)
    R, L, LX = 2, 8, hip.MSA_MAX_LEN + 1
    LXp = (LX + 31) // 32 * 32
    qkv, kb, S, ctx = z(R * LX * 192 + 8, b16), z(R * LX, f32), z(LX * LX, f32), z(R * LX * 64, b16)
    ws = z(2 * (LX * LXp + R * 64 * LXp), torch.uint8)
    p = lambda t: t.data_ptr()
    scores = lambda q, r, l, hd: h.oneprot_msa_row_scores(q, p(kb), p(S), 1, r, l, 1, hd, 0.125, None)
    context = lambda q, n, r, l, hd: h.oneprot_msa_row_context(p(S), q, p(kb), p(ctx), p(ws), n, 1, r, l, 1, hd, None)
    col = lambda q, r, l: h.oneprot_msa_col_attn(q, p(kb), p(ctx), 1, r, l, 1, 64, 0.125, None)
    # L beyond ONEPROT_MSA_MAX_LEN
    assert scores(p(qkv), R, LX, 64) == -1
    assert h.oneprot_msa_row_context_workspace(1, R, LX, 1) == 0
    assert context(p(qkv), ws.numel(), R, LX, 64) == -1
    # hd 64 only
    assert scores(p(qkv), R, L, 32) == -1
    need = h.oneprot_msa_row_context_workspace(1, R, L, 1)
    assert 0 < need <= ws.numel()
    assert context(p(qkv), need, R, L, 32) == -1
    # a workspace one byte short
    assert context(p(qkv), need - 1, R, L, 64) == -1
    # qkv one element into a buffer: not 16-byte aligned
    off = p(qkv[1:])
    assert off == p(qkv) + 2 and p(qkv) % 16 == 0
    assert scores(off, R, L, 64) == -1 and context(off, need, R, L, 64) == -1 and col(off, R, L) == -1
    # one row: the column attention is the v projection, the caller's business
    assert col(p(qkv), 1, L) == -1
    # embedding: position table too short, more rows than the row table, d beyond 64 * EMB_MAXV
    D = 2049
    tok, tt, pt, rt, ga, be, x = torch.full((R * L,), 5, dtype=torch.int64, device=DEV), z(33 * D, f32), z((L + 2) * D, f32), z(8 * D, f32), z(D, f32), z(D, f32), z(R * L * D, f32)
    embed = lambda d, n_pos, n_rows: h.oneprot_msa_embed_fwd(p(tok), p(tt), p(pt), p(rt), p(ga), p(be), p(x), 1, R, L, d, 33, n_pos, n_rows, 1, 1e-5, None)
    assert embed(128, L + 1, 8) == -1
    assert embed(128, L + 2, R - 1) == -1
    assert embed(D, L + 2, 8) == -1
    # and the same calls with nothing wrong are taken
    assert embed(128, L + 2, R) == 0 and embed(2048, L + 2, R) == 0
    assert scores(p(qkv), R, L, 64) == 0 and context(p(qkv), need, R, L, 64) == 0 and col(p(qkv), R, L) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2. scores of a trained tower
HOT_CASES = [((1, 3, 70, 2), 100.0), ((1, 50, 70, 2), 60.0), ((2, 5, 130, 12), 80.0), ((1, 2, 257, 1), 60.0)]      # (B, R, L, H), factor on q
HOT_IDS = [str(c[0]) for c in HOT_CASES]


def _hot(shape, amp):
    """randn with the q third multiplied by `amp` before the bf16 rounding: scores with a standard deviation of about `amp`; three trailing keys padded"""
    B, R, L, H = shape
    x = torch.randn(B * R * L, 3 * H * 64, generator=torch.Generator().manual_seed(7000 + R + L))
    x[:, :H * 64] *= amp
    return x.to(torch.bfloat16), _ids(B, R, L, [L - 3] * B, [R] * B)


@pytest.mark.parametrize("shape,amp", HOT_CASES, ids=HOT_IDS)
def test_row_attention_near_one_hot(shape, amp):
    """without the max subtraction exp(S) overflows from S = 88.7 on"""
    qkv, ids = _hot(shape, amp)
    smax = float(_check_row(shape, ids, qkv).abs().max())
    print(f"max |S| {smax:.1f}")
    assert smax > 150


@pytest.mark.parametrize("shape,amp", HOT_CASES, ids=HOT_IDS)
def test_col_attention_near_one_hot(shape, amp):
    qkv, ids = _hot(shape, amp)
    q, k = _check_col(shape, ids, qkv)
    valid = ~ids.eq(1).permute(0, 2, 1)                                   # [B, L, R]: of the compared columns, the keys that are not masked
    smax = float(MR.col_scores(q, k, shape[3]).abs()[valid[:, None, :, None, :].expand(-1, shape[3], -1, shape[1], -1)].max())
    print(f"max |S| {smax:.1f}")
    assert smax > 150


# ---------------------------------------------------------------------------------------------------------------- 3. masks as equalities
EQ_SHAPE = (2, 4, 70, 2)               # L = 70: Lp = 96, so P and V^T carry 26 columns past L


def _eq_ids(row0_holes=()):
    """MSA 0: four rows of 70 with a hole at (r = 2, i = 7) where row 0 holds a token; MSA 1: two rows of 41, a hole, and two fully padded rows"""
    B, R, L, _ = EQ_SHAPE
    return _ids(B, R, L, [70, 41], [4, 2], ((0, 2, 7), (1, 1, 5)) + tuple((0, 0, j) for j in row0_holes))


def _plant(qkv, thirds, where, seed, zero=False):
    """qkv with the q / k / v thirds `thirds` (0 / 1 / 2) set to +-1000 (exact in bf16), or to 0, at the tokens where[b, r, l]"""
    B, R, L, H = EQ_SHAPE
    x = qkv.clone().view(B, R, L, 3, H * 64)
    sign = torch.randint(0, 2, (B, R, L, H * 64), generator=torch.Generator().manual_seed(seed)) * 2 - 1
    val = (sign * (0 if zero else 1000)).to(torch.bfloat16)
    for t in thirds:
        x[:, :, :, t] = torch.where(where[..., None], val, x[:, :, :, t])
    return x.view(B * R * L, 3 * H * 64)


def test_q_of_padded_positions_counts_as_zero_bit_for_bit():
    B, R, L, H = EQ_SHAPE
    ids = _eq_ids()
    pad = ids.eq(1)
    assert bool(pad[0, 2, 7]) and not bool(pad[0, 0, 7]) and bool(pad[1, 2:].all())
    qkv = _qkv(B, R, L, H, 31)
    S_big, _ = _row(_plant(qkv, (0,), pad, 1), ids, H)
    S_zero, _ = _row(_plant(qkv, (0,), pad, 1, zero=True), ids, H)
    assert torch.isfinite(S_big).all() and float(S_zero.abs().max()) > 1
    assert torch.equal(S_big, S_zero)


def test_keys_row_zero_masks_leave_row_context_bit_identical():
    """k and v of EVERY row at the columns where row 0 is padded: their probabilities are exactly 0, and 0 * 1000 adds an exact 0 in the MFMA"""
    B, R, L, H = EQ_SHAPE
    ids = _eq_ids(row0_holes=(13, 66, 67, 68, 69))
    dead = ids.eq(1)[:, :1].expand(B, R, L)
    assert int(dead[0, 3].sum()) == 5 and int(dead[1, 0].sum()) == L - 41
    qkv = _qkv(B, R, L, H, 32)
    S_a, ctx_a = _row(qkv, ids, H)
    S_b, ctx_b = _row(_plant(qkv, (1, 2), dead, 2), ids, H)
    assert torch.isfinite(ctx_b).all() and not torch.equal(S_a, S_b)      # the planted keys did reach the kernel
    assert torch.equal(ctx_a, ctx_b)


def test_padded_column_keys_leave_column_context_bit_identical():
    B, R, L, H = EQ_SHAPE
    ids = _eq_ids()
    pad = ids.eq(1)
    qkv = _qkv(B, R, L, H, 33)
    ctx_a = _col(qkv, ids, H).view(B, R, L, H * 64)
    ctx_b = _col(_plant(qkv, (1, 2), pad, 3), ids, H).view(B, R, L, H * 64)
    live = (~pad).any(dim=1).to(DEV)                                      # [B, L]
    assert int(live.sum()) == 70 + 41 and torch.isfinite(ctx_b).all() and float(ctx_a.abs().max()) > 0.5
    sel = live[:, None, :, None].expand_as(ctx_a)
    assert torch.equal(ctx_a[sel], ctx_b[sel])


# ---------------------------------------------------------------------------------------------------------------- 4. the tower, stage by stage
WIDE = dict(layers=1, embed_dim=768, ffn_embed_dim=3072, attention_heads=12, max_positions=64, embed_positions_msa=True)      # one layer of the published width


def _wide_checkpoint(tmp_path):
    return _checkpoint(tmp_path, seed=1, arch=WIDE, name="msa_wide.pt", std=0.05)


def _check_stages(tr, tok, ffn_atol=None):
    """one run_layers with both hooks; then every stage of it against fp64 from the input the tower itself had at that stage.  ffn_atol: see the module docstring"""
    B, R, L = tok.shape
    d, f, H, n = tr.d, tr.f, tr.H, tr.n_layers
    tr.capture, tr.stages = [], []
    try:
        x, _ = tr.run_layers(tok.to(DEV))
        torch.cuda.synchronize()
        cap, st = [(k, i, t.cpu()) for k, i, t in tr.capture], [(k, i, t.cpu()) for k, i, t in tr.stages]
    finally:
        tr.capture = tr.stages = None
    att = ".v" if R == 1 else ".qkv"
    assert [(k, i) for k, i, _ in st] == [e for i in range(n) for e in (("row", i), ("row.qkv", i), ("col", i), ("col" + att, i), ("ffn", i))] + [("out", n)]
    assert [(k, i) for k, i, _ in cap] == [(k, i) for i in range(n) for k in ("row", "col")]
    assert torch.equal(st[-1][2], x.cpu())
    sd = MR.tower_operands(tr.state_dict(), bf)                            # the GEMMs read the bf16 mirror of their weights; LayerNorms, biases and tables stay fp32
    pad = tok.eq(1)
    assert not bool(pad[:, 0].all(dim=1).any())
    v4 = lambda t: t.to(F64).view(B, R, L, -1)
    zero = torch.zeros((), dtype=F64)
    close(v4(st[0][2]), MR.embed(tok, sd), 1e-5, 1e-5, "embedding")
    xs, ins = [s for s in st if "." not in s[0]], [s for s in st if "." in s[0]]
    a = 0
    for (kind, i, x_in), (_, _, x_next) in zip(xs, xs[1:]):
        x_in, x_next, tag = v4(x_in), v4(x_next), f"layer {i} {kind}"
        if kind == "ffn":
            close(x_next, MR.ffn(x_in, sd, i, rnd=bf), 1e-4, f32_gate(f)[1] if ffn_atol is None else ffn_atol, tag)
            continue
        blk = {"row": "row_self_attention", "col": "column_self_attention"}[kind]
        (name, _, t_in), (ck, ci, ctx) = ins[a], cap[a]
        a += 1
        assert (ck, ci) == (kind, i) and name.startswith(kind)
        proj = MR.qkv_proj(x_in, sd, i, blk, rnd=bf)
        if name.endswith(".v"):                                           # one row: the column attention is the v projection
            assert torch.equal(t_in, ctx)
            close(v4(ctx), proj[..., 2 * d:], *BF16_GATE, tag + " ctx = v_proj")
        else:
            close(v4(t_in), proj, *BF16_GATE, tag + " qkv")
            q, k, v = v4(t_in).chunk(3, dim=-1)
            if kind == "row":
                close(v4(ctx), MR.row_context(MR.row_scores(q, k, pad, H), v, pad, H), *BF16_GATE, tag + " ctx")
            else:
                sel = (~pad).any(dim=1)[:, None, :, None].expand(B, R, L, d)
                close(torch.where(sel, v4(ctx), zero), torch.where(sel, MR.col_context(q, k, v, pad, H), zero), *BF16_GATE, tag + " ctx")
        close(x_next, MR.attn_out(x_in, v4(ctx), sd, i, blk), *f32_gate(d), tag + " out-projection")
    assert a == len(ins) == len(cap)


def test_tower_stages_at_published_width(tmp_path):
    """d 768, 12 heads, FFN 3072: MSA 1 has fewer rows and columns, MSA 0 an interior hole"""
    from oneprot_amd.msa import MsaTransformer
    tr = MsaTransformer.from_pretrained(_wide_checkpoint(tmp_path)).to(DEV)
    assert (tr.n_layers, tr.d, tr.f, tr.H) == (1, 768, 3072, 12)
    tok = _tokens(2, 3, 40, [40, 29], [3, 2], 21)
    tok[0, 1, 17] = 1
    _check_stages(tr, tok)


def test_tower_stages_one_row(tmp_path):
    from oneprot_amd.msa import MsaTransformer
    tr = MsaTransformer.from_pretrained(_checkpoint(tmp_path)).to(DEV)
    _check_stages(tr, _tokens(1, 1, 40, [33], [1], 22))


def test_tower_stages_one_msa_per_group(tmp_path, monkeypatch):
    """ONEPROT_MSA_SCORE_BYTES=1: the row attention runs MSA by MSA on slices of kb, qkv and ctx.  MSA 0 holds two rows of the four: the tied scores are
    scaled by the PADDED row count"""
    from oneprot_amd.msa import MsaTransformer, plan_groups
    monkeypatch.setenv("ONEPROT_MSA_SCORE_BYTES", "1")
    assert len(plan_groups(3, 4, 50, 2)) == 3
    tr = MsaTransformer.from_pretrained(_checkpoint(tmp_path)).to(DEV)
    shape, lens, rows, seed = GROUPED
    _check_stages(tr, _tokens(*shape, lens, rows, seed), ffn_atol=4 * FFN_SELF_DIFFERENCE_GROUPED)
