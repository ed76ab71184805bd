"""Packed (variable-length) ESM batches on the MI355X: the varlen kernels through the C ABI against fp32 torch, the packed encoders against the
reference's goldens, and packed against padded on identical data."""
import functools
import json
import math
import os

import pytest
import torch

from oneprot_amd import hip
from oneprot_amd.packing import PackedTokens

pytestmark = pytest.mark.gpu

from oracle import oneprot_oracle as O  # noqa: E402
from tests.cases import cu as cu_of, esm_dir, gathered_tables, golden_pair_module, pack_shape, rope_half  # noqa: E402
from tests.gate import cos_sim  # noqa: E402

DEV = "cuda"
SEG_LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1026]


def _rot(x, cos, sin):       # x [..., T, hd]; cos / sin [T, hd/2] (half-split layout, hf modeling_esm.py:48-79)
    c, s = torch.cat([cos, cos], -1), torch.cat([sin, sin], -1)
    return x * c + O.rotate_half(x) * s


# ------------------------------------------------------------------------------------------------------------------ 1. varlen attention forward
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_varlen_attention_forward(hd):
    torch.manual_seed(hd)
    H = 2
    p, T, cu = pack_shape(SEG_LENGTHS)
    q = (torch.randn(H, T, hd) * 0.5).to(torch.bfloat16).to(DEV)
    k = torch.randn(H, T, hd).to(torch.bfloat16).to(DEV)
    v = torch.randn(H, T, hd).to(torch.bfloat16).to(DEV)
    ctx = torch.full((T, H * hd), 7.0, dtype=torch.bfloat16, device=DEV)       # garbage in the tail must be overwritten with zeros
    lse = torch.full((H, T), 7.0, device=DEV)
    w = p.attn_work()
    hip.call("oneprot_attn_varlen_fwd", q, k, v, p.cu_seqlens, w, w.shape[0], ctx, lse, len(p), T, H, hd)
    torch.cuda.synchronize()
    qf, kf, vf = q.float(), k.float(), v.float()
    for a, n in zip(cu[:-1], SEG_LENGTHS):
        s = (qf[:, a:a + n] @ kf[:, a:a + n].transpose(1, 2)) * math.log(2.0)          # q carries hd^-1/2 * log2(e): natural-log scores
        ref = torch.softmax(s, -1) @ vf[:, a:a + n]
        got = ctx[a:a + n].float().view(n, H, hd).transpose(0, 1)
        assert (got - ref).abs().max() < 3e-2, (n, float((got - ref).abs().max()))
        assert (lse[:, a:a + n] - torch.logsumexp(s, -1)).abs().max() < 1e-2, n
    assert (ctx[cu[-1]:] == 0).all() and (lse[:, cu[-1]:] == 0).all()


def test_varlen_attention_forward_large_scores():
    """scores of +-400 (natural units): the per-tile running maximum keeps the softmax exact"""
    torch.manual_seed(3)
    H, hd = 2, 32
    lengths = [5, 300, 1026, 77]
    p, T, cu = pack_shape(lengths)
    qd = torch.randn(H, T, hd)
    kd = torch.randn(H, T, hd)
    qd = qd / qd.norm(dim=-1, keepdim=True)
    kd = kd / kd.norm(dim=-1, keepdim=True)
    for a, n in zip(cu[:-1], lengths):              # every segment holds a score of +400 and one of -400
        kd[:, a] = qd[:, a]
        kd[:, a + n - 1] = -qd[:, a + n - 1]
    q = (qd * 400.0 / math.log(2.0)).to(torch.bfloat16).to(DEV)     # |q.k| ln 2 up to 400
    k = kd.to(torch.bfloat16).to(DEV)
    v = torch.randn(H, T, hd).to(torch.bfloat16).to(DEV)
    ctx = torch.empty(T, H * hd, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(H, T, device=DEV)
    w = p.attn_work()
    hip.call("oneprot_attn_varlen_fwd", q, k, v, p.cu_seqlens, w, w.shape[0], ctx, lse, len(p), T, H, hd)
    torch.cuda.synchronize()
    qf, kf, vf = q.float().double(), k.float().double(), v.float().double()
    for a, n in zip(cu[:-1], lengths):
        s = (qf[:, a:a + n] @ kf[:, a:a + n].transpose(1, 2)) * math.log(2.0)
        assert float(s.max()) > 390 and float(s.min()) < -390
        ref = torch.softmax(s, -1) @ vf[:, a:a + n]
        got = ctx[a:a + n].double().view(n, H, hd).transpose(0, 1)
        assert torch.isfinite(got).all()
        assert (got - ref).abs().max() < 5e-2, (n, float((got - ref).abs().max()))
        assert ((lse[:, a:a + n].double() - torch.logsumexp(s, -1)).abs() / torch.logsumexp(s, -1).abs().clamp(min=1)).max() < 1e-3


# ------------------------------------------------------------------------------------------------------------------ 2. varlen attention backward
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_varlen_attention_backward(hd):
    torch.manual_seed(10 + hd)
    H = 2
    lengths = [1, 17, 33, 130, 257, 600, 1026]
    p, T, cu = pack_shape(lengths)
    cos, sin = gathered_tables(lengths, T, hd)
    scale = hd ** -0.5
    q0, k0, v0 = (torch.randn(H, T, hd) for _ in range(3))
    q = (_rot(q0, cos, sin) * scale * hip.LOG2E).to(torch.bfloat16)
    k = _rot(k0, cos, sin).to(torch.bfloat16)
    v = v0.to(torch.bfloat16)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ctx = torch.empty(T, H * hd, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(H, T, device=DEV)
    w = p.attn_work()
    hip.call("oneprot_attn_varlen_fwd", qd, kd, vd, p.cu_seqlens, w, w.shape[0], ctx, lse, len(p), T, H, hd)
    dctx = torch.randn(T, H * hd).to(torch.bfloat16)
    dctx[cu[-1]:] = 0
    dctx = dctx.to(DEV)
    cos_d, sin_d = cos.to(DEV), sin.to(DEV)
    ws = torch.empty(hip.query("oneprot_attn_varlen_bwd_workspace", H, T), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        dqkv = torch.full((T, 3 * H * hd), 3.0, dtype=torch.bfloat16, device=DEV)
        hip.call("oneprot_attn_varlen_bwd", qd, kd, vd, p.cu_seqlens, w, w.shape[0], ctx, dctx, lse, cos_d, sin_d, scale, dqkv, ws, len(p), T, H, hd)
        outs.append(dqkv)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    dqkv = outs[0].float().cpu()
    assert (dqkv[cu[-1]:] == 0).all()
    # reference: autograd through rotary + scale + softmax, per segment, from the un-rotated projections
    q0r, k0r, v0r = q0.clone().requires_grad_(), k0.clone().requires_grad_(), v0.clone().requires_grad_()
    loss = 0.0
    for a, n in zip(cu[:-1], lengths):
        qs = _rot(q0r[:, a:a + n], cos[a:a + n], sin[a:a + n]) * scale
        ks = _rot(k0r[:, a:a + n], cos[a:a + n], sin[a:a + n])
        o = torch.softmax(qs @ ks.transpose(1, 2), -1) @ v0r[:, a:a + n]
        loss = loss + (o * dctx[a:a + n].float().cpu().view(n, H, hd).transpose(0, 1)).sum()
    loss.backward()
    dm = H * hd
    n_real = cu[-1]
    for i, ref in enumerate((q0r.grad, k0r.grad, v0r.grad)):
        got = dqkv[:n_real, i * dm:(i + 1) * dm].view(n_real, H, hd).transpose(0, 1)
        r = ref[:, :n_real]
        assert cos_sim(got, r) > 0.999, (i, cos_sim(got, r))
        assert (got - r).abs().max() < 0.05 * r.abs().max(), i


@pytest.mark.parametrize("lengths", [[1], [33], [130], [257], [130, 130]], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_split_kernels_padded_equals_packed(hd, lengths):
    """the padded and the packed split kernels are one body behind two decoders: the same sequences give the same bits through either.
    1: a single row; 33: a partial 32-key tile; 130: a second 128-row block; 257: a second 256-key chunk holding one key; [130, 130]: the second
    sequence (b = 1, start = 130) tells the head-major row, the token-major row and the rotary row of position 0 apart"""
    torch.manual_seed(100 * hd + sum(lengths))
    H, B, L = 2, len(lengths), lengths[0]
    assert all(n == L for n in lengths)
    n_real = B * L
    p, T, cu = pack_shape(lengths)
    cos_pk, sin_pk = gathered_tables(lengths, T, hd)
    cos_pad, sin_pad = rope_half(L, hd)
    for a in cu[:-1]:
        assert torch.equal(cos_pk[a:a + L], cos_pad) and torch.equal(sin_pk[a:a + L], sin_pad)
    scale = hd ** -0.5
    q = (_rot(torch.randn(H, T, hd), cos_pk, sin_pk) * scale * hip.LOG2E).to(torch.bfloat16).to(DEV)
    k = _rot(torch.randn(H, T, hd), cos_pk, sin_pk).to(torch.bfloat16).to(DEV)
    v = torch.randn(H, T, hd).to(torch.bfloat16).to(DEV)
    dctx = torch.randn(T, H * hd).to(torch.bfloat16).to(DEV)
    to_padded = lambda x: x[:, :n_real].reshape(H, B, L, -1).transpose(0, 1).contiguous()      # [H, T, *] -> [B, H, L, *]
    q_pad, k_pad, v_pad = to_padded(q), to_padded(k), to_padded(v)
    dctx_pad = dctx[:n_real].contiguous()
    # packed
    ctx_pk = torch.empty(T, H * hd, dtype=torch.bfloat16, device=DEV)
    lse_pk = torch.empty(H, T, device=DEV)
    dqkv_pk = torch.empty(T, 3 * H * hd, dtype=torch.bfloat16, device=DEV)
    w = p.attn_work()
    hip.call("oneprot_attn_varlen_fwd", q, k, v, p.cu_seqlens, w, w.shape[0], ctx_pk, lse_pk, len(p), T, H, hd)
    ws = torch.empty(hip.query("oneprot_attn_varlen_bwd_workspace", H, T), dtype=torch.uint8, device=DEV)
    hip.call("oneprot_attn_varlen_bwd", q, k, v, p.cu_seqlens, w, w.shape[0], ctx_pk, dctx, lse_pk, cos_pk.to(DEV), sin_pk.to(DEV), scale, dqkv_pk, ws,
             len(p), T, H, hd)
    # padded, through the split kernels
    ctx_pad = torch.empty(n_real, H * hd, dtype=torch.bfloat16, device=DEV)
    lse_pad = torch.empty(B, H, L, device=DEV)
    dqkv_pad = torch.empty(n_real, 3 * H * hd, dtype=torch.bfloat16, device=DEV)
    ws_pad = torch.empty(hip.query("oneprot_attn_bwd_workspace", B, H, L), dtype=torch.uint8, device=DEV)
    try:
        hip.query("oneprot_attn_force_fwd_path", 0)
        hip.query("oneprot_attn_force_bwd_path", 0)
        hip.call("oneprot_attn_fwd", q_pad, k_pad, v_pad, None, ctx_pad, lse_pad, B, H, L, hd)
        hip.call("oneprot_attn_bwd", q_pad, k_pad, v_pad, None, ctx_pad, dctx_pad, lse_pad, cos_pad.to(DEV), sin_pad.to(DEV), scale, dqkv_pad, ws_pad,
                 B, H, L, hd)
    finally:
        hip.query("oneprot_attn_force_fwd_path", -1)
        hip.query("oneprot_attn_force_bwd_path", -1)
    torch.cuda.synchronize()
    assert torch.isfinite(ctx_pad.float()).all() and torch.isfinite(dqkv_pad.float()).all() and dqkv_pad.float().abs().max() > 0
    assert torch.equal(ctx_pk[:n_real], ctx_pad)
    assert torch.equal(to_padded(lse_pk[:, :, None])[..., 0], lse_pad)
    assert torch.equal(dqkv_pk[:n_real], dqkv_pad)


@pytest.mark.parametrize("d", [64, 128])
def test_row_kernels_padded_equals_packed(d):
    """the row kernels that fork on the layout (embedding, pooling with and without the final LayerNorm) find their rows through the `row_seg` decoder of
    rowops.hip, one body for both forms (the pooling backward: two kernels with the same arithmetic): the same sequences give the same bits through
    the padded and the packed entry points (C ABI only).  The value-changing operations are
    the same in the same order; a padded sequence's pad rows add exact zeros.  Lengths: one row, a partial chunk, 33 = one token into the embedding's
    second chunk of 32, 130, and 257 = the padded L (no pad row; a 512-thread count loop's second trip has none, a 256-thread one's has one token).
    d = 64 / 128: 16 / 32 float4 columns for 64 lanes.  <mask> ids in two segments (their own token-dropout factors), one pad id inside a segment."""
    torch.manual_seed(7 + d)
    lengths = [1, 7, 33, 130, 257]
    N, L, T, V, hd, PAD, MASK, eps = len(lengths), 257, 512, 33, 32, 1, 32, 1e-5
    cu = cu_of(lengths)
    n_real = cu[-1]
    gen = torch.Generator().manual_seed(11)
    ids_pad = torch.full((N, L), PAD, dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids_pad[b, :n] = torch.randint(4, 24, (n,), generator=gen)
    ids_pad[2, [3, 20]] = MASK
    ids_pad[4, torch.randperm(257, generator=gen)[:40]] = MASK
    ids_pad[3, 50] = PAD                                             # a pad id inside a segment: no pooling weight, not counted
    ids_pk = torch.full((T,), PAD, dtype=torch.int64)
    for b, (a, n) in enumerate(zip(cu[:-1], lengths)):
        ids_pk[a:a + n] = ids_pad[b, :n]
    ids_pad, ids_pk = ids_pad.to(DEV), ids_pk.to(DEV)
    cu_d = torch.tensor(cu, dtype=torch.int32, device=DEV)
    segs = list(zip(range(N), cu[:-1], lengths))

    def same(pk, pad, what):                                         # pk [T, ...] per stream row, pad [N, L, ...]
        for b, a, n in segs:
            assert torch.equal(pk[a:a + n], pad[b, :n]), (what, b)

    # ---- embedding: x, the token-dropout factor per token = per row, the gathered rotary rows
    W = torch.randn(V, d).to(DEV)
    cos_t, sin_t = (t.to(DEV) for t in rope_half(1026, hd))
    x_pad, row_scale = torch.full((N, L, d), 5.0, device=DEV), torch.empty(N, device=DEV)
    hip.call("oneprot_esm_embed_fwd", ids_pad, W, x_pad, row_scale, N, L, d, V, PAD, MASK, 1)
    x_pk, tok_scale = torch.full((T, d), 5.0, device=DEV), torch.full((T,), 5.0, device=DEV)
    cos_o, sin_o = torch.empty(T, hd // 2, device=DEV), torch.empty(T, hd // 2, device=DEV)
    hip.call("oneprot_esm_embed_packed_fwd", ids_pk, cu_d, W, cos_t, sin_t, x_pk, tok_scale, cos_o, sin_o, N, T, L, d, V, hd // 2, 1026, PAD, MASK, 1)
    torch.cuda.synchronize()
    same(x_pk, x_pad, "embed x")
    assert x_pk[:n_real].abs().max() > 0 and len(set(row_scale.tolist())) == 3       # no <mask>, 2 of 33, 40 of 257
    for b, a, n in segs:
        assert (tok_scale[a:a + n] == row_scale[b]).all(), b
        assert torch.equal(cos_o[a:a + n], cos_t[:n]) and torch.equal(sin_o[a:a + n], sin_t[:n]), b
        assert (x_pad[b, n:] == 0).all()
    assert (x_pk[n_real:] == 0).all() and (tok_scale[n_real:] == 0).all()

    # ---- pooling inputs: finite everywhere, as the towers' pad rows are
    h_pk = torch.randn(T, d, device=DEV)
    h_pad = torch.randn(N, L, d, device=DEV)
    for b, a, n in segs:
        h_pad[b, :n] = h_pk[a:a + n]
    dpooled = torch.randn(N, d, device=DEV)
    gamma, beta = (1 + 0.1 * torch.randn(d)).to(DEV), (0.1 * torch.randn(d)).to(DEV)
    for mode in (0, 1):
        # pooling without a LayerNorm, forward and backward (fp32 and the bf16 copy)
        p_pad, p_pk = torch.empty(N, d, device=DEV), torch.empty(N, d, device=DEV)
        hip.call("oneprot_pool_fwd", h_pad, ids_pad, PAD, p_pad, N, L, d, mode)
        hip.call("oneprot_pool_packed_fwd", h_pk, ids_pk, cu_d, PAD, p_pk, N, T, d, mode)
        g_pad, g_pk = torch.full((N, L, d), 9.0, device=DEV), torch.full((T, d), 9.0, device=DEV)
        g16_pad, g16_pk = torch.empty(N, L, d, dtype=torch.bfloat16, device=DEV), torch.empty(T, d, dtype=torch.bfloat16, device=DEV)
        hip.call("oneprot_pool_bwd", dpooled, ids_pad, PAD, g_pad, g16_pad, N, L, d, mode)
        hip.call("oneprot_pool_packed_bwd", dpooled, ids_pk, cu_d, PAD, g_pk, g16_pk, N, T, d, mode)
        # final LayerNorm + pooling
        q_pad, q_pk = torch.empty(N, d, device=DEV), torch.empty(N, d, device=DEV)
        st_pad = [torch.empty(N, L, device=DEV) for _ in range(3)]
        st_pk = [torch.full((T,), 9.0, device=DEV) for _ in range(3)]
        hid_pad, hid_pk = torch.empty(N, L, d, device=DEV), torch.empty(T, d, device=DEV)
        hip.call("oneprot_lnpool_fwd", h_pad, ids_pad, PAD, gamma, beta, q_pad, *st_pad, None, hid_pad, N, L, d, eps, mode)
        hip.call("oneprot_lnpool_packed_fwd", h_pk, ids_pk, cu_d, PAD, gamma, beta, q_pk, *st_pk, hid_pk, N, T, d, eps, mode)
        torch.cuda.synchronize()
        assert torch.isfinite(p_pad).all() and torch.equal(p_pk, p_pad), ("pool_fwd", mode)
        same(g_pk, g_pad, ("pool_bwd", mode))
        same(g16_pk, g16_pad, ("pool_bwd bf16", mode))
        assert g_pad[3, 50].abs().max() == 0 and (g_pad[3, 49].abs().max() > 0) == (mode == 0)
        assert (g_pk[n_real:] == 0).all() and (g16_pk[n_real:] == 0).all()
        assert all((g_pad[b, n:] == 0).all() for b, a, n in segs)
        assert torch.isfinite(q_pad).all() and torch.equal(q_pk, q_pad), ("lnpool pooled", mode)
        for nm, s_pk, s_pad in zip(("mean", "rstd", "wrow"), st_pk, st_pad):
            same(s_pk, s_pad, ("lnpool " + nm, mode))
        same(hid_pk, hid_pad, ("lnpool hidden", mode))
        assert (st_pk[2][n_real:] == 0).all() and st_pk[2][cu[3] + 50] == 0      # wrow: the tail and the pad id weigh nothing


# ------------------------------------------------------------------------------------------------------------------ 3. packed embedding
def test_packed_embedding_forward_backward():
    torch.manual_seed(4)
    lengths = [40, 7, 300, 1026, 1]
    gen = torch.Generator().manual_seed(9)
    seqs = []
    for j, n in enumerate(lengths):
        s = torch.randint(4, 24, (n,), generator=gen)
        if j in (0, 2, 3):                                       # <mask> tokens in some segments: their own token-dropout factor
            s[torch.randperm(n, generator=gen)[: max(1, n // (5 + j))]] = 32
        seqs.append(s)
    p = PackedTokens.from_list(seqs).to(DEV)
    T, d, V, hd = p.T_pad, 64, 33, 32
    W = torch.randn(V, d)
    cos_t, sin_t = rope_half(1026, hd)
    x = torch.full((T, d), 5.0, device=DEV)
    tok_scale = torch.empty(T, device=DEV)
    cos_o, sin_o = torch.empty(T, hd // 2, device=DEV), torch.empty(T, hd // 2, device=DEV)
    hip.call("oneprot_esm_embed_packed_fwd", p.ids, p.cu_seqlens, W.to(DEV), cos_t.to(DEV), sin_t.to(DEV), x, tok_scale, cos_o, sin_o, len(p), T, p.max_len,
             d, V, hd // 2, 1026, 1, 32, 1)
    dx = torch.randn(T, d)
    dtable = torch.empty(V, d, device=DEV)
    ws = torch.empty(hip.query("oneprot_esm_embed_bwd_workspace", T, d, V), dtype=torch.uint8, device=DEV)
    hip.call("oneprot_esm_embed_packed_bwd", p.ids, dx.to(DEV), tok_scale, dtable, ws, T, d, V, 1, 32, 1, 0)
    torch.cuda.synchronize()
    x, cos_o, sin_o = x.cpu(), cos_o.cpu(), sin_o.cpu()
    Wr = W.clone().requires_grad_()
    loss = 0.0
    cu = cu_of(lengths)
    for a, n, s in zip(cu[:-1], lengths, seqs):
        ref = O.esm_embeddings(s[None], torch.ones(1, n, dtype=torch.int64), Wr, 32, True)[0]
        assert (x[a:a + n] - ref.detach()).abs().max() < 1e-5, n
        assert torch.equal(cos_o[a:a + n], cos_t[:n]) and torch.equal(sin_o[a:a + n], sin_t[:n])
        loss = loss + (ref * dx[a:a + n]).sum()
    loss.backward()
    assert (x[cu[-1]:] == 0).all() and (tok_scale[cu[-1]:] == 0).all()
    assert (dtable.cpu() - Wr.grad).abs().max() < 1e-3 * Wr.grad.abs().max()


# ------------------------------------------------------------------------------------------------------------------ 4. segment LayerNorm + pooling
@pytest.mark.parametrize("mode", ["mean", "cls", "attention1d"])
def test_segment_layernorm_pooling(mode):
    torch.manual_seed(5)
    lengths = [3, 1, 64, 257, 1026, 40]
    p, T, cu = pack_shape(lengths)
    d, eps = 128, 1e-5
    x = torch.randn(T, d)
    gamma, beta = 1 + 0.1 * torch.randn(d), 0.1 * torch.randn(d)
    pw, pb = 0.1 * torch.randn(d), 0.1 * torch.randn(1)
    N = len(p)
    xd = x.to(DEV)
    pooled = torch.empty(N, d, device=DEV)
    mean, rstd, wrow = (torch.empty(T, device=DEV) for _ in range(3))
    dpooled = torch.randn(N, d)
    dx = torch.full((T, d), 9.0, device=DEV)
    dx16 = torch.empty(T, d, dtype=torch.bfloat16, device=DEV)
    dg, db = torch.empty(d, device=DEV), torch.empty(d, device=DEV)
    ws = torch.empty(hip.query("oneprot_layernorm_bwd_workspace", d), dtype=torch.uint8, device=DEV)
    if mode == "attention1d":
        hidden = torch.empty(T, d, device=DEV)
        hip.call("oneprot_lnpool_packed_fwd", xd, p.ids, p.cu_seqlens, 1, gamma.to(DEV), beta.to(DEV), pooled, mean, rstd, wrow, hidden, N, T, d, eps, 0)
        attn = torch.empty(T, device=DEV)
        hip.call("oneprot_attnpool_packed_fwd", hidden, p.ids, p.cu_seqlens, 1, pw.to(DEV), pb.to(DEV), pooled, attn, N, p.max_len, d)
        dhidden = torch.full((T, d), 9.0, device=DEV)
        dw, dbias = torch.empty(d, device=DEV), torch.empty(1, device=DEV)
        hip.call("oneprot_attnpool_packed_bwd", hidden, attn, p.cu_seqlens, pw.to(DEV), dpooled.to(DEV), dw, dbias, dhidden,
                 torch.empty(hip.query("oneprot_attnpool_bwd_workspace", N, d), dtype=torch.uint8, device=DEV), N, T, p.max_len, d)
        hip.call("oneprot_layernorm_bwd", dhidden, 1, None, 0, xd, 0, gamma.to(DEV), mean, rstd, None, dx, dx16, dg, db, ws, T, d, 0)
        assert (dhidden[cu[-1]:] == 0).all()
    else:
        m = 0 if mode == "mean" else 1
        hip.call("oneprot_lnpool_packed_fwd", xd, p.ids, p.cu_seqlens, 1, gamma.to(DEV), beta.to(DEV), pooled, mean, rstd, wrow, None, N, T, d, eps, m)
        hip.call("oneprot_lnpool_packed_bwd", dpooled.to(DEV), p.cu_seqlens, wrow, xd, gamma.to(DEV), mean, rstd, dx, dx16, dg, db, ws, N, T, d)
    torch.cuda.synchronize()
    xr, gr, br, pwr, pbr = (t.clone().requires_grad_() for t in (x, gamma, beta, pw, pb))
    refs = []
    for a, n in zip(cu[:-1], lengths):
        hseg = O.layer_norm(xr[a:a + n], gr, br, eps)
        if mode == "mean":
            refs.append(hseg.mean(0))
        elif mode == "cls":
            refs.append(hseg[0])
        else:
            refs.append(O.attention1d_pool(hseg[None], pwr.view(1, d, 1), pbr, torch.ones(1, n))[0])
    ref = torch.stack(refs)
    assert (pooled.cpu() - ref.detach()).abs().max() < 1e-4 * max(1.0, float(ref.abs().max()))
    (ref * dpooled).sum().backward()
    assert (dx[cu[-1]:] == 0).all() and (dx16[cu[-1]:] == 0).all()
    assert (dx.cpu()[:cu[-1]] - xr.grad[:cu[-1]]).abs().max() < 1e-4 * max(1.0, float(xr.grad.abs().max()))
    assert (dg.cpu() - gr.grad).abs().max() < 1e-3 * max(1.0, float(gr.grad.abs().max()))
    assert (db.cpu() - br.grad).abs().max() < 1e-3 * max(1.0, float(br.grad.abs().max()))
    if mode == "attention1d":
        assert (dw.cpu() - pwr.grad).abs().max() < 1e-3 * max(1.0, float(pwr.grad.abs().max()))
        assert abs(float(dbias.cpu()) - float(pbr.grad)) < 1e-3 * max(1.0, abs(float(pbr.grad)))


# ------------------------------------------------------------------------------------------------------------------ 5. reference goldens
@pytest.fixture
def random_init(monkeypatch):
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")


@pytest.mark.parametrize("tag", ["hd16", "hd24", "hd32"])
def test_packed_forward_features_vs_reference(golden_dir, tag, tmp_path, random_init):
    g, module = golden_pair_module(golden_dir, tag, tmp_path)
    pad = g["cfg"]["pad"]
    with torch.no_grad():
        sf = module(PackedTokens.from_padded(g["seq_ids"], pad_id=pad).to(DEV), "sequence").cpu()
        mf = module(PackedTokens.from_padded(g["st_ids"], pad_id=pad).to(DEV), "struct_token").cpu()
    for got, ref, name in ((sf, g["sequence_features"], "sequence"), (mf, g["modality_features"], "struct_token")):
        assert got.shape == ref.shape
        cs = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
        assert cs.min() > 0.999, f"{name}: min cosine {cs.min()}"
        assert (got - ref).abs().max() < 0.05 * ref.abs().max(), name
    assert abs(mf.norm(dim=-1) - 1 / 0.07).max() < 1e-3


@pytest.mark.parametrize("tag,frozen_seq", [("hd16", False), ("hd24", False), ("hd32", False), ("hd32", True)])
def test_packed_training_substep_vs_reference(golden_dir, tag, frozen_seq, tmp_path, random_init):
    g, module = golden_pair_module(golden_dir, tag, tmp_path, frozen_seq=frozen_seq)
    pad = g["cfg"]["pad"]
    batch = {"struct_token": (PackedTokens.from_padded(g["seq_ids"], pad_id=pad).to(DEV), PackedTokens.from_padded(g["st_ids"], pad_id=pad).to(DEV),
                              "struct_token", None)}
    grads = {}
    orig_clip = module.clip_gradients

    def spy(opt, **kw):
        for name, enc in module.network.items():
            pref = "seq." if name == "sequence" else "st."
            tr = enc.transformer
            if tr.flat.grad is not None:
                for k in tr._spec:
                    grads[pref + "transformer." + k] = tr.view(k, tr.flat.grad).detach().cpu().clone()
            for k, p_ in enc.proj.named_parameters():
                if p_.grad is not None:
                    grads[pref + "proj." + k] = p_.grad.detach().cpu().clone()
        return orig_clip(opt, **kw)

    module.clip_gradients = spy
    loss = float(module.training_step(batch, 0))
    ref_loss = float(g["loss_total"])
    assert abs(loss - ref_loss) / abs(ref_loss) < 1e-3, (loss, ref_loss)
    keys = [k for k, ref in g["grads"].items() if k in grads and ref.abs().max() >= 1e-7]
    assert len(keys) > (15 if frozen_seq else 30)
    if frozen_seq:
        assert not any(k.startswith("seq.transformer.") for k in grads)
    big = max(float(g["grads"][k].norm()) for k in keys)
    for k in keys:
        c = cos_sim(grads[k], g["grads"][k])
        assert c > 0.98, (k, c)
        if float(g["grads"][k].norm()) >= 0.01 * big:
            assert c > 0.999, (k, c)
    allg = torch.cat([grads[k].flatten() for k in keys]); allr = torch.cat([g["grads"][k].flatten() for k in keys])
    assert cos_sim(allg, allr) > 0.9999
    if frozen_seq:
        return            # the reference's post-Adam weights are those of the trainable form
    gn = float(module.last_grad_norm)
    assert abs(gn - float(g["grad_total_norm"])) / float(g["grad_total_norm"]) < 2e-2, (gn, float(g["grad_total_norm"]))
    coef = min(1.0, 1.0 / (float(g["grad_total_norm"]) + 1e-6))
    for enc_name, after, gpref in (("sequence", g["sd_seq_after"], "seq."), ("struct_token", g["sd_st_after"], "st.")):
        sd = {k: v.cpu() for k, v in module.network[enc_name].state_dict().items()}
        for k, v in after.items():
            if "inv_freq" in k or gpref + k not in g["grads"]:
                continue
            ga = (g["grads"][gpref + k] * coef).abs()
            well = ga > max(1e-4, 0.02 * float(ga.max()))
            if well.any():
                assert (sd[k] - v)[well].abs().max() < 2e-4, k
            assert (sd[k] - v).abs().max() < 2.1e-3, k


# ------------------------------------------------------------------------------------------------------------------ 6. padded against packed
def _pair_module(path, lora=False, seed=0):
    os.environ.update(RANK="0", WORLD_SIZE="1")
    from oneprot_amd.encoders import SequenceEncoder, StructTokenEncoder
    from oneprot_amd.module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(seed)
    seq = SequenceEncoder(path, output_dim=256, pooling_type="mean", proj_type="mlp", use_lora=lora, lora_dropout=0.0, frozen=lora)
    st = StructTokenEncoder(path, output_dim=256, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    return OneProtLitModule(components={"sequence": seq, "struct_token": st}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                            use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(DEV)


def _substep_with_grads(module, batch):
    grads = {}
    orig = module.clip_gradients

    def spy(opt, **kw):
        for name, enc in module.network.items():
            tr = enc.transformer
            if tr.flat.grad is not None:
                grads[name] = tr.flat.grad.detach().clone()
            if getattr(tr, "_lora", None):
                grads[name + ".lora"] = torch.cat([tr.lora_A.grad.flatten(), tr.lora_B.grad.flatten()])
        return orig(opt, **kw)

    module.clip_gradients = spy
    return float(module.training_step(batch, 0)), grads


@pytest.mark.parametrize("lora", [False, True])
def test_padded_vs_packed_substep_150m_shape(tmp_path, random_init, lora):
    """ESM-2-150M layer shape (640 wide, 20 heads of 32, 30 layers) on ragged synthetic data, random init: the same sub-step in both layouts"""
    from oneprot_amd.data import SyntheticPairs
    path = esm_dir(tmp_path, "esm150", 30, 640, 20, 2560)
    rag = next(iter(SyntheticPairs("struct_token", 24, 512, seed=21, ragged=True)))
    pk = next(iter(SyntheticPairs("struct_token", 24, 512, seed=21, packed=True)))
    m_pad = _pair_module(path, lora=lora)
    m_pk = _pair_module(path, lora=lora)
    m_pk.load_state_dict(m_pad.state_dict())
    l_pad, g_pad = _substep_with_grads(m_pad, {"struct_token": (rag[0].to(DEV), rag[1].to(DEV), "struct_token", None)})
    l_pk, g_pk = _substep_with_grads(m_pk, {"struct_token": (pk[0].to(DEV), pk[1].to(DEV), "struct_token", None)})
    assert abs(l_pad - l_pk) / abs(l_pad) < 1e-3, (l_pad, l_pk)
    assert set(g_pad) == set(g_pk) and len(g_pad) >= 2
    for k in g_pad:
        assert cos_sim(g_pad[k], g_pk[k]) >= 0.999, (k, cos_sim(g_pad[k], g_pk[k]))


def test_padded_vs_packed_forward_650m_attention1d(tmp_path, random_init):
    """ESM-2-650M layer shape (1280 wide, 20 heads of 64; 6 of its 33 layers) with attention1d pooling, forward only"""
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.encoders import SequenceEncoder
    path = esm_dir(tmp_path, "esm650", 6, 1280, 20, 5120)
    torch.manual_seed(2)
    enc = SequenceEncoder(path, output_dim=512, pooling_type="attention1d", proj_type="linear", use_lora=False, frozen=True).to(DEV).eval()
    rag = next(iter(SyntheticPairs("sequence", 16, 512, seed=8, ragged=True)))[0]
    pk = next(iter(SyntheticPairs("sequence", 16, 512, seed=8, packed=True)))[0]
    with torch.no_grad():
        a = enc(rag.to(DEV)).cpu()
        b = enc(pk.to(DEV)).cpu()
    cs = torch.nn.functional.cosine_similarity(a, b, dim=-1)
    assert cs.min() >= 0.999, cs.min()
    assert (a - b).abs().max() < 0.05 * a.abs().max()
    hidden = enc.transformer(pk.to(DEV)).last_hidden_state
    assert hidden.shape == (pk.T_pad, 1280) and torch.isfinite(hidden).all()


# ------------------------------------------------------------------------------------------------------------------ 7. pack composition
def test_features_independent_of_pack_composition(tmp_path, random_init):
    from oneprot_amd.encoders import SequenceEncoder
    path = esm_dir(tmp_path, "esm", 4, 320, 20, 1280)
    torch.manual_seed(6)
    enc = SequenceEncoder(path, output_dim=128, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=True).to(DEV)
    gen = torch.Generator().manual_seed(1)
    mk = lambda n: torch.cat([torch.tensor([0]), torch.randint(4, 24, (n - 2,), generator=gen), torch.tensor([2])])
    target = mk(200)
    a = PackedTokens.from_list([target, mk(100), mk(300)], t_pad=1024).to(DEV)
    b = PackedTokens.from_list([mk(37), mk(511), target, mk(5)], t_pad=1024).to(DEV)
    with torch.no_grad():
        fa, fb = enc(a), enc(b)
    assert torch.equal(fa[0], fb[2])


# ------------------------------------------------------------------------------------------------------------------ 8. mixed pair
def test_mixed_pair_packed_esm_padded_bert(tmp_path, random_init):
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.encoders import SequenceEncoder, TextEncoder
    from oneprot_amd.module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    os.environ.update(RANK="0", WORLD_SIZE="1")
    esm = esm_dir(tmp_path, "esm", 4, 320, 20, 1280)
    bert = os.path.join(str(tmp_path), "bert")
    os.makedirs(bert)
    with open(os.path.join(bert, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=1000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                       max_position_embeddings=512, pad_token_id=0, layer_norm_eps=1e-12), f)

    def build():
        torch.manual_seed(3)
        seq = SequenceEncoder(esm, output_dim=128, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
        txt = TextEncoder(bert, output_dim=128, pooling_type="mean", proj_type="linear", use_logit_scale=True, frozen=True)
        txt.transformer.train_dropout = False
        return OneProtLitModule(components={"sequence": seq, "text": txt}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                                use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(DEV)

    rag = next(iter(SyntheticPairs("text", 12, 200, seed=4, ragged=True, text_vocab=1000)))
    pk = next(iter(SyntheticPairs("text", 12, 200, seed=4, packed=True, text_vocab=1000)))
    assert isinstance(pk[0], PackedTokens) and torch.equal(pk[1], rag[1])
    l_pad = float(build().training_step({"text": (rag[0].to(DEV), rag[1].to(DEV), "text", None)}, 0))
    l_mix = float(build().training_step({"text": (pk[0].to(DEV), pk[1].to(DEV), "text", None)}, 0))
    assert abs(l_pad - l_mix) / abs(l_pad) < 1e-3, (l_pad, l_mix)
    with pytest.raises(ValueError, match="same number"):
        build().training_step({"text": (pk[0].to(DEV), rag[1][:5].to(DEV), "text", None)}, 0)
