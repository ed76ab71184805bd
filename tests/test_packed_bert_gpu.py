"""Packed caption streams through the BERT text tower on the MI355X: the varlen attention kernels with probability dropout against the padded
kernels (bits) and against float64 with the exported mask, the packed embedding / position gradient / pooling kernels against torch, and the tower
packed against padded on identical captions (eval mode, train mode, the reference's goldens, LoRA, the module's sub-step)."""
import functools
import json
import math
import os

import pytest
import torch

from oneprot_amd import hip
from oneprot_amd.packing import PackedTokens

from tests.cases import cu as cu_of, gathered_tables, pack_shape, rope_half
from tests.gate import cos_sim

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _rc(name, *args):
    """status of an entry point, without hip.call's exception"""
    cargs = [hip.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
    return getattr(hip.lib(), name)(*cargs, hip.stream())


# ------------------------------------------------------------------------------------------------------------------ 1. bits: padded = packed
@pytest.mark.parametrize("lengths", [[1], [33], [130], [257], [130, 130], [33, 33, 33]], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_dropout_kernels_padded_equals_packed(hd, lengths):
    """the DROP = true varlen kernels against oneprot_attn_fwd_dropout / _bwd_dropout on the padded batch of the same sequences, same (p, seed,
    stream): the same bits.  The multi-segment cases catch a dropout stream that is not segment * H + head."""
    torch.manual_seed(100 * hd + sum(lengths))
    H, B, L = 2, len(lengths), lengths[0]
    n_real = B * L
    p, T, cu = pack_shape(lengths, pad_id=0)
    w = p.attn_work()
    scale = hd ** -0.5
    to_padded = lambda x: x[:, :n_real].reshape(H, B, L, -1).transpose(0, 1).contiguous()      # [H, T, *] -> [B, H, L, *]
    q = (torch.randn(H, T, hd) * scale * hip.LOG2E).to(torch.bfloat16).to(DEV)
    k = torch.randn(H, T, hd).to(torch.bfloat16).to(DEV)
    v = torch.randn(H, T, hd).to(torch.bfloat16).to(DEV)
    dctx = torch.randn(T, H * hd).to(torch.bfloat16).to(DEV)
    q_pad, k_pad, v_pad, dctx_pad = to_padded(q), to_padded(k), to_padded(v), dctx[:n_real].contiguous()
    cos_pk, sin_pk = (t.to(DEV) for t in gathered_tables(lengths, T, hd))
    cos_pad, sin_pad = (t.to(DEV) for t in rope_half(L, hd))
    ws = torch.empty(hip.query("oneprot_attn_varlen_bwd_workspace", H, T), dtype=torch.uint8, device=DEV)
    ws_pad = torch.empty(hip.query("oneprot_attn_bwd_workspace", B, H, L), dtype=torch.uint8, device=DEV)
    for prob in (0.1, 0.5):
        for rope in (False, True):          # null tables (BERT) and gathered per-token tables
            seed, stream = 4242 + hd, 9 + int(rope)
            ctx_pk = torch.empty(T, H * hd, dtype=torch.bfloat16, device=DEV)
            lse_pk = torch.empty(H, T, device=DEV)
            dqkv_pk = torch.empty(T, 3 * H * hd, dtype=torch.bfloat16, device=DEV)
            hip.call("oneprot_attn_varlen_fwd_dropout", q, k, v, p.cu_seqlens, w, w.shape[0], ctx_pk, lse_pk, len(p), T, H, hd, prob, seed, stream)
            hip.call("oneprot_attn_varlen_bwd_dropout", q, k, v, p.cu_seqlens, w, w.shape[0], ctx_pk, dctx, lse_pk, cos_pk if rope else None,
                     sin_pk if rope else None, scale, dqkv_pk, ws, len(p), T, H, hd, prob, seed, stream)
            ctx_pad = torch.empty(n_real, H * hd, dtype=torch.bfloat16, device=DEV)
            lse_pad = torch.empty(B, H, L, device=DEV)
            dqkv_pad = torch.empty(n_real, 3 * H * hd, dtype=torch.bfloat16, device=DEV)
            hip.call("oneprot_attn_fwd_dropout", q_pad, k_pad, v_pad, None, ctx_pad, lse_pad, B, H, L, hd, prob, seed, stream)
            hip.call("oneprot_attn_bwd_dropout", q_pad, k_pad, v_pad, None, ctx_pad, dctx_pad, lse_pad, cos_pad if rope else None, sin_pad if rope else None,
                     scale, dqkv_pad, ws_pad, B, H, L, hd, prob, seed, stream)
            torch.cuda.synchronize()
            tag = (prob, rope)
            assert torch.isfinite(ctx_pad.float()).all() and torch.isfinite(dqkv_pad.float()).all(), tag
            assert torch.equal(ctx_pk[:n_real], ctx_pad), tag
            assert torch.equal(to_padded(lse_pk[:, :, None])[..., 0], lse_pad), tag
            assert torch.equal(dqkv_pk[:n_real], dqkv_pad), tag


# ------------------------------------------------------------------------------------------------------------------ 2. ragged against float64
@pytest.mark.parametrize("hd", [64, 16])
def test_varlen_dropout_vs_float64_with_exported_mask(hd):
    """every segment of a ragged stream against float64 with the mask oneprot_attn_dropout_keep(N, H, max_len) exports, sliced [s, h, :n, :n]"""
    torch.manual_seed(20 + hd)
    lengths, H, prob, seed, stream = [1, 33, 130, 257, 64], 2, 0.5, 1234, 3
    N, Lmax = len(lengths), max(lengths)
    p, T, cu = pack_shape(lengths, pad_id=0)
    w = p.attn_work()
    scale = hd ** -0.5
    q = (torch.randn(H, T, hd) * scale * hip.LOG2E).to(torch.bfloat16)
    k = torch.randn(H, T, hd).to(torch.bfloat16)
    v = torch.randn(H, T, hd).to(torch.bfloat16)
    dctx = torch.randn(T, H * hd).to(torch.bfloat16)
    qd, kd, vd, dctx_d = q.to(DEV), k.to(DEV), v.to(DEV), dctx.to(DEV)
    keep = torch.empty(N, H, Lmax, Lmax, dtype=torch.uint8, device=DEV)
    hip.call("oneprot_attn_dropout_keep", keep, N, H, Lmax, prob, seed, stream)
    ws = torch.empty(hip.query("oneprot_attn_varlen_bwd_workspace", H, T), dtype=torch.uint8, device=DEV)

    def run(stream_id):
        ctx = torch.full((T, H * hd), 7.0, dtype=torch.bfloat16, device=DEV)            # garbage in the tail must be overwritten with zeros
        lse = torch.full((H, T), 7.0, device=DEV)
        dqkv = torch.full((T, 3 * H * hd), 3.0, dtype=torch.bfloat16, device=DEV)
        hip.call("oneprot_attn_varlen_fwd_dropout", qd, kd, vd, p.cu_seqlens, w, w.shape[0], ctx, lse, N, T, H, hd, prob, seed, stream_id)
        hip.call("oneprot_attn_varlen_bwd_dropout", qd, kd, vd, p.cu_seqlens, w, w.shape[0], ctx, dctx_d, lse, None, None, scale, dqkv, ws, N, T, H, hd,
                 prob, seed, stream_id)
        return ctx, lse, dqkv

    ctx, lse, dqkv = run(stream)
    ctx2, lse2, dqkv2 = run(stream)
    ctx3, _, _ = run(stream + 1)
    torch.cuda.synchronize()
    assert torch.equal(ctx, ctx2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)
    assert not torch.equal(ctx, ctx3)
    n_real = cu[-1]
    assert (ctx[n_real:] == 0).all() and (lse[:, n_real:] == 0).all() and (dqkv[n_real:] == 0).all()
    ctx, lse, dqkv, keep = ctx.cpu().double(), lse.cpu().double(), dqkv.cpu().double(), keep.cpu()
    assert torch.isfinite(dqkv).all() and torch.isfinite(ctx).all()
    keep_scale = 65536.0 / (65536 - int(prob * 65536 + 0.5))
    dm = H * hd
    dropped_rows = 0
    refs = [[], [], []]
    for s, (a, n) in enumerate(zip(cu[:-1], lengths)):
        # q carries hd^-1/2 * log2(e): the un-scaled query the gradient is taken with respect to is q / (scale * log2 e)
        q0 = (q[:, a:a + n].double() / (scale * hip.LOG2E)).requires_grad_()
        k0 = k[:, a:a + n].double().requires_grad_()
        v0 = v[:, a:a + n].double().requires_grad_()
        sc = (q0 * scale) @ k0.transpose(1, 2)
        m = keep[s, :, :n, :n].double()
        o = (torch.softmax(sc, -1) * m * keep_scale) @ v0
        do = dctx[a:a + n].double().view(n, H, hd).transpose(0, 1)
        (o * do).sum().backward()
        got = ctx[a:a + n].view(n, H, hd).transpose(0, 1)
        assert (got - o.detach()).abs().max() < 3e-2, (n, float((got - o.detach()).abs().max()))
        assert (lse[:, a:a + n] - torch.logsumexp(sc.detach(), -1)).abs().max() < 1e-2, n
        none_kept = m.sum(-1) == 0                                                   # [H, n]: rows whose every key is dropped
        dropped_rows += int(none_kept.sum())
        assert (got[none_kept] == 0).all()
        for i, ref in enumerate((q0.grad, k0.grad, v0.grad)):
            refs[i].append(ref)
    for i in range(3):                                                               # dq, dk, dv over the whole stream, as test_varlen_attention_backward
        ref = torch.cat(refs[i], 1)
        g = dqkv[:n_real, i * dm:(i + 1) * dm].view(n_real, H, hd).transpose(0, 1)
        assert (g - ref).abs().max() < 0.05 * ref.abs().max(), (i, float((g - ref).abs().max()), float(ref.abs().max()))
    assert dropped_rows >= 1                                                         # the length-1 segment loses its only key in one of the heads


# ------------------------------------------------------------------------------------------------------------------ 3. refused arguments
def test_varlen_dropout_refused_arguments():
    H, hd = 2, 16
    lengths = [33, 5]
    p, T, cu = pack_shape(lengths, pad_id=0)
    w = p.attn_work()

    def attempt(hd_, prob, cos=None, sin=None, fwd=True, bwd=True):
        q, k, v = (torch.randn(H, T, hd_).to(torch.bfloat16).to(DEV) for _ in range(3))
        ctx = torch.full((T, H * hd_), NAN, dtype=torch.bfloat16, device=DEV)
        lse = torch.full((H, T), NAN, device=DEV)
        dqkv = torch.full((T, 3 * H * hd_), NAN, dtype=torch.bfloat16, device=DEV)
        dctx = torch.zeros(T, H * hd_, dtype=torch.bfloat16, device=DEV)
        ws = torch.empty(hip.query("oneprot_attn_varlen_bwd_workspace", H, T), dtype=torch.uint8, device=DEV)
        if fwd:
            assert _rc("oneprot_attn_varlen_fwd_dropout", q, k, v, p.cu_seqlens, w, w.shape[0], ctx, lse, len(p), T, H, hd_, prob, 1, 2) == -1
        if bwd:
            assert _rc("oneprot_attn_varlen_bwd_dropout", q, k, v, p.cu_seqlens, w, w.shape[0], ctx, dctx, lse, cos, sin, hd_ ** -0.5, dqkv, ws, len(p), T, H,
                       hd_, prob, 1, 2) == -1
        torch.cuda.synchronize()
        # nothing was launched: not even the tail rows were zeroed
        assert torch.isnan(ctx.float()).all() and torch.isnan(lse).all() and torch.isnan(dqkv.float()).all()

    for prob in (1.0, -0.1, NAN):
        attempt(hd, prob)
    attempt(24, 0.1)
    half = torch.ones(T, hd // 2, device=DEV)
    attempt(hd, 0.1, cos=half, sin=None, fwd=False)
    attempt(hd, 0.1, cos=None, sin=half, fwd=False)


# ------------------------------------------------------------------------------------------------------------------ 4. packed embedding
def _bert_dir(tmp, name, hidden, heads, max_pos, vocab=120, layers=2, ffn=None, **extra):
    path = os.path.join(str(tmp), name)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                       intermediate_size=ffn or 2 * hidden, max_position_embeddings=max_pos, pad_token_id=0, layer_norm_eps=1e-12, **extra), f)
    return path


def _captions(lengths, vocab, seed):
    """caption ids: [CLS] = 2, body 5 .. vocab-1, [SEP] = 3 (a caption of one token is a lone [CLS])"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in lengths:
        s = torch.randint(5, vocab, (n,), generator=gen)
        s[0] = 2
        if n > 1:
            s[n - 1] = 3
        out.append(s)
    return out


def _pad_rows(seqs, pad=0):
    ids = torch.full((len(seqs), max(s.numel() for s in seqs)), pad, dtype=torch.int64)
    for b, s in enumerate(seqs):
        ids[b, :s.numel()] = s
    return ids


@pytest.fixture
def random_init(monkeypatch):
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")


def test_packed_bert_embedding_forward_backward(tmp_path, random_init):
    """d = 64, vocab 120, 64 positions; lengths [1, 5, 64, 3] in a 256-row stream: position 63 is reached by one segment only, token ids repeat
    across segments.  Forward through the C ABI, backward through the tower's _embedding_backward, both against torch."""
    from oneprot_amd import bert
    torch.manual_seed(7)
    d, V, n_pos, eps = 64, 120, 64, 1e-12
    lengths = [1, 5, 64, 3]
    seqs = _captions(lengths, V, 3)
    seqs[1][2] = seqs[2][10] = seqs[3][1] = 17                     # one token id in three segments
    p = PackedTokens.from_list(seqs, pad_id=0, t_pad=256).to(DEV)
    T, cu = p.T_pad, cu_of(lengths)
    tr = bert.BertTransformer(bert.ModelConfig(**dict(bert.BERT_DEFAULTS, vocab_size=V, hidden_size=d, num_hidden_layers=1, num_attention_heads=4,
                                                      intermediate_size=128, max_position_embeddings=n_pos, layer_norm_eps=eps))).to(DEV)
    e = "embeddings."
    with torch.no_grad():
        tr.view(e + "word_embeddings.weight").normal_()
        tr.view(e + "position_embeddings.weight").normal_()
        tr.view(e + "token_type_embeddings.weight").normal_()
        tr.view(e + "LayerNorm.weight").uniform_(0.5, 1.5)
        tr.view(e + "LayerNorm.bias").normal_(0, 0.1)
    word, pos, typ, gamma, beta = (tr.view(e + n).detach().cpu().clone() for n in ("word_embeddings.weight", "position_embeddings.weight",
                                                                                    "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias"))
    outs = []
    for _ in range(2):
        x = torch.full((T, d), NAN, device=DEV)
        x16 = torch.empty(T, d, dtype=torch.bfloat16, device=DEV)
        hip.call("oneprot_bert_embed_packed_fwd", p.ids, p.cu_seqlens, tr.view(e + "word_embeddings.weight"), tr.view(e + "position_embeddings.weight"),
                 tr.view(e + "token_type_embeddings.weight"), tr.view(e + "LayerNorm.weight"), tr.view(e + "LayerNorm.bias"), x, x16, len(p), T, d, V, n_pos, eps)
        outs.append((x, x16))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    x, x16 = outs[0][0].cpu(), outs[0][1].cpu()
    ids = p.ids.cpu()
    pos_idx = torch.zeros(T, dtype=torch.long)
    for a, n in zip(cu[:-1], lengths):
        pos_idx[a:a + n] = torch.arange(n)
    wr, pr, tr_, gr, br = (t.clone().requires_grad_() for t in (word, pos, typ, gamma, beta))
    ref = torch.nn.functional.layer_norm(wr[ids] + pr[pos_idx] + tr_[0], (d,), gr, br, eps)
    assert torch.isfinite(x).all()
    assert (x - ref.detach()).abs().max() < 1e-5                                  # the tail too: LN(word[pad] + pos[0] + type[0])
    assert torch.equal(x16, x.to(torch.bfloat16))
    # backward
    n_real = cu[-1]
    g = torch.randn(T, d)
    g[n_real:] = 0                                                                # what the tower hands over: zero gradient rows on the tail
    (ref * g).sum().backward()
    grads = []
    for _ in range(2):
        gflat = torch.zeros(tr._total, device=DEV)
        with torch.no_grad():
            tr._embedding_backward(bert.layout.of(tr, p), g.to(DEV), gflat)
        grads.append(gflat)
    torch.cuda.synchronize()
    assert torch.equal(grads[0], grads[1])
    got = {n: tr.view(e + n, grads[0]).cpu() for n in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                                                       "LayerNorm.weight", "LayerNorm.bias")}
    wref = wr.grad.clone()
    wref[0] = 0                                                                   # padding_idx row (nn.Embedding semantics)
    tref = torch.zeros_like(typ)
    tref[0] = tr_.grad[0]
    for name, r in (("word_embeddings.weight", wref), ("position_embeddings.weight", pr.grad), ("token_type_embeddings.weight", tref),
                    ("LayerNorm.weight", gr.grad), ("LayerNorm.bias", br.grad)):
        assert (got[name] - r).abs().max() < 1e-3 * r.abs().max(), (name, float((got[name] - r).abs().max()), float(r.abs().max()))
    assert (got["word_embeddings.weight"][0] == 0).all()
    # the position sum by itself: NaN in the tail rows of de is never read; rows no segment reaches are written as zeros
    de = torch.randn(T, d)
    de_nan = de.clone()
    de_nan[n_real:] = NAN
    res = []
    for src in (de, de_nan, de_nan):
        dpos = torch.full((n_pos, d), 5.0, device=DEV)
        hip.call("oneprot_segment_possum_f32", src.to(DEV), p.cu_seqlens, dpos, len(p), T, n_pos, d)
        res.append(dpos)
    torch.cuda.synchronize()
    assert torch.equal(res[0], res[1]) and torch.equal(res[1], res[2])
    want = torch.zeros(n_pos, d, dtype=torch.float64)
    for a, n in zip(cu[:-1], lengths):
        want[:n] += de[a:a + n].double()
    assert (res[0].cpu().double() - want).abs().max() < 1e-5
    assert torch.equal(res[0][63].cpu(), de[cu[2] + 63])                         # one segment only: the row itself
    short = PackedTokens.from_list([seqs[0], seqs[1], seqs[3]], pad_id=0, t_pad=256).to(DEV)      # max_len 5 of 64 rows asked for
    dpos = torch.full((n_pos, d), 5.0, device=DEV)
    hip.call("oneprot_segment_possum_f32", de_nan.to(DEV), short.cu_seqlens, dpos, len(short), T, n_pos, d)
    torch.cuda.synchronize()
    assert (dpos[5:] == 0).all() and torch.isfinite(dpos).all() and dpos[:5].abs().min() > 0


# ------------------------------------------------------------------------------------------------------------------ 5. packed pooling
@pytest.mark.parametrize("mode", [0, 1], ids=["mean", "cls"])
def test_packed_pooling_without_layernorm(mode):
    torch.manual_seed(5 + mode)
    lengths, d = [1, 7, 130], 64
    seqs = _captions(lengths, 120, 11)
    seqs[2][40] = 0                                                               # a pad id inside a segment: left out of the mean, as oneprot_pool_fwd does
    p = PackedTokens.from_list(seqs, pad_id=0).to(DEV)
    N, T, cu = len(p), p.T_pad, cu_of(lengths)
    x = torch.randn(T, d)
    dpooled = torch.randn(N, d)
    pooled = torch.empty(N, d, device=DEV)
    g = torch.full((T, d), 9.0, device=DEV)
    g16 = torch.full((T, d), 9.0, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_pool_packed_fwd", x.to(DEV), p.ids, p.cu_seqlens, 0, pooled, N, T, d, mode)
    hip.call("oneprot_pool_packed_bwd", dpooled.to(DEV), p.ids, p.cu_seqlens, 0, g, g16, N, T, d, mode)
    torch.cuda.synchronize()
    xr = x.clone().requires_grad_()
    refs = []
    for a, n, s in zip(cu[:-1], lengths, seqs):
        seg = xr[a:a + n]
        if mode == 0:
            m = (s != 0).float()[:, None]
            refs.append((seg * m).sum(0) / m.sum())
        else:
            refs.append(seg[0])
    ref = torch.stack(refs)
    (ref * dpooled).sum().backward()
    assert (pooled.cpu() - ref.detach()).abs().max() < 1e-4 * max(1.0, float(ref.abs().max()))
    assert (g.cpu() - xr.grad).abs().max() < 1e-4 * max(1.0, float(xr.grad.abs().max()))
    assert (g[cu[-1]:] == 0).all() and (g16[cu[-1]:] == 0).all()
    assert torch.equal(g16.cpu(), g.cpu().to(torch.bfloat16))
    if mode == 0:
        assert (g[cu[2] + 40] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 6. the tower, eval mode
TOWERS = {"hd16": dict(hidden=64, heads=4, max_pos=64, lengths=[9, 4, 64, 1]), "hd64": dict(hidden=128, heads=2, max_pos=512, lengths=[300, 17, 130])}


def _text_encoder(path, pooling="mean", frozen=True, seed=0, **kw):
    from oneprot_amd.encoders import TextEncoder
    torch.manual_seed(seed)
    return TextEncoder(path, output_dim=32, pooling_type=pooling, proj_type="linear", use_logit_scale=True, frozen=frozen, **kw).to(DEV)


def _tower_batch(name, tmp_path, **extra):
    t = TOWERS[name]
    path = _bert_dir(tmp_path, name, t["hidden"], t["heads"], t["max_pos"], **extra)
    seqs = _captions(t["lengths"], 120, 31)
    return path, _pad_rows(seqs).to(DEV), PackedTokens.from_list(seqs, pad_id=0).to(DEV)


def _assert_features_close(a, b):
    cs = torch.nn.functional.cosine_similarity(a.float(), b.float(), dim=-1)
    assert cs.min() >= 0.999, cs
    assert (a - b).abs().max() < 0.05 * a.abs().max()


@pytest.mark.parametrize("pooling", ["mean", "cls"])
@pytest.mark.parametrize("name", list(TOWERS))
def test_text_features_padded_vs_packed_eval(tmp_path, random_init, name, pooling):
    path, padded, packed = _tower_batch(name, tmp_path)
    enc = _text_encoder(path, pooling).eval()
    with torch.no_grad():
        a, b = enc(padded), enc(packed)
        hidden = enc.transformer(packed).last_hidden_state
    assert b.shape == (len(packed), 32)
    _assert_features_close(a, b)
    assert hidden.shape == (packed.T_pad, enc.transformer.d) and torch.isfinite(hidden).all()


def test_text_features_padded_vs_packed_attention1d(tmp_path, random_init):
    from oneprot_amd.encoders import Attention1dPooling
    path, padded, packed = _tower_batch("hd16", tmp_path)
    enc = _text_encoder(path, "mean")
    enc.pooling = Attention1dPooling(64).to(DEV)                   # (the constructor hard-codes 1280, as the reference does)
    enc = enc.eval()
    with torch.no_grad():
        _assert_features_close(enc(padded), enc(packed))


def _loss_and_grads(enc, ids, seq_feats):
    from oneprot_amd.loss import ClipLoss
    tr = enc.transformer
    tr.flat.grad = None
    for p_ in enc.parameters():
        p_.grad = None
    feats = enc(ids)
    loss = ClipLoss()(seq_feats, feats)
    loss.backward()
    grads = {}
    if tr.flat.grad is not None:
        grads["arena"] = tr.flat.grad.detach().clone()
    if getattr(tr, "_lora", None):
        grads["lora"] = torch.cat([tr.lora_A.grad.flatten(), tr.lora_B.grad.flatten()])
    grads["head"] = torch.cat([p_.grad.flatten() for p_ in enc.proj.parameters()])
    return float(loss.detach()), feats.detach(), grads


def _seq_feats(n):
    gen = torch.Generator().manual_seed(77)
    return torch.nn.functional.normalize(torch.randn(n, 32, generator=gen), dim=-1).to(DEV)


@pytest.mark.parametrize("lora", [False, True])
@pytest.mark.parametrize("name", list(TOWERS))
def test_trainable_text_tower_padded_vs_packed(tmp_path, random_init, name, lora):
    path, padded, packed = _tower_batch(name, tmp_path)
    kw = dict(use_lora=True, lora_dropout=0.0) if lora else {}
    enc = _text_encoder(path, "mean", frozen=False, **kw)
    enc.transformer.train_dropout = False
    if lora:
        with torch.no_grad():
            enc.transformer.lora_B.normal_(0, 0.05)                # (peft starts B at zero: dA would be zero and say nothing)
    sf = _seq_feats(len(packed))
    l_pad, f_pad, g_pad = _loss_and_grads(enc, padded, sf)
    l_pk, f_pk, g_pk = _loss_and_grads(enc, packed, sf)
    _assert_features_close(f_pad, f_pk)
    assert abs(l_pad - l_pk) / abs(l_pad) < 1e-3, (l_pad, l_pk)
    assert set(g_pad) == set(g_pk) and ("lora" if lora else "arena") in g_pad
    for k_ in g_pad:
        assert float(g_pad[k_].abs().max()) > 0, k_
        assert cos_sim(g_pad[k_], g_pk[k_]) >= 0.999, (k_, cos_sim(g_pad[k_], g_pk[k_]))


def _golden_encoder(golden_dir, fname, tmp_path, **kw):
    from src.models.components.text_encoder import TextEncoder
    g = torch.load(os.path.join(golden_dir, fname), weights_only=False)
    cfg = g["cfg"]
    path = os.path.join(str(tmp_path), "bert")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                       intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], pad_token_id=cfg["pad"], layer_norm_eps=cfg["eps"]), f)
    enc = TextEncoder(path, output_dim=cfg["output_dim"], use_logit_scale=True, learnable_logit_scale=False, use_lora=False, **kw)
    enc.transformer.train_dropout = False
    enc.load_state_dict(g["sd"], strict=True)
    packed = PackedTokens.from_padded(g["ids"], pad_id=cfg["pad"])
    assert torch.equal(packed.to_padded(g["ids"].shape[1]), g["ids"])            # the golden's rows are right-padded
    return g, cfg, enc.to(DEV), packed.to(DEV)


def test_packed_text_encoder_vs_reference(golden_dir, tmp_path, random_init):
    """tests/test_step_parity_gpu.py::test_text_encoder_vs_reference on the packed form of the same captions, the same assertions"""
    g, cfg, enc, packed = _golden_encoder(golden_dir, "bert_text.pt", tmp_path, pooling_type="cls", proj_type="mlp", frozen=True)
    enc = enc.eval()
    with torch.no_grad():
        feats = enc(packed).cpu()
        hidden = enc.transformer(input_ids=packed).last_hidden_state.cpu()
    ref_h = g["acts"]["last_hidden"]
    worst = 0.0
    for b, (a, n) in enumerate(zip(cu_of(packed.lengths)[:-1], packed.lengths)):
        worst = max(worst, float((hidden[a:a + n] - ref_h[b, :n]).abs().max()))
    assert worst < 0.05 * ref_h.abs().max()
    cs = torch.nn.functional.cosine_similarity(feats, g["features"], dim=-1)
    assert cs.min() > 0.999, cs
    assert abs(feats.norm(dim=-1) - 1 / 0.07).max() < 1e-3


def test_packed_trainable_text_encoder_gradients_vs_reference(golden_dir, tmp_path, random_init):
    """tests/test_step_parity_gpu.py::test_trainable_text_encoder_gradients_vs_reference on the packed form, the same assertions"""
    from src.models.components.loss import ClipLoss
    g, cfg, enc, packed = _golden_encoder(golden_dir, "bert_text_train.pt", tmp_path, pooling_type="mean", proj_type="linear", frozen=False)
    feats = enc(packed)
    cs = torch.nn.functional.cosine_similarity(feats.detach().cpu(), g["features"], dim=-1)
    assert cs.min() > 0.999, cs
    loss = ClipLoss()(g["seq_features"].to(DEV), feats)
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < 2e-3, (float(loss), float(g["loss"]))
    loss.backward()
    tr = enc.transformer
    got = {"transformer." + k: tr.view(k, tr.flat.grad).detach().cpu() for k in tr._spec}
    got.update({"proj." + k: p_.grad.detach().cpu() for k, p_ in enc.proj.named_parameters()})
    n = 0
    for k, ref in g["grads"].items():
        assert k in got, k
        if float(ref.norm()) < 1e-6:
            continue
        c = cos_sim(got[k], ref)
        assert c > 0.98, (k, c)
        if float(ref.norm()) > 0.05 * max(float(v.norm()) for v in g["grads"].values()):
            assert c > 0.999, (k, c)
        n += 1
    assert n >= 38
    wg = got["transformer.embeddings.word_embeddings.weight"]
    assert float(wg[cfg["pad"]].abs().max()) == 0.0
    unused = [r for r in range(cfg["vocab"]) if r not in set(g["ids"].flatten().tolist())]
    assert float(wg[unused].abs().max()) == 0.0
    allg = torch.cat([got[k].flatten() for k in g["grads"]]); allr = torch.cat([v.flatten() for v in g["grads"].values()])
    assert cos_sim(allg, allr) > 0.9995


# ------------------------------------------------------------------------------------------------------------------ 7. the tower, train mode
@pytest.mark.parametrize("name", list(TOWERS))
def test_train_mode_attention_dropout_padded_vs_packed(tmp_path, random_init, name):
    """hidden dropout off, attention-probability dropout 0.1: the packed masks are the padded batch's, so features and gradients agree as in eval mode"""
    path, padded, packed = _tower_batch(name, tmp_path, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.1)
    enc = _text_encoder(path, "mean", frozen=False).train()
    tr = enc.transformer
    tr.train_dropout = True
    sf = _seq_feats(len(packed))
    res = []
    for ids in (padded, packed):
        tr._drop_seed, tr._drop_calls = 99, 0
        res.append(_loss_and_grads(enc, ids, sf))
    (l_pad, f_pad, g_pad), (l_pk, f_pk, g_pk) = res
    _assert_features_close(f_pad, f_pk)
    assert abs(l_pad - l_pk) / abs(l_pad) < 1e-3, (l_pad, l_pk)
    for k_ in g_pad:
        assert cos_sim(g_pad[k_], g_pk[k_]) >= 0.999, (k_, cos_sim(g_pad[k_], g_pk[k_]))
    enc.eval()
    with torch.no_grad():
        assert not torch.allclose(enc(packed), f_pk, atol=1e-4)     # the dropout did act


@pytest.mark.parametrize("frozen", [True, False])
def test_train_mode_all_four_dropouts_packed(tmp_path, random_init, frozen):
    path, padded, packed = _tower_batch("hd16", tmp_path)           # BERT's defaults: p = 0.1 for all four
    enc = _text_encoder(path, "mean", frozen=frozen).train()
    tr = enc.transformer
    assert (float(tr.config.hidden_dropout_prob), float(tr.config.attention_probs_dropout_prob)) == (0.1, 0.1)
    sf = _seq_feats(len(packed))
    runs = []
    for _ in range(2):
        tr._drop_seed, tr._drop_calls = 123, 5
        runs.append(_loss_and_grads(enc, packed, sf))
    third = _loss_and_grads(enc, packed, sf)                        # call 6: new masks
    (l0, f0, g0), (l1, f1, g1) = runs
    assert torch.isfinite(f0).all() and all(torch.isfinite(v).all() for v in g0.values())
    assert ("arena" in g0) == (not frozen)
    assert torch.equal(f0, f1) and l0 == l1 and all(torch.equal(g0[k_], g1[k_]) for k_ in g0)
    assert not torch.allclose(third[1], f0, atol=1e-4)
    enc.eval()
    with torch.no_grad():
        assert not torch.allclose(enc(packed), f0, atol=1e-4)


def test_train_mode_backward_twice_from_one_saved_forward(tmp_path, random_init):
    """every mask is regenerated in the backward: two backward passes over the same saved forward give the same bits"""
    path, padded, packed = _tower_batch("hd16", tmp_path)
    enc = _text_encoder(path, "mean", frozen=False).train()
    tr = enc.transformer
    tr._drop_seed, tr._drop_calls = 5, 0
    assert tr._train_dropout()
    x, saved = tr.run_layers(packed, save=True)
    assert "drop_call" in saved
    T, d = packed.T_pad, tr.d
    g = torch.randn(T, d, device=DEV)
    g[packed.n_tokens:] = 0
    outs = []
    for s in (dict(saved, layers=list(saved["layers"])), saved):
        gflat = torch.zeros(tr._total, device=DEV)
        with torch.no_grad():
            tr.backward_layers(s, g.clone(), None, gflat)
        outs.append(gflat)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------ 8. pack composition
def test_text_features_independent_of_pack_composition(tmp_path, random_init):
    path = _bert_dir(tmp_path, "bert", 128, 2, 512)
    enc = _text_encoder(path, "mean").eval()
    mk = lambda n, seed: _captions([n], 120, seed)[0]
    target = mk(200, 1)
    a = PackedTokens.from_list([target, mk(100, 2), mk(300, 3)], pad_id=0, t_pad=1024).to(DEV)
    b = PackedTokens.from_list([mk(37, 4), mk(511, 5), target, mk(5, 6)], pad_id=0, t_pad=1024).to(DEV)
    with torch.no_grad():
        fa, fb = enc(a), enc(b)
    assert torch.equal(fa[0], fb[2])


# ------------------------------------------------------------------------------------------------------------------ 9. the module
def test_module_substep_both_sides_packed(tmp_path, random_init):
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.encoders import SequenceEncoder, TextEncoder
    from oneprot_amd.module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    esm = os.path.join(str(tmp_path), "esm")
    os.makedirs(esm)
    with open(os.path.join(esm, "config.json"), "w") as f:
        json.dump(dict(model_type="esm", vocab_size=33, hidden_size=320, num_hidden_layers=4, num_attention_heads=20, intermediate_size=1280), f)
    bert = _bert_dir(tmp_path, "bert", 256, 4, 512, vocab=1000, ffn=512)

    def build():
        torch.manual_seed(3)
        seq = SequenceEncoder(esm, output_dim=128, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
        txt = TextEncoder(bert, output_dim=128, pooling_type="mean", proj_type="linear", use_logit_scale=True, frozen=True)
        txt.transformer.train_dropout = False
        return OneProtLitModule(components={"sequence": seq, "text": txt}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                                use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(DEV)

    rag = next(iter(SyntheticPairs("text", 12, 200, ragged=True, text_vocab=1000)))
    pk = next(iter(SyntheticPairs("text", 12, 200, packed=True, packed_text=True, text_vocab=1000)))
    assert isinstance(pk[0], PackedTokens) and isinstance(pk[1], PackedTokens) and pk[1].pad_id == 0
    l_pad = float(build().training_step({"text": (rag[0].to(DEV), rag[1].to(DEV), "text", None)}, 0))
    l_pk = float(build().training_step({"text": (pk[0].to(DEV), pk[1].to(DEV), "text", None)}, 0))
    assert abs(l_pad - l_pk) / abs(l_pad) < 1e-3, (l_pad, l_pk)
    five = PackedTokens.from_padded(rag[1][:5], pad_id=0)
    with pytest.raises(ValueError, match="same number"):
        build().training_step({"text": (pk[0].to(DEV), five.to(DEV), "text", None)}, 0)
