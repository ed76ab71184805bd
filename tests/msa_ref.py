"""Restatement of the published MSA Transformer forward (esm_msa1b_t12_100M_UR50S architecture, eval mode) in plain torch, fp64 by default: the
reference the MSA tests compare the HIP tower against.  A helper module like tests/philox_ref.py, not a test.

PARITY UNPINNED: fair-esm is not available here and there is no checkpoint, so nothing below was run against it.  Every rule is restated from the published
model (Rao et al. 2021, "MSA Transformer"; fair-esm MSATransformer / AxialTransformerLayer / RowSelfAttention / ColumnSelfAttention /
LearnedPositionalEmbedding), in particular:
  * positions = cumsum(non-pad) * non-pad + padding_idx per row, table of max_positions + padding_idx + 1 rows;
  * the MSA-row embedding [1, 1024, 1, d] indexed by r; emb_layer_norm_before, then x * non-pad;
  * layer = three pre-LN residual blocks: tied row attention, column attention, FFN (erf-GELU); LN eps 1e-5; emb_layer_norm_after at the end;
  * tied row attention: q scaled by hd^-1/2 / sqrt(R) with R the PADDED row count, q zeroed at padded positions, scores summed over rows, keys masked
    (-10000) where ROW 0 is padded;
  * column attention: for R = 1 out_proj(v_proj(x)); else q scaled by hd^-1/2, keys (j, l) that are padding get -10000.
State-dict keys are the published module keys (oneprot_amd/msa.py)."""
import math

import torch
import torch.nn.functional as F

PAD = 1


def positions(tokens, pad=PAD):
    m = tokens.ne(pad).long()
    return torch.cumsum(m, dim=-1) * m + pad


def _ln(x, sd, p, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _lin(x, sd, p):
    return x @ sd[p + ".weight"].T + sd[p + ".bias"]


def embed(tokens, sd, pad=PAD):
    R = tokens.shape[1]
    x = sd["embed_tokens.weight"][tokens] + sd["embed_positions.weight"][positions(tokens, pad)] + sd["msa_position_embedding"][:, :R]
    x = _ln(x, sd, "emb_layer_norm_before")
    return x * tokens.ne(pad).unsqueeze(-1).to(x.dtype)


def row_scores(q, k, pad_mask, H):
    """q, k: the projections [B, R, L, H * hd]; pad_mask bool [B, R, L] -> S [B, H, L, L] (before the key mask)"""
    B, R, L, D = q.shape
    hd = D // H
    q = q.reshape(B, R, L, H, hd) * (hd ** -0.5 / math.sqrt(R))
    q = q * (~pad_mask)[..., None, None].to(q.dtype)
    return torch.einsum("brihc,brjhc->bhij", q, k.reshape(B, R, L, H, hd))


def row_scores_loop(q, k, pad_mask, H):
    """the same sum with the rows taken one at a time"""
    B, R, L, D = q.shape
    hd = D // H
    S = torch.zeros(B, H, L, L, dtype=q.dtype, device=q.device)
    for r in range(R):
        qr = q[:, r].reshape(B, L, H, hd) * (hd ** -0.5 / math.sqrt(R)) * (~pad_mask[:, r])[..., None, None].to(q.dtype)
        S = S + torch.einsum("bihc,bjhc->bhij", qr, k[:, r].reshape(B, L, H, hd))
    return S


def row_probs(S, pad_mask):
    return torch.softmax(S.masked_fill(pad_mask[:, 0][:, None, None, :], -10000.0), dim=-1)


def row_context(S, v, pad_mask, H, p_round=None):
    """ctx [B, R, L, H * hd]; p_round: optional rounding applied to the probabilities (the kernels hold them in bf16)"""
    B, R, L, D = v.shape
    P = row_probs(S, pad_mask)
    if p_round is not None:
        P = p_round(P)
    return torch.einsum("bhij,brjhc->brihc", P, v.reshape(B, R, L, H, D // H)).reshape(B, R, L, D)


def col_scores(q, k, H):
    """S [B, H, L, R, R] of the column attention (before the key mask): S[b, h, l, i, j] = hd^-1/2 q[b, i, l, h] . k[b, j, l, h]"""
    B, R, L, D = q.shape
    hd = D // H
    return torch.einsum("bilhc,bjlhc->bhlij", q.reshape(B, R, L, H, hd) * hd ** -0.5, k.reshape(B, R, L, H, hd))


def col_context(q, k, v, pad_mask, H, general=False):
    """ctx [B, R, L, H * hd] of the column attention; R = 1 takes the published shortcut (ctx = v) unless `general`"""
    B, R, L, D = q.shape
    hd = D // H
    if R == 1 and not general:
        return v
    S = col_scores(q, k, H).masked_fill(pad_mask.permute(0, 2, 1)[:, None, :, None, :], -10000.0)
    return torch.einsum("bhlij,bjlhc->bilhc", torch.softmax(S, dim=-1), v.reshape(B, R, L, H, hd)).reshape(B, R, L, D)


def layer(x, sd, i, pad_mask, H, taps=None):
    p = f"layers.{i}."
    a = p + "row_self_attention."
    h = _ln(x, sd, a + "layer_norm")
    q, k, v = (_lin(h, sd, a + f"layer.{n}_proj") for n in "qkv")
    ctx = row_context(row_scores(q, k, pad_mask, H), v, pad_mask, H)
    if taps is not None:
        taps.append(("row", i, ctx))
    x = x + _lin(ctx, sd, a + "layer.out_proj")
    a = p + "column_self_attention."
    h = _ln(x, sd, a + "layer_norm")
    q, k, v = (_lin(h, sd, a + f"layer.{n}_proj") for n in "qkv")
    ctx = col_context(q, k, v, pad_mask, H)
    if taps is not None:
        taps.append(("col", i, ctx))
    x = x + _lin(ctx, sd, a + "layer.out_proj")
    a = p + "feed_forward_layer."
    h = _ln(x, sd, a + "layer_norm")
    return x + _lin(F.gelu(_lin(h, sd, a + "layer.fc1")), sd, a + "layer.fc2")


# The blocks of `layer` one stage at a time, each from that stage's own input (the per-stage tower test hands them what the tower captured).  `rnd`: optional
# rounding applied where the tower holds a bf16 tensor (LayerNorm output, GELU output); chained without it they are `layer` (tests/test_msa_cpu.py).
def qkv_proj(x, sd, i, blk, rnd=None):
    """x [.., d] -> the q | k | v projections of LN(x) side by side [.., 3 d]: one product with the stacked weights; blk: row_self_attention / column_self_attention"""
    a = f"layers.{i}.{blk}."
    h = _ln(x, sd, a + "layer_norm")
    h = h if rnd is None else rnd(h)
    w = torch.cat([sd[a + f"layer.{n}_proj.weight"] for n in "qkv"])
    return h @ w.T + torch.cat([sd[a + f"layer.{n}_proj.bias"] for n in "qkv"])


def attn_out(x, ctx, sd, i, blk):
    return x + _lin(ctx, sd, f"layers.{i}.{blk}.layer.out_proj")


def ffn(x, sd, i, rnd=None):
    a = f"layers.{i}.feed_forward_layer."
    h = _ln(x, sd, a + "layer_norm")
    u = F.gelu(_lin(h if rnd is None else rnd(h), sd, a + "layer.fc1"))
    return x + _lin(u if rnd is None else rnd(u), sd, a + "layer.fc2")


GEMM_WEIGHTS = ("_proj.weight", "fc1.weight", "fc2.weight")


def tower_operands(sd, rnd, dtype=torch.float64):
    """the state dict as the tower reads it: the GEMM weights through `rnd` (its bf16 mirror), LayerNorms, biases and tables as they are"""
    return {k: (rnd(v.detach().cpu()) if k.endswith(GEMM_WEIGHTS) else v.detach().cpu().to(dtype)) for k, v in sd.items() if v.is_floating_point()}


def ffn_rounding_self_difference(tokens, sd, heads, rnd, pad=PAD):
    """The reference against itself: per layer, max |ffn with `rnd` on the LayerNorm and GELU outputs - ffn exact| from the same FFN input, along the forward with
    `rnd` wherever the tower holds a bf16 tensor.  What a bf16 tie flip between an fp32 and an fp64 LayerNorm can at most do to the FFN stage is a fraction of it."""
    sd = tower_operands(sd, rnd)
    n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    pad_mask = tokens.eq(pad)
    x, out = embed(tokens, sd, pad), []
    for i in range(n_layers):
        q, k, v = rnd(qkv_proj(x, sd, i, "row_self_attention", rnd)).chunk(3, dim=-1)
        x = attn_out(x, rnd(row_context(row_scores(q, k, pad_mask, heads), v, pad_mask, heads)), sd, i, "row_self_attention")
        q, k, v = rnd(qkv_proj(x, sd, i, "column_self_attention", rnd)).chunk(3, dim=-1)
        x = attn_out(x, rnd(col_context(q, k, v, pad_mask, heads)), sd, i, "column_self_attention")
        y = ffn(x, sd, i, rnd)
        out.append(float((y - ffn(x, sd, i)).abs().max()))
        x = y
    return out


def forward(tokens, sd, heads, dtype=torch.float64, pad=PAD, taps=None):
    """tokens int64 [B, R, L]; sd: state dict with the published keys -> the last representation [B, R, L, d] (after emb_layer_norm_after)"""
    sd = {k: v.to(device=tokens.device, dtype=dtype) for k, v in sd.items() if v.is_floating_point()}
    n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    pad_mask = tokens.eq(pad)
    x = embed(tokens, sd, pad)
    for i in range(n_layers):
        x = layer(x, sd, i, pad_mask, heads, taps)
    return _ln(x, sd, "emb_layer_norm_after")


def encoder_features(tokens, enc_sd, heads, use_all_msa, pooling, dtype=torch.float64, pad=PAD):
    """MsaEncoder.forward (ref msa_encoder.py:35-52) on an encoder state dict (transformer.*, proj.*, norm.*) -> (hidden [B, R, L, d], features [B, D])"""
    tr = {k[len("transformer."):]: v for k, v in enc_sd.items() if k.startswith("transformer.")}
    hid = forward(tokens, tr, heads, dtype, pad)
    m = tokens.ne(pad).to(dtype)
    if use_all_msa:
        pooled = (hid * m.unsqueeze(-1)).sum(dim=(1, 2)) / m.sum(dim=(1, 2)).unsqueeze(-1)
    elif pooling == "mean":
        pooled = (hid[:, 0] * m[:, 0].unsqueeze(-1)).sum(1) / m[:, 0].sum(1, keepdim=True)
    else:
        pooled = hid[:, 0, 0]
    g = lambda k: enc_sd[k].to(device=tokens.device, dtype=dtype)
    y = pooled
    if "proj.1.weight" in enc_sd:
        y = F.layer_norm(y, (y.shape[-1],), g("proj.0.weight"), g("proj.0.bias"), 1e-5) @ g("proj.1.weight").T
        if "proj.4.weight" in enc_sd:
            y = F.layer_norm(F.gelu(y), (y.shape[-1],), g("proj.3.weight"), g("proj.3.bias"), 1e-5) @ g("proj.4.weight").T
    y = F.normalize(y, dim=-1)
    if "norm.1.log_logit_scale" in enc_sd:
        y = y * min(math.exp(float(enc_sd["norm.1.log_logit_scale"])), 100.0)
    return hid, y
