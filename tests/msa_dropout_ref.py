"""The train-mode forward of the published MSA Transformer restated in fp64 on top of tests/msa_ref.py, with every dropout mask an INPUT: the reference
the MSA dropout tests compare the HIP tower against.  A helper module like tests/msa_ref.py and tests/philox_ref.py, not a test; it never calls a kernel.

PARITY UNPINNED, as in tests/msa_ref.py: restated from the published fair-esm modules, not run against them.
  * MSATransformer.forward: emb_layer_norm_before -> dropout(p = dropout) -> x * non-pad;
  * NormalizedResidualBlock (all three blocks of a layer): x = residual + dropout(layer(layer_norm(x))), p = dropout;
  * RowSelfAttention: probs = dropout(softmax(scores)), p = attention_dropout, on [H, B, L, L]: one mask element per (b, h, i, j) for all R rows;
  * ColumnSelfAttention, R > 1: the same on [H, L, B, R, R]; R = 1 is out_proj(v_proj(x)) with no attention dropout (the block's residual dropout applies);
  * FeedForwardNetwork: fc2(activation_dropout(gelu(fc1(x)))).
A mask is a pair (keep, scale): keep a bool (or 0 / 1) tensor of the site's shape, scale the factor of the kept values; None = no dropout at that site.

`tower_masks` builds the masks of one call of oneprot_amd.msa.MsaTransformer on the host from tests/philox_ref.py and the tower's own stream numbering
(`_drop_stream(call, layer, site)`; sites: layer -1 / 0 the embeddings; 0 row probabilities, 1 row-block output, 2 column probabilities, 3 column-block
output, 4 FFN activation, 5 FFN output).  Hidden masks index the flat [T, d] / [T, f] element, row masks are attn_keep(B, H, L, ...), column masks
attn_keep(B * H * L, 1, R, ...) viewed as [B, H, L, R, R]."""
import math

import torch
import torch.nn.functional as F

from tests import msa_ref as MR
from tests import philox_ref as PR

PAD = MR.PAD
SITES = dict(row_probs=0, row_out=1, col_probs=2, col_out=3, ffn_act=4, ffn_out=5)


def drop(x, mask):
    """dropout with a given mask: keep * scale * x"""
    if mask is None:
        return x
    keep, scale = mask
    return x * keep.to(device=x.device, dtype=x.dtype) * float(scale)


def row_context(S, v, pad_mask, H, mask=None):
    """MR.row_context with the probabilities dropped: mask = (keep [B, H, L, L], scale); sum and maximum are those of the undropped softmax"""
    B, R, L, D = v.shape
    P = drop(MR.row_probs(S, pad_mask), mask)
    return torch.einsum("bhij,brjhc->brihc", P, v.reshape(B, R, L, H, D // H)).reshape(B, R, L, D)


def col_context(q, k, v, pad_mask, H, mask=None, general=False):
    """MR.col_context with the probabilities dropped: mask = (keep [B, H, L, R, R], scale).  R = 1 takes the published shortcut, which has no dropout."""
    B, R, L, D = q.shape
    hd = D // H
    if R == 1 and not general:
        return v
    S = MR.col_scores(q, k, H).masked_fill(pad_mask.permute(0, 2, 1)[:, None, :, None, :], -10000.0)
    return torch.einsum("bhlij,bjlhc->bilhc", drop(torch.softmax(S, dim=-1), mask), v.reshape(B, R, L, H, hd)).reshape(B, R, L, D)


def embed(tokens, sd, mask=None, pad=PAD):
    R = tokens.shape[1]
    x = sd["embed_tokens.weight"][tokens] + sd["embed_positions.weight"][MR.positions(tokens, pad)] + sd["msa_position_embedding"][:, :R]
    x = drop(MR._ln(x, sd, "emb_layer_norm_before"), mask)
    return x * tokens.ne(pad).unsqueeze(-1).to(x.dtype)


def layer(x, sd, i, pad_mask, H, masks):
    """masks: {site name (SITES) or number: (keep, scale)}; a missing site is not dropped"""
    m = lambda name: masks.get(name, masks.get(SITES[name]))
    p = f"layers.{i}."
    a = p + "row_self_attention."
    h = MR._ln(x, sd, a + "layer_norm")
    q, k, v = (MR._lin(h, sd, a + f"layer.{n}_proj") for n in "qkv")
    ctx = row_context(MR.row_scores(q, k, pad_mask, H), v, pad_mask, H, m("row_probs"))
    x = x + drop(MR._lin(ctx, sd, a + "layer.out_proj"), m("row_out"))
    a = p + "column_self_attention."
    h = MR._ln(x, sd, a + "layer_norm")
    q, k, v = (MR._lin(h, sd, a + f"layer.{n}_proj") for n in "qkv")
    ctx = col_context(q, k, v, pad_mask, H, m("col_probs"))
    x = x + drop(MR._lin(ctx, sd, a + "layer.out_proj"), m("col_out"))
    a = p + "feed_forward_layer."
    h = MR._ln(x, sd, a + "layer_norm")
    u = drop(F.gelu(MR._lin(h, sd, a + "layer.fc1")), m("ffn_act"))
    return x + drop(MR._lin(u, sd, a + "layer.fc2"), m("ffn_out"))


def forward(tokens, sd, heads, masks, dtype=torch.float64, pad=PAD):
    """MR.forward in train mode.  masks: {(layer, site): (keep, scale)}, layer -1 / site 0 = the embedding dropout; missing entries are not dropped."""
    sd = {k: v.to(device=tokens.device, dtype=dtype) for k, v in sd.items() if v.is_floating_point()}
    n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    pad_mask = tokens.eq(pad)
    x = embed(tokens, sd, masks.get((-1, 0)), pad)
    for i in range(n_layers):
        x = layer(x, sd, i, pad_mask, heads, {s: masks[(i, s)] for s in SITES.values() if (i, s) in masks})
    return MR._ln(x, sd, "emb_layer_norm_after")


def encoder_features(tokens, enc_sd, heads, use_all_msa, pooling, masks, dtype=torch.float64, pad=PAD):
    """MR.encoder_features on the train-mode hidden state"""
    tr = {k[len("transformer."):]: v for k, v in enc_sd.items() if k.startswith("transformer.")}
    hid = forward(tokens, tr, heads, masks, dtype, pad)
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


# ---------------------------------------------------------------------------------------------------------------- masks on the host
def scale_of(p):
    return float(PR.dropout_threshold(p)[1])


def hidden_mask(shape, p, seed, stream):
    """(keep, scale) of the Philox kernels over the flat elements of a tensor of `shape`"""
    n = int(math.prod(shape))
    return torch.from_numpy(PR.philox_keep(n, p, seed, stream)).view(*shape), scale_of(p)


def row_mask(B, H, L, p, seed, stream, b_first=0):
    """(keep [B, H, L, L], scale) of the tied row attention: MSAs b_first .. b_first + B - 1 of the batch"""
    return torch.from_numpy(PR.attn_keep(b_first + B, H, L, p, seed, stream))[b_first:], scale_of(p)


def col_mask(B, H, L, R, p, seed, stream):
    """(keep [B, H, L, R, R], scale) of the column attention"""
    return torch.from_numpy(PR.attn_keep(B * H * L, 1, R, p, seed, stream)).view(B, H, L, R, R), scale_of(p)


def tower_masks(stream, shape, d, f, H, n_layers, probs, seed):
    """every mask of one train-mode call.  stream(layer, site) -> stream id (functools.partial(tower._drop_stream, call)); shape = (B, R, L);
    probs = (dropout, attention_dropout, activation_dropout)"""
    B, R, L = shape
    p_h, p_a, p_f = probs
    masks = {(-1, 0): hidden_mask((B, R, L, d), p_h, seed, stream(-1, 0))}
    for i in range(n_layers):
        masks[(i, 0)] = row_mask(B, H, L, p_a, seed, stream(i, 0))
        if R > 1:
            masks[(i, 2)] = col_mask(B, H, L, R, p_a, seed, stream(i, 2))
        for site in (1, 3, 5):
            masks[(i, site)] = hidden_mask((B, R, L, d), p_h, seed, stream(i, site))
        masks[(i, 4)] = hidden_mask((B, R, L, f), p_f, seed, stream(i, 4))
    return masks
