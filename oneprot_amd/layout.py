"""The padded / packed fork of the token towers, once on the host side (the device side is `row_seg` of csrc/rowops.hip and `AttnSlab`
of csrc/attention.hip).  A layout owns what depends on how the sequences lie in memory and nothing else: the geometry, the attention launches and the
pooling end (final LayerNorm + mean / CLS / attention1d pooling, forward and backward).  Every other stage of a tower runs row-wise on T = B * L rows.

    PaddedLayout   ids int64 [B, L]: N = B sequences of L rows; attention masks padding through the key-padding bias.
    PackedLayout   a PackedTokens stream (oneprot_amd.packing): ONE row-wise sequence of T_pad rows (B = 1, L = T_pad), N segments [cu[b], cu[b+1]) and a
                   tail of pad rows (finite activations, exactly zero gradient rows); attention runs per segment (varlen kernels: the segment end is
                   the only mask, no key-bias tensor is built).

The towers subclass both with their own embedding stages (esm.py: embed / embed_bwd; bert.py: embed / pos_rows / pos_bwd) and name the pair in
`tower.layouts`; `of(tower, ids)` picks.  Constructing a layout launches nothing."""
import torch

from . import hip
from .packing import PackedTokens


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def of(tr, ids):
    """the layout of `ids` for tower `tr`: tr.layouts = (padded class, packed class)"""
    padded, packed = tr.layouts
    return packed(tr, ids) if isinstance(ids, PackedTokens) else padded(tr, ids)


class _Layout:
    cos = sin = None          # rotary tables the attention backward un-rotates dq / dk with (ESM's embed sets them; None: BERT, no rotary)

    # ---- the pooling end: shared composition over the per-layout launches _lnpool / _pool / _attnpool (+ _bwd) below
    @staticmethod
    def _final_ln(tr, src=None):
        return tr.view("encoder.emb_layer_norm_after.weight", src), tr.view("encoder.emb_layer_norm_after.bias", src)

    def final_hidden(self, tr, x):
        """what a HF-style forward() returns: the (final-LayerNorm'ed, where the tower has one) hidden state, [B, L, d] or the stream's [T_pad, d]"""
        if getattr(tr, "final_layer_norm", True):
            hidden = torch.empty(self.T, tr.d, device=x.device)
            self._lnpool(tr, x, torch.empty(self.N, tr.d, device=x.device), (None, None, None), hidden, 0)
            x = hidden
        return x.view(*self.shape, tr.d)

    def pool_fwd(self, tr, x, pooling, keep):
        """Final LayerNorm + pooling of the last layer's output x fp32 [T, d] (a post-LN tower, final_layer_norm = False, pools x directly).
        Returns (pooled [N, d] in sequence order, (mean, rstd, wrow) per row for the LayerNorm backward when `keep`, (hidden, attn) of attention1d)."""
        d, dev, pad, mode = tr.d, x.device, tr.config.pad_token_id, pooling.mode
        final_ln = getattr(tr, "final_layer_norm", True)
        pooled = torch.empty(self.N, d, device=dev)
        fin = tuple(torch.empty(self.T, device=dev) for _ in range(3)) if (keep and final_ln) else (None, None, None)
        hidden = attn = None
        if mode == 2:                                   # attention1d: needs the normalised hidden state itself
            w = pooling.layer.weight
            if w.numel() != d:
                raise RuntimeError(f"Attention1dPooling was built for hidden size {w.numel()} but the encoder width is {d} "
                                   "(the reference hard-codes 1280: base_encoder.py:180)")
            hidden = x
            if final_ln:
                hidden = torch.empty(self.T, d, device=dev)
                self._lnpool(tr, x, pooled, fin, hidden, 0)
            attn = torch.empty(self.T, device=dev)
            self._attnpool(hidden, pad, w, pooling.layer.bias, pooled, attn, d)
        elif final_ln:
            self._lnpool(tr, x, pooled, fin, None, mode)
        else:
            self._pool(x, pad, pooled, d, mode)
        return pooled, fin, (hidden, attn)

    def attnpool_bwd(self, pool, w, dpooled, want_dx):
        """attention1d backward: (dw, db, gradient of the hidden state [T, d] or None); the packed form writes zeros into the tail rows"""
        hidden, attn = pool
        d, dev = hidden.shape[-1], hidden.device
        dw, db = torch.empty(d, device=dev), torch.empty(1, device=dev)
        dhidden = torch.empty(self.T, d, device=dev) if want_dx else None
        self._attnpool_bwd(hidden, attn, w, dpooled, dw, db, dhidden, _ws(hip.query("oneprot_attnpool_bwd_workspace", self.N, d), dev), d)
        return dw.view_as(w), db, dhidden

    def pool_bwd(self, tr, mode, dpooled, dhidden, fin, x_final, gflat):
        """(g fp32, g16 bf16) [T, d]: the gradient of the last layer's output from dpooled [N, d] (mean / CLS) or from attention1d's dhidden; the final
        LayerNorm's parameter gradients go into gflat"""
        d, dev = tr.d, dpooled.device
        g, g16 = torch.empty(self.T, d, device=dev), torch.empty(self.T, d, dtype=torch.bfloat16, device=dev)
        if not getattr(tr, "final_layer_norm", True):   # BERT: pooling reads the last layer's output directly
            if mode == 2:
                g.copy_(dhidden)      # (g16 stays unwritten: a post-LN tower's backward_layers starts with a LayerNorm backward on g and never reads it)
            else:
                self._pool_bwd(dpooled, tr.config.pad_token_id, g, g16, d, mode)
            return g, g16
        mean, rstd, wrow = fin
        lnw, (gw, gb) = self._final_ln(tr)[0], self._final_ln(tr, gflat)
        ws = _ws(hip.query("oneprot_layernorm_bwd_workspace", d), dev)
        if mode == 2:
            hip.layernorm_bwd(dhidden, 1, x_final, lnw, mean, rstd, g, gw, gb, ws, self.T, d, dx16=g16)
        else:                                           # dy[t] = dpooled[sequence of t] * wrow[t]
            self._lnpool_bwd(dpooled, wrow, x_final, lnw, mean, rstd, g, g16, gw, gb, ws, d)
        return g, g16


class PaddedLayout(_Layout):
    packed = False

    def __init__(self, tr, ids):
        self.ids = ids.contiguous()
        self.B, self.L = self.shape = tuple(ids.shape)
        self.T, self.N = self.B * self.L, self.B

    def make_key_bias(self, pad_id):
        """the additive key-padding bias of attention, fp32 [B, L]: one launch, from the tower's embed()"""
        self.key_bias = torch.empty(self.B, self.L, dtype=torch.float32, device=self.ids.device)
        hip.call("oneprot_key_padding_bias", self.ids, self.key_bias, self.T, pad_id)

    # drop = (p, seed, stream): attention-probability dropout (bert.py); None: the plain kernels
    def attn_fwd(self, q, k, v, ctx, lse, H, hd, drop=None):
        hip.call("oneprot_attn_fwd_dropout" if drop else "oneprot_attn_fwd", q, k, v, self.key_bias, ctx, lse, self.B, H, self.L, hd, *(drop or ()))

    def attn_workspace(self, H, dev):
        return torch.empty(hip.query("oneprot_attn_bwd_workspace", self.B, H, self.L), dtype=torch.uint8, device=dev)

    def attn_bwd(self, st, dctx, q_scale, dqkv, ws, H, hd, drop=None):
        hip.call("oneprot_attn_bwd_dropout" if drop else "oneprot_attn_bwd", st["q"], st["k"], st["v"], self.key_bias, st["ctx"], dctx, st["lse"], self.cos,
                 self.sin, q_scale, dqkv, ws, self.B, H, self.L, hd, *(drop or ()))

    def _lnpool(self, tr, x, pooled, fin, hidden, mode):
        hip.call("oneprot_lnpool_fwd", x, self.ids, tr.config.pad_token_id, *self._final_ln(tr), pooled, *fin, None, hidden, self.B, self.L, tr.d,
                 tr.config.layer_norm_eps, mode)

    def _lnpool_bwd(self, dpooled, wrow, x, lnw, mean, rstd, g, g16, gw, gb, ws, d):
        hip.layernorm_bwd(dpooled, 2, x, lnw, mean, rstd, g, gw, gb, ws, self.T, d, wrow=wrow, L=self.L, dx16=g16)

    def _pool(self, x, pad, pooled, d, mode):
        hip.call("oneprot_pool_fwd", x, self.ids, pad, pooled, self.B, self.L, d, mode)

    def _pool_bwd(self, dpooled, pad, g, g16, d, mode):
        hip.call("oneprot_pool_bwd", dpooled, self.ids, pad, g, g16, self.B, self.L, d, mode)

    def _attnpool(self, hidden, pad, w, b, pooled, attn, d):
        hip.call("oneprot_attnpool_fwd", hidden, self.ids, pad, w, b, pooled, attn, self.B, self.L, d)

    def _attnpool_bwd(self, hidden, attn, w, dpooled, dw, db, dhidden, ws, d):
        hip.call("oneprot_attnpool_bwd", hidden, attn, w, dpooled, dw, db, dhidden, ws, self.B, self.L, d)


class PackedLayout(_Layout):
    packed = True

    def __init__(self, tr, packed):
        self.p = packed
        self.ids, self.cu = packed.ids, packed.cu_seqlens
        self.N, self.B, self.L = len(packed), 1, packed.T_pad
        self.T, self.shape = packed.T_pad, (packed.T_pad,)
        self.work = packed.attn_work()

    def attn_fwd(self, q, k, v, ctx, lse, H, hd, drop=None):
        hip.call("oneprot_attn_varlen_fwd_dropout" if drop else "oneprot_attn_varlen_fwd", q, k, v, self.cu, self.work, self.work.shape[0], ctx, lse, self.N,
                 self.T, H, hd, *(drop or ()))

    def attn_workspace(self, H, dev):
        return torch.empty(hip.query("oneprot_attn_varlen_bwd_workspace", H, self.T), dtype=torch.uint8, device=dev)

    def attn_bwd(self, st, dctx, q_scale, dqkv, ws, H, hd, drop=None):
        hip.call("oneprot_attn_varlen_bwd_dropout" if drop else "oneprot_attn_varlen_bwd", st["q"], st["k"], st["v"], self.cu, self.work, self.work.shape[0],
                 st["ctx"], dctx, st["lse"], self.cos, self.sin, q_scale, dqkv, ws, self.N, self.T, H, hd, *(drop or ()))

    def _lnpool(self, tr, x, pooled, fin, hidden, mode):
        hip.call("oneprot_lnpool_packed_fwd", x, self.ids, self.cu, tr.config.pad_token_id, *self._final_ln(tr), pooled, *fin, hidden, self.N, self.T, tr.d,
                 tr.config.layer_norm_eps, mode)

    def _lnpool_bwd(self, dpooled, wrow, x, lnw, mean, rstd, g, g16, gw, gb, ws, d):
        hip.call("oneprot_lnpool_packed_bwd", dpooled, self.cu, wrow, x, lnw, mean, rstd, g, g16, gw, gb, ws, self.N, self.T, d)

    def _pool(self, x, pad, pooled, d, mode):
        hip.call("oneprot_pool_packed_fwd", x, self.ids, self.cu, pad, pooled, self.N, self.T, d, mode)

    def _pool_bwd(self, dpooled, pad, g, g16, d, mode):
        hip.call("oneprot_pool_packed_bwd", dpooled, self.ids, self.cu, pad, g, g16, self.N, self.T, d, mode)

    def _attnpool(self, hidden, pad, w, b, pooled, attn, d):
        hip.call("oneprot_attnpool_packed_fwd", hidden, self.ids, self.cu, pad, w, b, pooled, attn, self.N, self.p.max_len, d)

    def _attnpool_bwd(self, hidden, attn, w, dpooled, dw, db, dhidden, ws, d):
        hip.call("oneprot_attnpool_packed_bwd", hidden, attn, self.cu, w, dpooled, dw, db, dhidden, ws, self.N, self.T, self.p.max_len, d)
