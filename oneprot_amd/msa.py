"""MSA Transformer tower on the HIP kernels -- what the reference obtains from `esm.pretrained.load_model_and_alphabet_local` in MsaEncoder
(ref msa_encoder.py:18,36): fair-esm's MSATransformer (esm_msa1b_t12_100M_UR50S: 12 axial layers, d 768, 12 heads of 64, FFN 3072, learned positions,
an embedding per MSA row).  Forward only: the reference freezes the tower (msa_encoder.py:30-32), so there is no backward.

PARITY UNPINNED: fair-esm and its checkpoint are not available to this tree.  The arithmetic is restated from the published model and tested against the
fp64 restatement tests/msa_ref.py; neither has been compared with a fair-esm run.  State-dict keys are the published module keys -- those a reference
OneProt checkpoint holds under `network.msa.transformer.` -- and load strictly.

Known differences: masked keys are excluded instead of biased by -10000 (equal wherever a query has one valid key).

TRAIN-MODE DROPOUT, on request.  The reference puts the tower in eval (msa_encoder.py:30) and Lightning's `module.train()` then switches the whole network
back, so every training step of the reference runs the frozen tower with fair-esm's three dropouts active (0.1 each in the published model): `dropout`
after emb_layer_norm_before and on the output of each of a layer's three residual blocks (NormalizedResidualBlock), `attention_dropout` on the
probabilities of the row and the column attention, `activation_dropout` between the FFN's GELU and fc2.  `run_layers(tokens, drop=True)` /
`forward(tokens, drop=True)` reproduce that with masks from our own generators (the distribution of nn.Dropout, not torch's stream): the attention masks
are the per-element hash of the BERT tower's attention dropout (oneprot_msa_row_context_dropout / oneprot_msa_col_attn_dropout; the tied row attention
has one mask element per (b, h, i, j) for all rows), the hidden masks Philox of (seed, call, layer, site, element of the flat [T, d] / [T, f] tensor).
OFF by default: the tower's own `.training` stays False whatever `.train()` is called with, and MsaEncoder asks for `drop` only when it is in train mode
and the switch -- `transformer.train_dropout` (None: follow ONEPROT_MSA_DROPOUT, default 0) -- is on.  The default forward is unchanged bit for bit.

Per layer: LayerNorm -> one QKV GEMM (bf16 [T, 3d]) -> tied row attention (oneprot_msa_row_scores + oneprot_msa_row_context) -> out-projection + residual;
the same with oneprot_msa_col_attn (R = 1: out_proj(v_proj(x)), as published); LayerNorm -> FFN-1 + GELU -> FFN-2 + residual.  The row-attention score
map S [B, H, L, L] fp32 is the one large temporary (its bf16 probabilities and the transposed V of the same MSAs ride along in a workspace): the row
attention runs in groups of whole MSAs so that S stays under ONEPROT_MSA_SCORE_BYTES (default 1 GiB); the grouping is a pure function of (B, R, L, budget) and cannot change a bit of the result (every MSA is computed by its own work-groups).

RAGGED BATCHES.  `run_layers` / `forward` also take an oneprot_amd.packing.PackedMsa -- a stream of MSAs, each a dense R_b x L_b block at its own depth and
length.  The row-wise stages run on the stream's T_pad rows as they are; the embedding and the two attentions use the *_ragged entry
points (one kernel body behind two geometry decoders, csrc/msa.hip); the row scale and the one-row shortcut take R from `padded_shape`, the padded batch the
stream stands for.  At every position of a block the attention calls give the padded batch's bits, dropped probabilities included; the hidden and activation
dropout masks index the stream's own flat [T_pad, d] / [T_pad, f] element: the same distribution as the padded batch's, another draw.  A PackedTokens stream is
refused as before.
"""
import os

import torch

from . import hip
from .arena import ArenaModule, ModelConfig
from .packing import PackedMsa, PackedTokens

MSA_DEFAULTS = dict(model_type="msa_transformer", num_layers=12, embed_dim=768, ffn_embed_dim=3072, attention_heads=12, max_positions=1024,
                    embed_positions_msa=True, msa_rows=1024, vocab_size=33, padding_idx=1, cls_idx=0, eos_idx=2, mask_idx=32, layer_norm_eps=1e-5)
# fair-esm's three dropout probabilities (MSATransformer.add_args; 0.1 each in esm_msa1b_t12_100M_UR50S): used by the train-mode forward only
MSA_DEFAULTS.update(dropout=0.1, attention_dropout=0.1, activation_dropout=0.1)
_ARCH_KEYS = (("layers", "num_layers"), ("embed_dim", "embed_dim"), ("ffn_embed_dim", "ffn_embed_dim"), ("attention_heads", "attention_heads"),
              ("max_positions", "max_positions"), ("embed_positions_msa", "embed_positions_msa"), ("dropout", "dropout"),
              ("attention_dropout", "attention_dropout"), ("activation_dropout", "activation_dropout"))
_BLOCKS = ("row_self_attention", "column_self_attention")


def score_bytes_budget():
    return int(os.environ.get("ONEPROT_MSA_SCORE_BYTES", str(1 << 30)))


def plan_groups(B, R, L, H, budget=None):
    """[(b0, b1), ...]: consecutive groups of whole MSAs whose fp32 score maps [H, L, L] fit `budget` bytes together (one MSA per group when even a single
    map does not).  A pure function of its arguments."""
    budget = score_bytes_budget() if budget is None else int(budget)
    per = 4 * H * L * L
    g = max(1, min(B, budget // per))
    return [(b0, min(b0 + g, B)) for b0 in range(0, B, g)]


def plan_groups_ragged(shapes, H, budget=None):
    """plan_groups for a ragged batch: [(b0, b1), ...] consecutive groups of whole MSAs whose fp32 score maps, sum of 4 * H * L_b^2 bytes, fit `budget`
    together (an MSA whose own map does not is a group by itself).  A pure function of the shapes [(R_b, L_b)], H and the budget; every MSA is computed by
    its own work-groups, so the grouping cannot change a bit."""
    budget = score_bytes_budget() if budget is None else int(budget)
    groups, b0, used = [], 0, 0
    for b, (_, l) in enumerate(shapes):
        per = 4 * H * l * l
        if b > b0 and used + per > budget:
            groups.append((b0, b))
            b0, used = b, 0
        used += per
    groups.append((b0, len(shapes)))
    return groups


class _MsaLayout:
    """How the MSAs of a batch lie in memory, and every launch that depends on it -- the MSA tower's counterpart of layout.py: the key bias and the
    embedding, the row attention's score maps and workspace (groups of whole MSAs under the score budget), the two attentions, the pooling end.
    B MSAs on T rows, Tn of them tokens; R, L: the padded batch's, also for a ragged one (the row scale, the one-row shortcut, the column dropout's
    stride).  drop = (p, seed, stream) selects an attention's dropout form, a false value the plain kernel.  Constructing a layout launches nothing."""

    def embed(self, tr, x):
        """the additive key-padding bias fp32 [T] (kept for the attentions) and x fp32 [T, d] = emb_layer_norm_before(token + position + MSA-row embedding)"""
        cfg, pad = tr.config, tr.config.padding_idx
        self.kb = torch.empty(self.T, device=x.device)
        hip.call("oneprot_key_padding_bias", self.ids, self.kb, self.T, pad)
        name, tables, geom = self._embed_form()
        hip.call(name, self.ids, *tables, tr.view("embed_tokens.weight"), tr.view("embed_positions.weight"), tr.view("msa_position_embedding"),
                 tr.view("emb_layer_norm_before.weight"), tr.view("emb_layer_norm_before.bias"), x, *geom, tr.d, cfg.vocab_size, cfg.max_positions + pad + 1,
                 cfg.msa_rows, pad, cfg.layer_norm_eps)


class _MsaPadded(_MsaLayout):
    """tokens int64 [B, R, L]: T = B * R * L rows, MSA b at rows b * R * L onwards"""

    def __init__(self, tr, tokens):
        self.ids, (self.B, self.R, self.L), self.H, self.hd = tokens.contiguous(), tokens.shape, tr.H, tr.hd
        self.T = self.Tn = self.B * self.R * self.L

    def _embed_form(self):
        return "oneprot_msa_embed_fwd", (), (self.B, self.R, self.L)

    def alloc_scores(self):
        B, R, L, H, dev = self.B, self.R, self.L, self.H, self.ids.device
        self.groups = plan_groups(B, R, L, H)
        gmax = max(b1 - b0 for b0, b1 in self.groups)
        self.S = torch.empty(gmax, H, L, L, device=dev)
        self.ws = torch.empty(hip.query("oneprot_msa_row_context_workspace", gmax, R, L, H), dtype=torch.uint8, device=dev)     # probabilities + V transposed, per group

    def row_attn(self, qkv, ctx, row_scale, drop):
        R, L, H, hd, kb, S, ws = self.R, self.L, self.H, self.hd, self.kb, self.S, self.ws
        for b0, b1 in self.groups:
            t0, t1 = b0 * R * L, b1 * R * L
            hip.call("oneprot_msa_row_scores", qkv[t0:t1], kb[t0:t1], S, b1 - b0, R, L, H, hd, row_scale)
            # b0: the mask is that of the MSA's place in the batch, whatever the grouping
            hip.call("oneprot_msa_row_context" + ("_dropout" if drop else ""), S, qkv[t0:t1], kb[t0:t1], ctx[t0:t1], ws, ws.numel(), b1 - b0, R, L, H, hd,
                     *((b0, *drop) if drop else ()))

    def col_attn(self, qkv, ctx, drop):
        hip.call("oneprot_msa_col_attn" + ("_dropout" if drop else ""), qkv, self.kb, ctx, self.B, self.R, self.L, self.H, self.hd, self.hd ** -0.5, *(drop or ()))

    def pool(self, tr, x, all_rows, mode, want_hidden):
        """(representation n_layers fp32 [B, R, L, d] -- [B, L, d] for row 0, None unless wanted --, pooled [B, d]): final LayerNorm fused with the pooling,
        over every non-pad (r, l) of an MSA (`all_rows`) or over its row 0"""
        B, R, L, d, dev = self.B, self.R, self.L, tr.d, x.device
        if all_rows:                                    # one "sequence" of R * L tokens per MSA
            ids, n = self.ids.view(B, R * L), R * L
        else:
            x, ids, n = x.view(B, R, L, d)[:, 0].contiguous(), self.ids[:, 0].contiguous(), L
        pooled, hidden = torch.empty(B, d, device=dev), (torch.empty(B, n, d, device=dev) if want_hidden else None)
        hip.call("oneprot_lnpool_fwd", x, ids, tr.config.padding_idx, tr.view("emb_layer_norm_after.weight"), tr.view("emb_layer_norm_after.bias"), pooled, None,
                 None, None, None, hidden, B, n, d, tr.config.layer_norm_eps, mode)
        return (hidden.view(B, R, L, d) if (all_rows and want_hidden) else hidden), pooled


class _MsaRagged(_MsaLayout):
    """a PackedMsa: the stream's T_pad rows, MSA b a dense R_b x L_b block at cu_tokens[b]; the *_ragged entry points follow the blocks"""

    def __init__(self, tr, pk):
        self.p, self.ids, self.B, (self.R, self.L), self.H, self.hd = pk, pk.ids, len(pk), pk.padded_shape, tr.H, tr.hd
        self.T, self.Tn = pk.T_pad, pk.n_tokens

    def _embed_form(self):
        self.whole = w = self.p.tables(self.H)[0]       # the whole stream as one call: embedding bounds and the column attention
        return "oneprot_msa_embed_ragged_fwd", (self.p.cu_tokens, self.p.row_lens()), (self.B, self.T, w["max_R"], w["max_L"])

    def alloc_scores(self):
        H, dev = self.H, self.ids.device
        self.groups = self.p.tables(H, plan_groups_ragged(self.p.shapes, H))
        self.S = torch.empty(max(g["s_elems"] for g in self.groups), device=dev)
        self.ws = torch.empty(max(hip.query("oneprot_msa_row_context_ragged_workspace", g["sum_l_lp"], g["sum_r_lp"], H) for g in self.groups), dtype=torch.uint8, device=dev)

    def row_attn(self, qkv, ctx, row_scale, drop):
        H, hd, kb, S, ws = self.H, self.hd, self.kb, self.S, self.ws
        for g in self.groups:
            hip.call("oneprot_msa_row_scores_ragged", qkv, kb, S, g["geo"], g["n"], g["max_L"], H, hd, row_scale)
            hip.call("oneprot_msa_row_context_ragged" + ("_dropout" if drop else ""), S, qkv, kb, ctx, ws, ws.numel(), g["geo"], g["n"], g["max_R"], g["max_L"],
                     g["sum_l_lp"], g["sum_r_lp"], H, hd, self.Tn, self.T, *((g["b_first"], *drop) if drop else ()))

    def col_attn(self, qkv, ctx, drop):                 # one call over the stream; a block of one row inside a deeper batch is the kernel's
        w = self.whole
        hip.call("oneprot_msa_col_attn_ragged" + ("_dropout" if drop else ""), qkv, self.kb, ctx, w["geo"], self.B, w["max_R"], w["max_L"], self.H, self.hd,
                 self.hd ** -0.5, self.Tn, self.T, *((self.L, *drop) if drop else ()))

    def pool(self, tr, x, all_rows, mode, want_hidden):
        """(representation n_layers as a stream fp32 [T_pad, d] -- `PackedMsa.unpack` gives the [R_b, L_b, d] blocks; for row 0 the list of the N [L_b, d]
        row-0 representations; None unless wanted --, pooled [N, d] in MSA order).  Pooling per segment of the stream (oneprot_lnpool_packed_fwd, which walks
        a segment of any length): every MSA's R_b * L_b tokens with cu_tokens as the segment table, or its row 0 gathered into a small stream of its own."""
        pk, N, d, dev, ids, cu, T = self.p, self.B, tr.d, x.device, self.ids, self.p.cu_tokens, self.T
        if not all_rows:
            idx, cu, n0 = pk.row0()
            x, ids, T = x.index_select(0, idx), ids.index_select(0, idx), idx.numel()
        pooled, hidden = torch.empty(N, d, device=dev), (torch.empty(T, d, device=dev) if want_hidden else None)
        hip.call("oneprot_lnpool_packed_fwd", x, ids, cu, tr.config.padding_idx, tr.view("emb_layer_norm_after.weight"), tr.view("emb_layer_norm_after.bias"),
                 pooled, None, None, None, hidden, N, T, d, tr.config.layer_norm_eps, mode)
        if want_hidden and not all_rows:
            hidden = list(hidden[:n0].split([l for _, l in pk.shapes]))
        return hidden, pooled


def upgrade_fair_esm_state_dict(sd):
    """The published key upgrade for this model: the `encoder.` / `sentence_encoder.` prefixes are stripped and `row` and `column` change places in the key
    names (fair-esm's loader does both for msa_transformer checkpoints)."""
    out = {}
    for k, v in sd.items():
        for pre in ("encoder.sentence_encoder.", "sentence_encoder.", "encoder."):
            if k.startswith(pre):
                k = k[len(pre):]
                break
        k = k.replace("row", "\0").replace("column", "row").replace("\0", "column")
        out[k] = v
    return out


def config_from_args(args):
    """architecture from the `args` (argparse.Namespace or dict) / `cfg` entry of a fair-esm checkpoint"""
    if args is not None and not isinstance(args, dict):
        args = getattr(args, "model", args)
        args = args if isinstance(args, dict) else vars(args)
    elif isinstance(args, dict) and isinstance(args.get("model"), (dict,)):
        args = args["model"]
    cfg = dict(MSA_DEFAULTS)
    for src, dst in _ARCH_KEYS:
        if args and args.get(src) is not None:
            cfg[dst] = type(MSA_DEFAULTS[dst])(args[src])
    return ModelConfig(**cfg)


class MsaTransformer(ArenaModule):
    final_layer_norm = True
    accepts_packed = False                # no PackedTokens stream (an ESM / BERT input); its own packed input is the PackedMsa
    max_rows = hip.MSA_MAX_ROWS           # deepest MSA the column-attention kernel takes in one pass

    def __init__(self, config):
        super().__init__()
        self.config = config
        d, f, n, H = config.embed_dim, config.ffn_embed_dim, config.num_layers, config.attention_heads
        self.d, self.f, self.n_layers, self.H = d, f, n, H
        self.hd = d // H
        if self.hd != 64 or d != H * 64:
            raise NotImplementedError(f"head_dim {d / H:g}: the MSA attention kernels are built for head_dim 64 (the published model)")
        if not getattr(config, "embed_positions_msa", True):
            raise NotImplementedError("embed_positions_msa=False: the published esm_msa1b model carries the MSA-row embedding")
        pad = config.padding_idx
        self._init_arena()
        self._add("embed_tokens.weight", (config.vocab_size, d))
        self._add("embed_positions.weight", (config.max_positions + pad + 1, d))
        self._add("msa_position_embedding", (1, config.msa_rows, 1, d))
        for nm in ("emb_layer_norm_before", "emb_layer_norm_after"):
            self._add(nm + ".weight", (d,))
            self._add(nm + ".bias", (d,))
        for i in range(n):
            for blk in _BLOCKS:
                p = f"layers.{i}.{blk}."
                for nm in "qkv":                        # q | k | v adjacent: one [3d, d] GEMM operand
                    self._add(p + f"layer.{nm}_proj.weight", (d, d))
                for nm in "qkv":
                    self._add(p + f"layer.{nm}_proj.bias", (d,))
                self._add(p + "layer.out_proj.weight", (d, d))
                self._add(p + "layer.out_proj.bias", (d,))
                self._add(p + "layer_norm.weight", (d,))
                self._add(p + "layer_norm.bias", (d,))
            p = f"layers.{i}.feed_forward_layer."
            for nm, shp in (("layer.fc1.weight", (f, d)), ("layer.fc1.bias", (f,)), ("layer.fc2.weight", (d, f)), ("layer.fc2.bias", (d,)),
                            ("layer_norm.weight", (d,)), ("layer_norm.bias", (d,))):
                self._add(p + nm, shp)
        V = config.vocab_size                           # heads present in checkpoints, unused by the reference (ref msa_encoder.py:36 reads representations only)
        for k, s in (("lm_head.weight", (V, d)), ("lm_head.bias", (V,)), ("lm_head.dense.weight", (d, d)), ("lm_head.dense.bias", (d,)),
                     ("lm_head.layer_norm.weight", (d,)), ("lm_head.layer_norm.bias", (d,)), ("contact_head.regression.weight", (1, n * H)),
                     ("contact_head.regression.bias", (1,))):
            self._extra[k] = s
        self._finish_arena()
        self.reset_parameters()
        self.capture = None                             # test hook: a list that receives (kind, layer, ctx clone) of every attention output
        self.stages = None                              # second test hook: a list that receives (name, layer, clone): the residual stream on entry to every block ("row" /
                                                        # "col" / "ffn") and after the last layer ("out"), and what each attention read ("row.qkv" / "col.qkv"; R = 1: "col.v")
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def train(self, mode=True):
        """always eval: the tower is frozen, and its train-mode dropout is an argument of the forward (`drop`), not a module mode"""
        return super().train(False)

    # ---- fair-esm's train-mode dropouts, on request (module docstring).  The switch: None follows ONEPROT_MSA_DROPOUT (default 0 = off).
    train_dropout = None

    def dropout_enabled(self):
        """whether MsaEncoder asks for the train-mode dropouts when it is in train mode"""
        if self.train_dropout is not None:
            return bool(self.train_dropout)
        return os.environ.get("ONEPROT_MSA_DROPOUT", "0") != "0"

    def _drop_probs(self):
        cfg = self.config
        return tuple(float(getattr(cfg, k, MSA_DEFAULTS[k])) for k in ("dropout", "attention_dropout", "activation_dropout"))

    def _next_drop_call(self):
        return self._next_call()

    def _drop_stream(self, call, layer, site):
        """stream id of a dropout site.  layer -1, site 0: the embedding dropout; within a layer 0 = row probabilities, 1 = row-block output,
        2 = column probabilities, 3 = column-block output, 4 = FFN activation, 5 = FFN output.  Hidden masks index the flat [T, d] / [T, f] element."""
        return self._rng_stream(self.RNG_DOMAIN_MSA, (call * (self.n_layers + 1) + layer + 1) * 8 + site)

    _norm_weight_suffixes = ("layer_norm.weight", "emb_layer_norm_before.weight", "emb_layer_norm_after.weight")

    @torch.no_grad()
    def reset_parameters(self):
        super().reset_parameters()
        self.view("embed_tokens.weight")[self.config.padding_idx].zero_()

    def layout(self, tokens):
        """the layout of a padded [B, R, L] batch or of a PackedMsa"""
        return (_MsaRagged if isinstance(tokens, PackedMsa) else _MsaPadded)(self, tokens)

    def check_input(self, tokens):
        """every refusal, before anything touches the device"""
        if isinstance(tokens, PackedTokens):
            raise NotImplementedError("MsaEncoder: packed token streams are an ESM-tower input; the MSA tower takes padded [B, R, L] tokens")
        cfg = self.config
        if isinstance(tokens, PackedMsa):               # a ragged batch: the type has refused the kernels' own limits; here the checkpoint's
            if tokens.pad_id != cfg.padding_idx:
                raise ValueError(f"MsaEncoder: the stream was packed with pad id {tokens.pad_id}, the tower's is {cfg.padding_idx}")
            R, L = (max(v) for v in zip(*tokens.shapes))
            if L > cfg.max_positions:
                raise ValueError(f"sequence length {L} exceeds max_positions {min(cfg.max_positions, hip.MSA_MAX_LEN)}")
            if R > cfg.msa_rows:
                raise NotImplementedError(f"MSA depth {R}: the column-attention kernel takes up to {min(self.max_rows, cfg.msa_rows)} rows in one pass")
            if len(tokens) * self.H > 65535:
                raise ValueError(f"{len(tokens)} MSAs in one stream: the attention kernels take up to {65535 // self.H}")
            if not tokens.is_cuda:
                raise hip.HipKernelError("OneProt HIP path needs CUDA(ROCm) tensors; there is no CPU fallback")
            return
        if tokens.dim() != 3:
            raise ValueError(f"MSA tokens must be [B, R, L], got {tuple(tokens.shape)}")
        B, R, L = tokens.shape
        if L > cfg.max_positions or L > hip.MSA_MAX_LEN:
            raise ValueError(f"sequence length {L} exceeds max_positions {min(cfg.max_positions, hip.MSA_MAX_LEN)}")
        if R > self.max_rows or R > cfg.msa_rows:
            raise NotImplementedError(f"MSA depth {R}: the column-attention kernel takes up to {min(self.max_rows, cfg.msa_rows)} rows in one pass")
        if not tokens.is_cuda:
            raise hip.HipKernelError("OneProt HIP path needs CUDA(ROCm) tensors; there is no CPU fallback")

    @torch.no_grad()
    def run_layers(self, tokens, save=False, drop=False):
        """tokens int64 [B, R, L] -> (pre-final-LayerNorm hidden state fp32 [B*R*L, d], None).  drop=True: fair-esm's train-mode forward -- one call id is
        drawn and every dropout site applies its mask (module docstring).
        tokens a PackedMsa -> the same on its stream, fp32 [T_pad, d]: every row-wise stage runs on the T_pad rows as they are, the embedding and the two
        attentions follow the blocks (the *_ragged entry points), R of the row scale and of the one-row shortcut is the padded batch's."""
        self.check_input(tokens)
        if save:
            raise NotImplementedError("the MSA tower is frozen: there is no backward")
        self._refresh_bf16_mirror()
        lay = self.layout(tokens)
        T, R = lay.T, lay.R
        d, f, hd, dev = self.d, self.f, self.hd, lay.ids.device
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        b16 = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
        eps = self.config.layer_norm_eps
        x = f32(T, d)
        lay.embed(self, x)
        if drop:
            call, seed = self._next_drop_call(), self._drop_seed
            p_h, p_a, p_f = self._drop_probs()
            y, u_drop = f32(T, d), b16(T, f)            # a block's output before its dropout; dropout(u) in a buffer of its own (oneprot_dropout_bf16 declares
                                                        # its operands __restrict__ and the header does not allow y = x for it, unlike the fp32 kernels)
            # MSATransformer.forward: emb_layer_norm_before -> dropout_module -> x * (1 - padding_mask); the kernel above has zeroed the padding already
            hip.call("oneprot_dropout_f32", x, x, T * d, p_h, seed, self._drop_stream(call, -1, 0))
        lay.alloc_scores()
        h, qkv, ctx, u = b16(T, d), b16(T, 3 * d), b16(T, d), b16(T, f)
        row_scale = hd ** -0.5 / R ** 0.5               # R = the padded row count, as published
        for i in range(self.n_layers):
            for blk in _BLOCKS:
                p = f"layers.{i}.{blk}."
                if self.stages is not None:
                    self.stages.append((blk[:3], i, x.clone()))
                hip.layernorm_fwd(x, self.view(p + "layer_norm.weight"), self.view(p + "layer_norm.bias"), T, d, eps, y16=h)
                if blk == "column_self_attention" and R == 1:       # one row: softmax over a single key (fair-esm ColumnSelfAttention.forward)
                    hip.gemm_nt(h, self._w16(p + "layer.v_proj.weight"), T, d, d, hip.EPI_BF16, ctx, bias=self.view(p + "layer.v_proj.bias"))
                else:
                    o, n = self.span(p + "layer.q_proj.weight", p + "layer.v_proj.weight")
                    ob, nb = self.span(p + "layer.q_proj.bias", p + "layer.v_proj.bias")
                    hip.gemm_nt(h, self._bf16[o:o + n], T, 3 * d, d, hip.EPI_BF16, qkv, bias=self.flat.data[ob:ob + nb])
                    if blk == "row_self_attention":
                        lay.row_attn(qkv, ctx, row_scale, drop and (p_a, seed, self._drop_stream(call, i, 0)))
                    else:
                        lay.col_attn(qkv, ctx, drop and (p_a, seed, self._drop_stream(call, i, 2)))
                if self.capture is not None:
                    self.capture.append((blk[:3], i, ctx.clone()))
                if self.stages is not None:             # the attention kernels leave qkv as they found it
                    one_row = blk == "column_self_attention" and R == 1
                    self.stages.append((blk[:3] + (".v" if one_row else ".qkv"), i, (ctx if one_row else qkv).clone()))
                if drop:        # NormalizedResidualBlock: x = residual + dropout(layer(layer_norm(x))) -- the add leaves the GEMM epilogue so that the mask sits between
                    hip.gemm_nt(ctx, self._w16(p + "layer.out_proj.weight"), T, d, d, hip.EPI_F32, y, bias=self.view(p + "layer.out_proj.bias"))
                    hip.call("oneprot_dropout_add_f32", y, x, x, T * d, p_h, seed, self._drop_stream(call, i, 1 if blk == "row_self_attention" else 3))
                else:
                    hip.gemm_nt(ctx, self._w16(p + "layer.out_proj.weight"), T, d, d, hip.EPI_BIAS_RESID, x, bias=self.view(p + "layer.out_proj.bias"), aux=x)
            p = f"layers.{i}.feed_forward_layer."
            if self.stages is not None:
                self.stages.append(("ffn", i, x.clone()))
            hip.layernorm_fwd(x, self.view(p + "layer_norm.weight"), self.view(p + "layer_norm.bias"), T, d, eps, y16=h)
            hip.gemm_nt(h, self._w16(p + "layer.fc1.weight"), T, f, d, hip.EPI_BIAS_GELU, u, bias=self.view(p + "layer.fc1.bias"))
            if drop:            # FeedForwardNetwork: fc2(activation_dropout(gelu(fc1(x)))), then the block's own dropout
                hip.call("oneprot_dropout_bf16", u, u_drop, T * f, p_f, seed, self._drop_stream(call, i, 4))
                hip.gemm_nt(u_drop, self._w16(p + "layer.fc2.weight"), T, d, f, hip.EPI_F32, y, bias=self.view(p + "layer.fc2.bias"))
                hip.call("oneprot_dropout_add_f32", y, x, x, T * d, p_h, seed, self._drop_stream(call, i, 5))
            else:
                hip.gemm_nt(u, self._w16(p + "layer.fc2.weight"), T, d, f, hip.EPI_BIAS_RESID, x, bias=self.view(p + "layer.fc2.bias"), aux=x)
        if self.stages is not None:
            self.stages.append(("out", self.n_layers, x.clone()))
        return x, None

    @torch.no_grad()
    def forward(self, tokens, repr_layers=(), drop=False, **_):
        """MSATransformer-compatible call: {"representations": {n_layers: [B, R, L, d]}} (the last representation, after emb_layer_norm_after);
        drop=True: with fair-esm's train-mode dropouts (run_layers)"""
        x, _ = self.run_layers(tokens, drop=drop)
        y = torch.empty_like(x)
        hip.layernorm_fwd(x, self.view("emb_layer_norm_after.weight"), self.view("emb_layer_norm_after.bias"), x.shape[0], self.d, self.config.layer_norm_eps, y32=y)
        if isinstance(tokens, PackedMsa):               # the representation as the stream [T_pad, d] (PackedMsa.unpack gives the blocks)
            return {"representations": {self.n_layers: y}}
        B, R, L = tokens.shape
        return {"representations": {self.n_layers: y.view(B, R, L, self.d)}}

    @classmethod
    def from_pretrained(cls, model_name_or_path, **_):
        """`model_name_or_path`: a raw fair-esm checkpoint file, {"args" | "cfg": ..., "model": state dict} (what the reference hands to
        esm.pretrained.load_model_and_alphabet_local, msa_encoder.py:18).  PARITY UNPINNED: the key upgrade and the architecture fields follow the published
        loader, not a run of it."""
        path, cfg, sd = str(model_name_or_path), ModelConfig(**MSA_DEFAULTS), None
        if os.path.isfile(path):
            ck = torch.load(path, map_location="cpu", weights_only=False)
            cfg = config_from_args(ck.get("cfg") if ck.get("cfg") is not None else ck.get("args"))
            sd = upgrade_fair_esm_state_dict(ck["model"])
            for k in ("embed_tokens.weight", "msa_position_embedding"):
                if k in sd:
                    setattr(cfg, "vocab_size" if k == "embed_tokens.weight" else "msa_rows", sd[k].shape[0 if k == "embed_tokens.weight" else 1])
        model, missing, unexpected = cls._from_checkpoint(sd, model_name_or_path, "a fair-esm .pt file", ("lm_head.", "contact_head.", "extra."), cfg)
        unexpected = [u for u in unexpected if not u.endswith("_float_tensor")]
        if missing or unexpected:
            raise OSError(f"checkpoint {model_name_or_path}: missing {missing[:5]}, unexpected {unexpected[:5]}")
        return model
