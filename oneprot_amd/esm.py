"""ESM-2 encoder ("transformer" member of the Sequence / StructToken encoders) running on the HIP kernels.

Replaces, for the OneProt hot path, what the reference gets from HF `AutoModel.from_pretrained(...)`
(ref sequence_encoder.py:8-19,51-55; struct_token_encoder.py:26-27) -- i.e. transformers' EsmModel
(modeling_esm.py:198-760).  State-dict key names are identical to EsmModel's, so OneProt / HF checkpoints load.

Memory layout: the parameters live in the fp32 arena of arena.py (q,k,v weights adjacent => one fused [3d,d] QKV operand), the
adapters are lora.py's; the gradient w.r.t. the arena is produced as one flat fp32 tensor by the hand-written backward below, so clip-norm and Adam
are single launches over contiguous memory.
"""
import json
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import hip
from . import layout
from .arena import ArenaModule, ModelConfig, load_weight_file, _Out      # noqa: F401  (re-exported: the names this module used to define)
from .lora import LoraArena

KNOWN_ESM = {   # public facts of the ESM-2 checkpoints (SURVEY.md section 8 header)
    "esm2_t6_8M_UR50D": dict(num_hidden_layers=6, hidden_size=320, intermediate_size=1280),
    "esm2_t12_35M_UR50D": dict(num_hidden_layers=12, hidden_size=480, intermediate_size=1920),
    "esm2_t30_150M_UR50D": dict(num_hidden_layers=30, hidden_size=640, intermediate_size=2560),
    "esm2_t33_650M_UR50D": dict(num_hidden_layers=33, hidden_size=1280, intermediate_size=5120),
}
ESM_DEFAULTS = dict(model_type="esm", vocab_size=33, pad_token_id=1, mask_token_id=32, num_attention_heads=20, layer_norm_eps=1e-5,
                    token_dropout=True, position_embedding_type="rotary", emb_layer_norm_before=False, max_position_embeddings=1026,
                    initializer_range=0.02, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def resolve_config(model_name_or_path, defaults_by_type=None):
    """Local directory with config.json, or a known hub id (no network in this environment).
    Mirrors the failure mode of AutoConfig.from_pretrained: OSError when it cannot be resolved."""
    path = str(model_name_or_path)
    cfg_file = os.path.join(path, "config.json")
    if os.path.isfile(cfg_file):
        with open(cfg_file) as f:
            raw = json.load(f)
        base = dict(ESM_DEFAULTS) if raw.get("model_type", "esm") == "esm" else {}
        base.update(raw)
        return ModelConfig(**base), path
    short = path.split("/")[-1]
    if short in KNOWN_ESM:
        base = dict(ESM_DEFAULTS)
        base.update(KNOWN_ESM[short])
        return ModelConfig(**base), None
    raise OSError(f"{model_name_or_path} is not a local folder with a config.json and is not a known ESM-2 model identifier")


# experiment hook: ONEPROT_GELU_CODE_DROP_BITS=n rounds the saved one-byte gelu'(z) codes to 8 - n bits (n = 1: twice the quantisation step).  Used by
# tests/test_baseline_shapes_gpu.py to attribute the backward's deviation from the fp32 oracle; 0 (default) leaves the codes alone.
_GELU_CODE_DROP_BITS = int(os.environ.get("ONEPROT_GELU_CODE_DROP_BITS", "0"))


class _EsmPadded(layout.PaddedLayout):
    """The ESM stages of a padded [B, L] batch: embedding (token-dropout factor per row) and rotary tables (positions 0..L-1, the GEMM epilogue reads
    row % L).  Everything but these, attention and the pooling end (layout.py) runs row-wise on the B*L rows."""

    def embed(self, tr, x):
        cfg = tr.config
        self.cos, self.sin = tr._rope(self.L)
        self.make_key_bias(cfg.pad_token_id)
        self.row_scale = torch.empty(self.B, device=x.device)
        hip.call("oneprot_esm_embed_fwd", self.ids, tr.view("embeddings.word_embeddings.weight"), x, self.row_scale, self.B, self.L, tr.d, cfg.vocab_size,
                 cfg.pad_token_id, cfg.mask_token_id, 1 if cfg.token_dropout else 0)

    def embed_bwd(self, tr, g, dtable):
        cfg, V = tr.config, tr.config.vocab_size
        ws = torch.empty(hip.query("oneprot_esm_embed_bwd_workspace", self.T, tr.d, V), dtype=torch.uint8, device=g.device)
        hip.call("oneprot_esm_embed_bwd", self.ids, g, self.row_scale, dtable, ws, self.B, self.L, tr.d, V, cfg.pad_token_id, cfg.mask_token_id,
                 1 if cfg.token_dropout else 0, 0)


class _EsmPacked(layout.PackedLayout):
    """The same on a packed token stream: q / k / v come out of the QKV GEMM as [H, T_pad, hd], its rotary epilogue reads row t of per-token tables; the
    embedding counts the token-dropout factor per segment and gathers those tables."""

    def embed(self, tr, x):
        cfg, dev = tr.config, x.device
        cos_t, sin_t = tr._rope(tr.MAX_POSITIONS)
        half = cos_t.shape[1]
        self.tok_scale = torch.empty(self.T, device=dev)
        self.cos, self.sin = torch.empty(self.T, half, device=dev), torch.empty(self.T, half, device=dev)
        hip.call("oneprot_esm_embed_packed_fwd", self.ids, self.cu, tr.view("embeddings.word_embeddings.weight"), cos_t, sin_t, x, self.tok_scale, self.cos, self.sin,
                 self.N, self.T, self.p.max_len, tr.d, cfg.vocab_size, half, cos_t.shape[0], cfg.pad_token_id, cfg.mask_token_id, 1 if cfg.token_dropout else 0)

    def embed_bwd(self, tr, g, dtable):
        cfg, V = tr.config, tr.config.vocab_size
        ws = torch.empty(hip.query("oneprot_esm_embed_bwd_workspace", self.T, tr.d, V), dtype=torch.uint8, device=g.device)
        hip.call("oneprot_esm_embed_packed_bwd", self.ids, g, self.tok_scale, dtable, ws, self.T, tr.d, V, cfg.pad_token_id, cfg.mask_token_id,
                 1 if cfg.token_dropout else 0, 0)


def _check_recompute_k(k):
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError(f"recompute_layers must be a non-negative int (0 = off), got {k!r}")
    return k


def recompute_plan(n_layers, k):
    """Layer segments [0,k), [k,2k), ... of a tower of n_layers (the last one may be short; k >= n_layers: one segment) as a list of (lo, hi), or None
    when k = 0 (recomputation off).  The forward keeps the activations of the top segment only and a boundary record per lower segment."""
    _check_recompute_k(k)
    if isinstance(n_layers, bool) or not isinstance(n_layers, int) or n_layers < 1:
        raise ValueError(f"n_layers must be a positive int, got {n_layers!r}")
    if k == 0:
        return None
    return [(lo, min(lo + k, n_layers)) for lo in range(0, n_layers, k)]


class EsmTransformer(LoraArena):
    """EsmModel replacement.  `add_pooling_layer` only controls whether the (unused) HF pooler parameters exist,
    as in the reference (SequenceEncoder: False, StructTokenEncoder: True)."""
    layouts = (_EsmPadded, _EsmPacked)      # layout.of(self, ids)

    def __init__(self, config, add_pooling_layer=True):
        super().__init__()
        if getattr(config, "position_embedding_type", "rotary") != "rotary" or getattr(config, "emb_layer_norm_before", False):
            raise NotImplementedError("only rotary ESM-2 configurations are on the OneProt hot path")
        self.config = config
        d, f, n, V = config.hidden_size, config.intermediate_size, config.num_hidden_layers, config.vocab_size
        self.d, self.f, self.n_layers, self.H = d, f, n, config.num_attention_heads
        self.hd = d // self.H
        # The attention / RoPE kernels are built for head_dim 16/32/64.  Any other even head_dim <= 64 (ESM-2-35M: 24) runs on the
        # next larger one: each head's two RoPE halves are placed at the start of the two halves of a zero-padded head
        # (`_head_pad_maps`), in the bf16 GEMM operands only -- parameters, gradients and checkpoints keep the HF shapes.
        self.hdp = next((c for c in (16, 32, 64) if c >= self.hd), None)
        if self.hdp is None or self.hd % 2 or self.hd * self.H != d or d % 8 or (self.H * self.hdp) % 64:
            raise NotImplementedError(f"head_dim {self.hd} x {self.H} heads (hidden {d}): kernels need an even head_dim <= 64 and heads*padded_head_dim % 64 == 0")
        self.dp = self.H * self.hdp
        self._padded = self.hdp != self.hd
        self._init_arena()
        self._add("embeddings.word_embeddings.weight", (V, d))
        for i in range(n):
            p = f"encoder.layer.{i}."
            for nm in ("query", "key", "value"):
                self._add(p + f"attention.self.{nm}.weight", (d, d))
            for nm in ("query", "key", "value"):
                self._add(p + f"attention.self.{nm}.bias", (d,))
            self._add(p + "attention.output.dense.weight", (d, d))
            self._add(p + "attention.output.dense.bias", (d,))
            self._add(p + "attention.LayerNorm.weight", (d,))
            self._add(p + "attention.LayerNorm.bias", (d,))
            self._add(p + "intermediate.dense.weight", (f, d))
            self._add(p + "intermediate.dense.bias", (f,))
            self._add(p + "output.dense.weight", (d, f))
            self._add(p + "output.dense.bias", (d,))
            self._add(p + "LayerNorm.weight", (d,))
            self._add(p + "LayerNorm.bias", (d,))
        self._add("encoder.emb_layer_norm_after.weight", (d,))
        self._add("encoder.emb_layer_norm_after.bias", (d,))
        # parameters HF carries but the hot path never touches (kept for strict state-dict compatibility)
        if add_pooling_layer:
            self._extra["pooler.dense.weight"] = (d, d)
            self._extra["pooler.dense.bias"] = (d,)
        self._extra["contact_head.regression.weight"] = (1, n * self.H)
        self._extra["contact_head.regression.bias"] = (1,)
        self._finish_arena()
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, self.hd, 2, dtype=torch.float32) / self.hd))
        self.register_buffer("inv_freq", inv_freq, persistent=False)
        self._rope_cache = {}
        self._pad_ops = {}
        self._wo_packed = {}
        self.reset_parameters()

    _norm_weight_suffixes = ("LayerNorm.weight", "layer_norm_after.weight")

    @torch.no_grad()
    def reset_parameters(self):
        std = super().reset_parameters()
        pad = self.config.pad_token_id
        if pad is not None:
            self.view("embeddings.word_embeddings.weight")[pad].zero_()
        for k, p in self.extra.items():
            if p.dim() > 1:
                p.normal_(0.0, std)

    _sd_extra_buffers = (("rotary_embeddings.inv_freq", lambda self: self.inv_freq.detach().clone()),)
    # rotary buffers: model-level (transformers >= 5) or per-layer (4.33) keys are accepted, values recomputed;
    # hub checkpoints also carry an unused absolute position table that HF ignores as well
    _load_ignore_suffixes = ("rotary_embeddings.inv_freq", "embeddings.position_embeddings.weight", "embeddings.position_ids")

    def resize_token_embeddings(self, new_vocab):
        """ref struct_token_encoder.py:27: append rows (normal(0, initializer_range), as transformers 4.33 did)."""
        old = self.config.vocab_size
        if new_vocab == old:
            return
        old_views = {k: v.clone() for k, v in self.named_views().items()}
        old_spec = self._spec
        self.config.vocab_size = new_vocab
        self._spec, self._cursor = OrderedDict(), 0
        for name, (_, _, shape) in old_spec.items():
            self._add(name, (new_vocab, self.d) if name == "embeddings.word_embeddings.weight" else shape)
        self._total = self._cursor
        req = self.flat.requires_grad
        self.flat = nn.Parameter(torch.zeros(self._total, device=self.flat.device), requires_grad=req)
        with torch.no_grad():
            for name, v in old_views.items():
                dst = self.view(name)
                if name == "embeddings.word_embeddings.weight":
                    dst[:old] = v[:old]
                    dst[old:].normal_(0.0, getattr(self.config, "initializer_range", 0.02))
                else:
                    dst.copy_(v)
        self._bf16_version = None

    def get_input_embeddings_weight(self):
        return self.view("embeddings.word_embeddings.weight")

    # ----------------------------------------------------------------------------------------- device-side caches
    def _refresh_bf16(self):
        if not self._refresh_bf16_mirror():
            return
        dev = self.flat.device
        if self._padded:
            self._refresh_padded_heads()
        # out-projection weights packed for the full-row GEMM that also applies the following LayerNorm (csrc/gemm_nt_ln.hip; d = 640 only)
        if self._fused_ln_ok():
            for i in range(self.n_layers):
                t = self._wo_packed.get(i)
                if t is None or t.device != dev:
                    t = self._wo_packed[i] = torch.empty(self.d * self.dp, dtype=torch.bfloat16, device=dev)
                hip.call("oneprot_gemm_ln_pack_weight", self._w16(f"encoder.layer.{i}.attention.output.dense.weight"), t, self.d, self.dp)
        if self.flat.requires_grad:
            d, f = self.d, self.f
            self._transpose_layer_weights("w1", "encoder.layer.{i}.intermediate.dense.weight", f, d)
            self._transpose_layer_weights("w2", "encoder.layer.{i}.output.dense.weight", d, f)
            if not self._padded:
                self._transpose_layer_weights("o", "encoder.layer.{i}.attention.output.dense.weight", d, d)
                self._transpose_qkv_weights()

    def _fused_ln_ok(self):
        """the full-row GEMM + LayerNorm kernel is built for 640-wide rows with un-padded heads (ESM-2-150M); ONEPROT_FUSED_LN=0 keeps the pair (A/B runs)"""
        return self.d == 640 and not self._padded and os.environ.get("ONEPROT_FUSED_LN", "1") != "0"

    def _head_pad_maps(self):
        """(rowmap [3d], colmap [d]): position of HF row s*d + h*hd + j of the fused QKV weight inside the padded [3*dp] layout, and of
        context column h*hd + j inside [dp].  j < hd/2 -> j ; j >= hd/2 -> hdp/2 + (j - hd/2): the RoPE partner of padded column c is
        c +- hdp/2, as the hd=hdp kernels assume."""
        dev = self.flat.device
        if self._pad_ops.get("maps_dev") != dev:
            half, hhp = self.hd // 2, self.hdp // 2
            j = torch.arange(self.hd)
            within = torch.where(j < half, j, hhp + j - half)
            col = (torch.arange(self.H)[:, None] * self.hdp + within[None, :]).reshape(-1)
            row = (torch.arange(3)[:, None] * self.dp + col[None, :]).reshape(-1)
            self._pad_ops["maps"] = (row.to(dev), col.to(dev))
            self._pad_ops["maps_dev"] = dev
        return self._pad_ops["maps"]

    def _refresh_padded_heads(self):
        """bf16 QKV / out-proj operands (and their transposes for the dgrad GEMMs) in the padded-head layout; a layout permutation
        of the bf16 mirror, redone whenever the mirror is."""
        d, dp, dev = self.d, self.dp, self.flat.device
        rowmap, colmap = self._head_pad_maps()
        for i in range(self.n_layers):
            p = f"encoder.layer.{i}."
            (o, n), (ob, nb) = self._qkv_spans(i)
            ops = self._pad_ops.get(i)
            if ops is None or ops["qkv"].device != dev:
                ops = dict(qkv=torch.zeros(3 * dp, d, dtype=torch.bfloat16, device=dev), bqkv=torch.zeros(3 * dp, device=dev),
                           o=torch.zeros(d, dp, dtype=torch.bfloat16, device=dev))
                self._pad_ops[i] = ops
            ops["qkv"][rowmap] = self._bf16[o:o + n].view(3 * d, d)
            ops["bqkv"][rowmap] = self.flat.data[ob:ob + nb]
            ops["o"][:, colmap] = self._w16(p + "attention.output.dense.weight")
            if self.flat.requires_grad:
                self._bf16_T[(i, "qkv")] = ops["qkv"].t().contiguous()       # [d, 3dp]
                self._bf16_T[(i, "o")] = ops["o"].t().contiguous()           # [dp, d]

    def _qkv_operands(self, i):
        """(W_qkv bf16 [3*dp, d], bias fp32 [3*dp], W_o bf16 [d, dp]) for layer i"""
        if self._padded:
            ops = self._pad_ops[i]
            return ops["qkv"], ops["bqkv"], ops["o"]
        (o, n), (ob, nb) = self._qkv_spans(i)
        return self._bf16[o:o + n], self.flat.data[ob:ob + nb], self._w16(f"encoder.layer.{i}.attention.output.dense.weight")

    MAX_POSITIONS = 1026      # rows of the rotary tables a packed batch gathers from (ESM-2's max_position_embeddings; PackedTokens enforces it)

    def _rope(self, L):
        key = (L, self.flat.device)
        if key not in self._rope_cache:
            t = torch.arange(L, dtype=torch.float32)
            freqs = torch.outer(t, self.inv_freq.detach().float().cpu())      # hf modeling_esm.py:150-158 (positions = arange(L))
            cos, sin = freqs.cos(), freqs.sin()
            if self._padded:      # padded dims hold zeros; rotate them by angle 0
                extra = self.hdp // 2 - self.hd // 2
                cos = torch.cat([cos, torch.ones(L, extra)], 1)
                sin = torch.cat([sin, torch.zeros(L, extra)], 1)
            self._rope_cache[key] = (cos.contiguous().to(self.flat.device), sin.contiguous().to(self.flat.device))
        return self._rope_cache[key]

    # ----------------------------------------------------------------------------------------- forward / backward
    # Activation recomputation by layer segments (DESIGN.md sections 3 and 6): None = read ONEPROT_RECOMPUTE_LAYERS at call time, else 0 (off).  An int k > 0
    # keeps, of a training forward, only the top segment's activations and one boundary record per lower segment of k layers; the backward re-runs each
    # lower segment from its record with the forward's own launches before it walks it.  Not part of the state dict.
    recompute_layers = None

    def _recompute_k(self):
        k = self.recompute_layers
        if k is None:
            raw = os.environ.get("ONEPROT_RECOMPUTE_LAYERS", "").strip()
            try:
                k = int(raw) if raw else 0
            except ValueError:
                raise ValueError(f"ONEPROT_RECOMPUTE_LAYERS must be a non-negative integer, got {raw!r}") from None
        return _check_recompute_k(k)

    def run_layers(self, ids, save):
        """Embedding + n layers on padded ids [B, L] or a PackedTokens stream (B = 1, L = T_pad for every row-wise stage).
        Returns (x_final fp32 [T,d], saved-dict or None)."""
        if not ids.is_cuda:
            raise hip.HipKernelError("OneProt HIP path needs CUDA(ROCm) tensors; there is no CPU fallback")
        self._refresh_bf16()
        lay = layout.of(self, ids)
        B, L, T = lay.B, lay.L, lay.T
        d, f, dp, n = self.d, self.f, self.dp, self.n_layers
        x = torch.empty(T, d, dtype=torch.float32, device=ids.device)
        lay.embed(self, x)
        # segments of a recomputing forward: only where activations are kept to begin with (a training forward that needs the tower's gradient) and only
        # when there is a segment below the top one
        plan = recompute_plan(n, self._recompute_k()) if (save and self.training) else None
        if plan is not None and len(plan) < 2:
            plan = None
        fused_ln = self._fused_ln_ok() and T % 128 == 0
        # FFN-2 + residual AND the next layer's first LayerNorm in one launch of the 8-phase GEMM (row statistics completed across the work-groups of a row
        # panel: oneprot_gemm_bf16_nt_resid_ln8); ONEPROT_FFN2_LN=0 keeps the pair (A/B runs)
        ln8_mode = os.environ.get("ONEPROT_FFN2_LN", "1")    # "0": never; "force": whenever the shape is served (tests: small batches against the oracle); else when it pays
        if plan is not None and getattr(self, "_grad_overlap", None) is not None:
            # the recompute pass runs inside the backward, beside the all-reduce channels of GradOverlap: kernels whose work-groups wait for each other are
            # not co-resident with anything, so BOTH passes of such an application take the wait-free pair (bit identity needs the same forms twice)
            ln8_mode = "0"
        ln8_min = 0 if ln8_mode == "0" else (1 if ln8_mode == "force" else 2)
        ffn2_ln = ln8_min > 0 and not self._padded and hip.query("oneprot_gemm_resid_ln8_eligible", T, d, f) >= ln8_min
        outproj_ln8 = not fused_ln and ln8_min > 0 and not self._padded and hip.query("oneprot_gemm_resid_ln8_eligible", T, d, dp) >= ln8_min
        # decided once per application: a recompute pass reads the forms (and the LoRA call id) back from `saved`, never from the environment
        run = dict(layout=lay, forms=dict(fused_ln=fused_ln, ffn2_ln=ffn2_ln, outproj_ln8=outproj_ln8), lora_call=self._lora_next_call(), bufs=None)
        saved = dict(layout=lay, layers=[None] * n, B=B, L=L, forms=run["forms"]) if save else None
        if save and run["lora_call"] is not None:
            saved["lora_call"] = run["lora_call"]
        if plan is None:
            x, _ = self._run_range(run, x, None, 0, n, save, saved["layers"] if save else None)
        else:
            bounds = saved["bounds"] = {}
            pre = None
            for lo, hi in plan[:-1]:      # the frozen tower's shared buffers; the layer under a boundary writes the boundary's x_in (and h1 | stats) into buffers of their own
                bounds[lo] = dict(x_in=x, h1=pre[0] if pre is not None else None, stats=pre[1] if pre is not None else None)
                x, pre = self._run_range(run, x, pre, lo, hi, False, None, boundary=True)
            saved["plan"] = plan
            lo, hi = plan[-1]
            x, _ = self._run_range(run, x, pre, lo, hi, True, saved["layers"])
        if save:
            saved["x_final"] = x
        return x, saved

    def _run_range(self, run, x, pre, lo, hi, save, layers, boundary=False):
        """Layers lo..hi-1 on the residual stream x fp32 [T,d]: THE layer body -- the plain forward, the first forward of a recomputing tower and its
        recompute pass all come through here.  pre: (h1, stats [2,T] or None) of layer lo when the launch below it already wrote them, else None.
        save: every layer keeps its record in layers[i] and writes x_mid / x_out out of place; otherwise the layers share one set of buffers and update
        the stream in place.  boundary (not saving): a segment of a recomputing forward -- x and pre belong to a boundary record, so layer lo leaves them
        alone (its x_mid goes to a work buffer), layer hi-1 writes x_out (and the next layer's h1 | stats) into fresh buffers, which become the next
        record, and FFN-1 runs in the two-output form the recompute pass will take (see below).
        Returns (x_out of layer hi-1, pre of layer hi)."""
        cfg, lay, forms, lora_call = self.config, run["layout"], run["forms"], run["lora_call"]
        B, L, T = lay.B, lay.L, lay.T
        d, f, H, hd, dp = self.d, self.f, self.H, self.hdp, self.dp        # hd: kernel (padded) head dim
        q_scale = self.hd ** -0.5
        dev = x.device
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        b16 = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
        eps = cfg.layer_norm_eps
        fused_ln, ffn2_ln, outproj_ln8 = forms["fused_ln"], forms["ffn2_ln"], forms["outproj_ln8"]
        # (pointer, bytes): partial row statistics + work queues; asked for per pass (another tower may have grown the workspace since the forward)
        sched_ws = hip.sched_workspace(T) if (ffn2_ln or outproj_ln8 or hip.dynamic_tiles_wanted()) else None
        if not save:
            if run["bufs"] is None:
                run["bufs"] = dict(h=b16(T, d), q=b16(B, H, L, hd), k=b16(B, H, L, hd), v=b16(B, H, L, hd), ctx=b16(T, dp), u=b16(T, f))
            bufs = run["bufs"]
            h, q, k, v, ctx_, u = bufs["h"], bufs["q"], bufs["k"], bufs["v"], bufs["ctx"], bufs["u"]
        for i in range(lo, hi):
            p = f"encoder.layer.{i}."
            if save:
                stats1 = pre[1] if pre is not None else f32(2, T)      # mean | rstd of the first LayerNorm
                st = dict(x_in=x, mean1=stats1[0], rstd1=stats1[1], mean2=f32(T), rstd2=f32(T), h1=pre[0] if pre is not None else b16(T, d), q=b16(B, H, L, hd),
                          k=b16(B, H, L, hd), v=b16(B, H, L, hd), ctx=b16(T, dp), lse=f32(B, H, L), h2=b16(T, d), z=torch.empty(T, f, dtype=torch.uint8, device=dev),
                          u=b16(T, f))
                h1, q, k, v, ctx_, h2, u, z = st["h1"], st["q"], st["k"], st["v"], st["ctx"], st["h2"], st["u"], st["z"]
                m1, r1, m2, r2, lse = st["mean1"], st["rstd1"], st["mean2"], st["rstd2"], st["lse"]
            else:
                h1 = pre[0] if pre is not None else h
                h2 = h
                z = m1 = r1 = m2 = r2 = lse = None
                if boundary:
                    # FFN-1 without a second output is another kernel (forward-only GELU: a polynomial of its own, csrc/gemm_epi.h); the recompute pass will run
                    # the two-output form, and the residual stream above this segment must be the one IT produces, bit for bit -- so the first forward runs
                    # that form too, its one-byte codes going to a scratch buffer.  Every other launch only leaves optional stores out.
                    if "z" not in bufs:
                        bufs["z"] = torch.empty(T, f, dtype=torch.uint8, device=dev)
                    z = bufs["z"]
            if pre is None:
                hip.layernorm_fwd(x, self.view(p + "attention.LayerNorm.weight"), self.view(p + "attention.LayerNorm.bias"), T, d, eps, y16=h1, mean=m1, rstd=r1)
            w_qkv, b_qkv, w_o = self._qkv_operands(i)
            lora_u = self._qkv_forward(i, h1, w_qkv, b_qkv, T, 3 * dp, (lay.cos, lay.sin, L, H, hd), q_scale * hip.LOG2E, q, k, v, lora_call)
            if save:
                st["lora_u"] = lora_u
            lay.attn_fwd(q, k, v, ctx_, lse, H, hd)
            if save:
                x_mid = f32(T, d)
            elif boundary and i == lo:      # x is a boundary record's x_in: the stream moves to a work buffer here and is updated in place from then on
                if "xw" not in bufs:
                    bufs["xw"] = f32(T, d)
                x_mid = bufs["xw"]
            else:
                x_mid = x
            if fused_ln:
                # out-projection + bias + residual AND the FFN's pre-LayerNorm in one full-row kernel: x_mid is not read back by a LayerNorm launch
                # (measured on cfg-2: 0.28-0.29 ms against 0.31-0.32 ms for the pair; the FFN-2 / next-layer pair goes through the 8-phase GEMM with the
                # statistics finished across work-groups instead, below -- this full-row form ties with the pair there, NOTEBOOK.md section 6c)
                hip.call("oneprot_gemm_bf16_nt_resid_ln", ctx_, self._wo_packed[i], T, d, dp, dp, self.view(p + "attention.output.dense.bias"), x, x_mid,
                         self.view(p + "LayerNorm.weight"), self.view(p + "LayerNorm.bias"), eps, h2, m2, r2)
            elif outproj_ln8:
                # wider rows (ESM-2-650M, d = 1280): the same pair through the 8-phase GEMM with the statistics finished across its four column tiles
                stats2 = f32(2, T) if save else None
                hip.call("oneprot_gemm_bf16_nt_resid_ln8", ctx_, w_o, T, d, dp, dp, dp, self.view(p + "attention.output.dense.bias"), x, x_mid,
                         self.view(p + "LayerNorm.weight"), self.view(p + "LayerNorm.bias"), eps, h2, stats2, *sched_ws)
                if save:
                    st["mean2"], st["rstd2"] = stats2[0], stats2[1]
            else:
                hip.gemm_nt(ctx_, w_o, T, d, dp, hip.EPI_BIAS_RESID, x_mid, bias=self.view(p + "attention.output.dense.bias"), aux=x)
                hip.layernorm_fwd(x_mid, self.view(p + "LayerNorm.weight"), self.view(p + "LayerNorm.bias"), T, d, eps, y16=h2, mean=m2, rstd=r2)
            hip.gemm_nt(h2, self._w16(p + "intermediate.dense.weight"), T, f, d, hip.EPI_BIAS_GELU, u, bias=self.view(p + "intermediate.dense.bias"), out1=z)
            if save and _GELU_CODE_DROP_BITS:      # experiment hook (tests: what the one-byte gelu' codes cost the gradient): keep only the top 8 - n bits
                nb = _GELU_CODE_DROP_BITS
                z.add_(1 << (nb - 1)).bitwise_and_(0xFF & ~((1 << nb) - 1))
            fresh = save or (boundary and i == hi - 1)      # this layer's outputs outlive the shared buffers
            x_out = f32(T, d) if fresh else x_mid
            if ffn2_ln and i + 1 < self.n_layers:
                pn = f"encoder.layer.{i + 1}.attention.LayerNorm."
                pre = (b16(T, d), f32(2, T)) if fresh else (h, None)
                hip.call("oneprot_gemm_bf16_nt_resid_ln8", u, self._w16(p + "output.dense.weight"), T, d, f, f, f, self.view(p + "output.dense.bias"), x_mid, x_out,
                         self.view(pn + "weight"), self.view(pn + "bias"), eps, pre[0], pre[1], *sched_ws)
            else:
                pre = None
                hip.gemm_nt(u, self._w16(p + "output.dense.weight"), T, d, f, hip.EPI_BIAS_RESID, x_out, bias=self.view(p + "output.dense.bias"), aux=x_mid)
            if save:
                st["x_mid"] = x_mid
                layers[i] = st
            x = x_out
        return x, pre

    def _recompute_segment(self, saved, lo, hi):
        """the activations of layers lo..hi-1 again, from the segment's boundary record, by the forward's own launches in the saving form; nothing a
        forward call advances moves (the LoRA call id and the kernel forms come from `saved`, the bf16 operands are the step's)"""
        b = saved["bounds"][lo]
        run = dict(layout=saved["layout"], forms=saved["forms"], lora_call=saved.get("lora_call"), bufs=None)
        self._run_range(run, b["x_in"], (b["h1"], b["stats"]) if b["h1"] is not None else None, lo, hi, True, saved["layers"])

    GRAD_CHUNK_LAYERS = 6      # arena-gradient ranges are handed to `on_ready` every this many layers (overlapped all-reduce)

    def backward_layers(self, saved, g, g16, gflat, on_ready=None):
        """g: fp32 [T,d] gradient w.r.t. the last layer's output (consumed in place), g16: its bf16 copy;
        gflat: fp32 arena gradient (written).  on_ready(lo, hi): called as soon as the arena-gradient range [lo, hi) is final
        (the arena is laid out embeddings | layer 0 .. n-1 | final LayerNorm, and the backward walks the layers downwards), so the
        data-parallel all-reduce of the upper layers runs under the backward of the lower ones."""
        lay = saved["layout"]
        T, d, f, H, hd, dp = lay.T, self.d, self.f, self.H, self.hdp, self.dp
        q_scale = self.hd ** -0.5
        dev = g.device
        gv = lambda name: self.view(name, gflat)
        b16 = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
        ws_ln = torch.empty(hip.query("oneprot_layernorm_bwd_workspace", d), dtype=torch.uint8, device=dev)
        lora_raw, lora_tn = self._lora_backward_setup(saved, dev)
        ws_tn = self._tn_workspace(((3 * dp, d), (f, d), (d, f), (d, dp)) + lora_tn, dev)
        ws_at = lay.attn_workspace(H, dev)
        dz = b16(T, f)
        dh = b16(T, d)
        dctx = b16(T, dp) if self._padded else dh
        dqkv = b16(T, 3 * dp)
        ready_hi = self._total
        if self._padded:      # weight gradients come out in the padded-head layout and are gathered back into the arena gradient
            rowmap, colmap = self._head_pad_maps()
            gw_qkv, gb_qkv, gw_o = torch.empty(3 * dp, d, device=dev), torch.empty(3 * dp, device=dev), torch.empty(d, dp, device=dev)
        # FFN-1 and QKV weight gradients each in one launch with the LayerNorm backward that follows their data gradient (disjoint CUs: oneprot_gemm_tn_ln_bwd).
        # Single rank only: the CUs of the LayerNorm role on top of an all-reduce's reserve have not been measured.
        wg_ln = (hip.wgrad_ln_wanted() and not self._lora and not self._padded and hip.cu_reserve_wanted() == 0 and int(os.environ.get("WORLD_SIZE", "1")) == 1
                 and hip.query("oneprot_gemm_tn_ln_bwd_eligible", T, f, d) == 1 and hip.query("oneprot_gemm_tn_ln_bwd_eligible", T, 3 * dp, d) == 1)
        bounds = saved.get("bounds")
        seg_of_top = {hi - 1: (lo, hi) for lo, hi in saved["plan"][:-1]} if bounds is not None else {}
        for i in reversed(range(self.n_layers)):
            if i in seg_of_top:      # entering a segment the forward did not keep: re-run it from its boundary record first
                self._recompute_segment(saved, *seg_of_top[i])
            st = saved["layers"][i]
            p = f"encoder.layer.{i}."
            # ---- FFN2: x_out = x_mid + u W2^T + b2        (weight grad + bias grad in one TN launch)
            self._wgrad(g16, st["u"], T, d, f, gv(p + "output.dense.weight"), gv(p + "output.dense.bias"), ws_tn)
            hip.gemm_nt(g16, self._bf16_T[(i, "w2")], T, f, d, hip.EPI_GELU_BWD, dz, aux=st["z"])
            # ---- FFN1: z = h2 W1^T + b1
            # ---- LN2 (input x_mid): g += LN'(dh); also refreshes the bf16 copy g16
            if wg_ln:      # data gradient first, then the weight gradient beside the LayerNorm backward
                hip.gemm_nt(dz, self._bf16_T[(i, "w1")], T, d, f, hip.EPI_BF16, dh)
                hip.gemm_tn_ln_bwd(dz, st["h2"], T, f, d, gv(p + "intermediate.dense.weight"), gv(p + "intermediate.dense.bias"), ws_tn, dh, st["x_mid"],
                                   self.view(p + "LayerNorm.weight"), st["mean2"], st["rstd2"], g, gv(p + "LayerNorm.weight"), gv(p + "LayerNorm.bias"), ws_ln,
                                   hip.wgrad_ln_cus(f), add_to=g, dx16=g16)
            else:
                self._wgrad(dz, st["h2"], T, f, d, gv(p + "intermediate.dense.weight"), gv(p + "intermediate.dense.bias"), ws_tn)
                hip.gemm_nt(dz, self._bf16_T[(i, "w1")], T, d, f, hip.EPI_BF16, dh)
                hip.layernorm_bwd(dh, 0, st["x_mid"], self.view(p + "LayerNorm.weight"), st["mean2"], st["rstd2"], g, gv(p + "LayerNorm.weight"), gv(p + "LayerNorm.bias"),
                                  ws_ln, T, d, add_to=g, dx16=g16)
            # ---- out-proj: x_mid = x_in + ctx Wo^T + bo
            hip.gemm_tn(g16, st["ctx"], T, d, dp, gw_o if self._padded else gv(p + "attention.output.dense.weight"), gv(p + "attention.output.dense.bias"), ws_tn)
            hip.gemm_nt(g16, self._bf16_T[(i, "o")], T, dp, d, hip.EPI_BF16, dctx)
            # ---- attention
            lay.attn_bwd(st, dctx, q_scale, dqkv, ws_at, H, hd)
            # ---- QKV projection
            (o, n), (ob, nb) = self._qkv_spans(i)
            if not wg_ln:
                hip.gemm_tn(dqkv, st["h1"], T, 3 * dp, d, gw_qkv if self._padded else gflat[o:o + n], gb_qkv if self._padded else gflat[ob:ob + nb], ws_tn)
            if self._padded:
                gv(p + "attention.output.dense.weight").copy_(gw_o[:, colmap])
                gflat[o:o + n].view(3 * d, d).copy_(gw_qkv[rowmap])
                gflat[ob:ob + nb].copy_(gb_qkv[rowmap])
            hip.gemm_nt(dqkv, self._bf16_T[(i, "qkv")], T, d, 3 * dp, hip.EPI_BF16, dh)
            if lora_raw is not None:      # two-branch LoRA: adapter gradients, and dh += mask * (du A) / keep
                self._lora_branch_backward(i, st["h1"], st["lora_u"], dqkv, T, saved["lora_call"], ws_tn, lora_raw, dh16=dh)
            # ---- LN1 (input x_in)
            if wg_ln:
                hip.gemm_tn_ln_bwd(dqkv, st["h1"], T, 3 * dp, d, gflat[o:o + n], gflat[ob:ob + nb], ws_tn, dh, st["x_in"], self.view(p + "attention.LayerNorm.weight"),
                                   st["mean1"], st["rstd1"], g, gv(p + "attention.LayerNorm.weight"), gv(p + "attention.LayerNorm.bias"), ws_ln,
                                   hip.wgrad_ln_cus(3 * dp), add_to=g, dx16=g16)
            else:
                hip.layernorm_bwd(dh, 0, st["x_in"], self.view(p + "attention.LayerNorm.weight"), st["mean1"], st["rstd1"], g, gv(p + "attention.LayerNorm.weight"),
                                  gv(p + "attention.LayerNorm.bias"), ws_ln, T, d, add_to=g, dx16=g16)
            saved["layers"][i] = st = None      # release this layer's activations
            if bounds is not None:
                bounds.pop(i, None)      # ... and, under its bottom layer, the segment's boundary record
            if on_ready is not None and i > 0 and i % self.GRAD_CHUNK_LAYERS == 0:
                lo = self._spec[f"encoder.layer.{i}.attention.self.query.weight"][0]
                on_ready(lo, ready_hi)
                ready_hi = lo
        lay.embed_bwd(self, g, gv("embeddings.word_embeddings.weight"))
        if on_ready is not None:
            on_ready(0, ready_hi)

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, **_):
        """EsmModel-compatible call returning .last_hidden_state (no autograd; the trainable path is
        oneprot_amd.encoders' fused encode).  Packed input: last_hidden_state is the stream's [T_pad, d] (tail rows: the pad embedding's)."""
        x, _ = self.run_layers(input_ids, save=False)
        return _Out(layout.of(self, input_ids).final_hidden(self, x))

    @classmethod
    def from_pretrained(cls, model_name_or_path, config=None, add_pooling_layer=True, **_):
        cfg, path = resolve_config(model_name_or_path)
        if config is not None:
            cfg = config
        sd = load_weight_file(path)
        if sd is not None:
            sd = {(k[4:] if k.startswith("esm.") else k): v for k, v in sd.items()}
        model, missing, _ = cls._from_checkpoint(sd, model_name_or_path, "model.safetensors / pytorch_model.bin", ("pooler.", "contact_head.", "extra."), cfg,
                                                 add_pooling_layer=add_pooling_layer)
        if missing:
            raise OSError(f"checkpoint {model_name_or_path} lacks tensors: {missing[:5]}...")
        return model
