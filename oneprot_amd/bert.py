"""BERT text tower on the HIP kernels -- what the reference obtains from `AutoModel.from_pretrained` in TextEncoder
(ref text_encoder.py:33) i.e. transformers' BertModel (hf modeling_bert.py:53-108 embeddings, 139-204 attention, 354-417 layer;
post-LN, 1/sqrt(hd) inside attention, erf-GELU).  State-dict keys are BertModel's.  Forward and hand-written backward
(`frozen=False`, the TextEncoder signature default).  Dropout follows the reference: HF's four train-mode dropouts (p = 0.1) are active whenever the
module is in train mode, also for the frozen tower (ref text_encoder.py:56-62 never switches it to eval -- SURVEY.md section 8 a7); `.eval()`,
`transformer.train_dropout = False` or ONEPROT_BERT_DROPOUT=0 run p = 0, which is what parity against the eval-mode reference is defined on
(see _train_dropout below)."""
import os

import torch

from . import hip
from . import layout
from .arena import ModelConfig, load_weight_file, _Out
from .esm import resolve_config
from .lora import LoraArena
from .packing import PackedTokens

BERT_DEFAULTS = dict(model_type="bert", vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                     max_position_embeddings=512, type_vocab_size=2, pad_token_id=0, layer_norm_eps=1e-12, initializer_range=0.02,
                     hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
KNOWN_BERT = {"BiomedNLP-BiomedBERT-base-uncased-abstract-fulltext": {}, "BiomedNLP-PubMedBERT-base-uncased-abstract-fulltext": {}, "bert-base-uncased": {}}


def resolve_bert_config(model_name_or_path):
    path = str(model_name_or_path)
    if os.path.isfile(os.path.join(path, "config.json")):
        cfg, p = resolve_config(path)
        base = dict(BERT_DEFAULTS)
        base.update(cfg.to_dict())
        return ModelConfig(**base), p
    if path.split("/")[-1] in KNOWN_BERT:
        return ModelConfig(**BERT_DEFAULTS), None
    raise OSError(f"{model_name_or_path} is not a local folder with a config.json and is not a known BERT model identifier")


class _BertPadded(layout.PaddedLayout):
    """The BERT stages of a padded [B, L] batch: embedding (position l = row % L) and the position-table gradient (sum over the batch)."""

    def embed(self, tr, x, h):
        cfg, e = tr.config, "embeddings."
        self.make_key_bias(cfg.pad_token_id)
        hip.call("oneprot_bert_embed_fwd", self.ids, tr.view(e + "word_embeddings.weight"), tr.view(e + "position_embeddings.weight"),
                 tr.view(e + "token_type_embeddings.weight"), tr.view(e + "LayerNorm.weight"), tr.view(e + "LayerNorm.bias"), x, h, self.B, self.L, tr.d,
                 cfg.vocab_size, cfg.layer_norm_eps)

    def pos_rows(self, tr):
        """the position-embedding row of every token: fp32 [T, d]"""
        return tr.view("embeddings.position_embeddings.weight")[:self.L].repeat(self.B, 1)

    def pos_bwd(self, de, dpos, d):
        """dpos rows 0 .. n-1 from de [T, d]: the sum over the batch; returns n"""
        hip.call("oneprot_rowsum_f32", de, dpos[:self.L], self.B, self.L * d)
        return self.L


class _BertPacked(layout.PackedLayout):
    """The same on a packed caption stream (pad id = the tower's pad_token_id; the QKV epilogue's rotary tables are the (1, 0) rows of _norope(T_pad)):
    absolute positions restart at every segment and the position-table gradient sums row l over the segments that reach it.

    Dropout: the attention-probability masks are those of the padded batch of the same captions in the same order (stream s * H + h, positions within
    the segment).  The hidden-state Philox masks are indexed by element of the [T_pad, d] stream, so they differ from the padded layout's [B * L, d]
    masks: the same distribution, another draw."""

    def embed(self, tr, x, h):
        cfg, e = tr.config, "embeddings."
        hip.call("oneprot_bert_embed_packed_fwd", self.ids, self.cu, tr.view(e + "word_embeddings.weight"), tr.view(e + "position_embeddings.weight"),
                 tr.view(e + "token_type_embeddings.weight"), tr.view(e + "LayerNorm.weight"), tr.view(e + "LayerNorm.bias"), x, h, self.N, self.T, tr.d,
                 cfg.vocab_size, cfg.max_position_embeddings, cfg.layer_norm_eps)

    def pos_rows(self, tr):
        # the position of every stream row, built on the host from the lengths (no device read-back); tail rows take position 0
        key = ("bert_pos", str(self.ids.device))
        idx = self.p._work.get(key)
        if idx is None:
            host = torch.zeros(self.T, dtype=torch.int64)
            host[:self.p.n_tokens] = torch.cat([torch.arange(n) for n in self.p.lengths])
            idx = self.p._work[key] = host.to(self.ids.device)
        return tr.view("embeddings.position_embeddings.weight")[idx]

    def pos_bwd(self, de, dpos, d):
        n = self.p.max_len
        hip.call("oneprot_segment_possum_f32", de, self.cu, dpos[:n], self.N, self.T, n, d)
        return n


class BertTransformer(LoraArena):
    final_layer_norm = False      # post-LN model: pooling reads the last layer's output directly
    layouts = (_BertPadded, _BertPacked)      # layout.of(self, ids)
    accepts_packed = True         # run_layers / backward_layers take a PackedTokens stream (oneprot_amd.packing)

    def __init__(self, config):
        super().__init__()
        self.config = config
        d, f, n = config.hidden_size, config.intermediate_size, config.num_hidden_layers
        self.d, self.f, self.n_layers, self.H = d, f, n, config.num_attention_heads
        self.hd = d // self.H
        if self.hd not in (16, 32, 64) or d % 64:
            raise NotImplementedError(f"head_dim {self.hd} / hidden {d}: kernels are built for head_dim 16/32/64, hidden % 64 == 0")
        self._init_arena()
        self._add("embeddings.word_embeddings.weight", (config.vocab_size, d))
        self._add("embeddings.position_embeddings.weight", (config.max_position_embeddings, d))
        self._add("embeddings.token_type_embeddings.weight", (getattr(config, "type_vocab_size", 2), d))
        self._add("embeddings.LayerNorm.weight", (d,))
        self._add("embeddings.LayerNorm.bias", (d,))
        for i in range(n):
            p = f"encoder.layer.{i}."
            for nm in ("query", "key", "value"):
                self._add(p + f"attention.self.{nm}.weight", (d, d))
            for nm in ("query", "key", "value"):
                self._add(p + f"attention.self.{nm}.bias", (d,))
            for nm, shp in (("attention.output.dense.weight", (d, d)), ("attention.output.dense.bias", (d,)), ("attention.output.LayerNorm.weight", (d,)),
                            ("attention.output.LayerNorm.bias", (d,)), ("intermediate.dense.weight", (f, d)), ("intermediate.dense.bias", (f,)),
                            ("output.dense.weight", (d, f)), ("output.dense.bias", (d,)), ("output.LayerNorm.weight", (d,)), ("output.LayerNorm.bias", (d,))):
                self._add(p + nm, shp)
        self._extra["pooler.dense.weight"] = (d, d)       # HF pooler: present in checkpoints, unused by the reference
        self._extra["pooler.dense.bias"] = (d,)
        self._finish_arena()
        self._ones_zeros = {}
        self.reset_parameters()

    _load_ignore_suffixes = ("embeddings.position_ids",)

    def _norope(self, L, dev):
        key = (L, dev)
        if key not in self._ones_zeros:
            self._ones_zeros[key] = (torch.ones(L, self.hd // 2, device=dev), torch.zeros(L, self.hd // 2, device=dev))
        return self._ones_zeros[key]

    def _refresh_bf16(self):
        if not self._refresh_bf16_mirror():
            return
        if self.flat.requires_grad:          # transposed bf16 weights for the dgrad GEMMs
            d, f = self.d, self.f
            self._transpose_qkv_weights()
            self._transpose_layer_weights("o", "encoder.layer.{i}.attention.output.dense.weight", d, d)
            self._transpose_layer_weights("w1", "encoder.layer.{i}.intermediate.dense.weight", f, d)
            self._transpose_layer_weights("w2", "encoder.layer.{i}.output.dense.weight", d, f)

    # ---- hf's train-mode dropout (hidden_dropout_prob / attention_probs_dropout_prob, 0.1 in bert-base).  The reference never switches its text tower
    # to eval mode (text_encoder.py:59), so even the frozen tower of the shipped configuration is stochastic there -- and so it is here since round 5:
    # ON by default in train mode (ONEPROT_BERT_DROPOUT=0 or `transformer.train_dropout = False` switch it off: the parity tests against the
    # eval-mode reference do).  All four dropouts, for a frozen tower (forward only) and a trainable one (the backward regenerates every mask: the dense
    # outputs' gradients pass through the same hidden masks, the attention backward runs its masked form, oneprot_attn_bwd_dropout).  Hidden masks come
    # from the counter-based generator of the LoRA dropout (Philox4x32-10 of seed, call, layer, site, element), the attention masks from a per-element hash.
    train_dropout = None

    def _train_dropout(self):
        on = self.train_dropout if self.train_dropout is not None else os.environ.get("ONEPROT_BERT_DROPOUT", "1") != "0"
        cfg = self.config
        if not (on and self.training):
            return False
        return float(cfg.hidden_dropout_prob) > 0 or float(cfg.attention_probs_dropout_prob) > 0

    def _drop_stream(self, call_id, layer, site):
        """stream id of a dropout site: layer -1 = embeddings; site 0 = attention probabilities, 1 = attention output dense, 2 = FFN output dense"""
        return self._rng_stream(self.RNG_DOMAIN_BERT, (call_id * (self.n_layers + 1) + (layer + 1)) * 4 + site)

    @torch.no_grad()
    def run_layers(self, ids, save=False):
        """Embeddings + n post-LN layers on padded ids [B, L] or a PackedTokens stream (B = 1, L = T_pad for every row-wise stage).
        Returns (last hidden state fp32 [T,d], saved-dict or None)."""
        cfg = self.config
        if isinstance(ids, PackedTokens) and ids.max_len > cfg.max_position_embeddings:
            raise ValueError(f"sequence length {ids.max_len} exceeds max_position_embeddings {cfg.max_position_embeddings}")
        if not ids.is_cuda:
            raise hip.HipKernelError("OneProt HIP path needs CUDA(ROCm) tensors; there is no CPU fallback")
        self._refresh_bf16()
        lay = layout.of(self, ids)
        B, L = lay.B, lay.L
        if not lay.packed and L > cfg.max_position_embeddings:
            raise ValueError(f"sequence length {L} exceeds max_position_embeddings {cfg.max_position_embeddings}")
        T, d, f, H, hd = B * L, self.d, self.f, self.H, self.hd
        dev = ids.device
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        b16 = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
        one, zero = self._norope(L, dev)
        x, h, tmp = f32(T, d), b16(T, d), f32(T, d)
        lay.embed(self, x, h)
        drop = self._train_dropout()
        if drop:      # hf's train-mode dropouts: embeddings, attention probabilities, the two dense outputs of every layer
            drop_call = self._next_call()
            p_h, p_a = float(cfg.hidden_dropout_prob), float(cfg.attention_probs_dropout_prob)
            y_drop = f32(T, d)
            hip.call("oneprot_dropout_f32", x, x, T * d, p_h, self._drop_seed, self._drop_stream(drop_call, -1, 0))
            hip.call("oneprot_cast_f32_to_bf16", x, h, T * d)
        saved = dict(layout=lay, layers=[], B=B, L=L) if save else None
        if drop and save:
            saved["drop_call"] = drop_call
        q, k, v, ctx, u = b16(B, H, L, hd), b16(B, H, L, hd), b16(B, H, L, hd), b16(T, d), b16(T, f)
        eps = cfg.layer_norm_eps
        lora_call = self._lora_next_call()
        if save and lora_call is not None:
            saved["lora_call"] = lora_call
        for i in range(self.n_layers):
            p = f"encoder.layer.{i}."
            if save:     # per layer: input (bf16), attention operands, the two pre-LN sums with their statistics, FFN intermediates
                st = dict(x16=h, q=b16(B, H, L, hd), k=b16(B, H, L, hd), v=b16(B, H, L, hd), ctx=b16(T, d), lse=f32(B, H, L), s1=f32(T, d), mean1=f32(T), rstd1=f32(T),
                          y1=f32(T, d), y16=b16(T, d), z=torch.empty(T, f, dtype=torch.uint8, device=dev), u=b16(T, f), s2=f32(T, d), mean2=f32(T), rstd2=f32(T))
                q, k, v, ctx, u, z, lse = st["q"], st["k"], st["v"], st["ctx"], st["u"], st["z"], st["lse"]
                s1, s2, y1, y16, x_out, h_out = st["s1"], st["s2"], st["y1"], st["y16"], f32(T, d), b16(T, d)
                m1, r1, m2, r2 = st["mean1"], st["rstd1"], st["mean2"], st["rstd2"]
            else:
                z = lse = m1 = r1 = m2 = r2 = None
                s1 = s2 = tmp
                y1, y16, x_out, h_out = x, h, x, h
            (o, n), (ob, nb) = self._qkv_spans(i)
            # rotary tables (1, 0) turn the QKV epilogue into "q *= 1/sqrt(hd), head-major q/k/v" (scores scaled inside attention in HF: same product)
            lora_u = self._qkv_forward(i, h, self._bf16[o:o + n], self.flat.data[ob:ob + nb], T, 3 * d, (one, zero, L, H, hd), hd ** -0.5 * hip.LOG2E, q, k, v, lora_call)
            if save:
                st["lora_u"] = lora_u
            lay.attn_fwd(q, k, v, ctx, lse, H, hd, drop=drop and (p_a, self._drop_seed, self._drop_stream(drop_call, i, 0)))
            if drop:
                # s1 = x + dropout(ctx Wo^T + bo): the residual add leaves the GEMM epilogue so that the mask can sit between the two
                hip.gemm_nt(ctx, self._w16(p + "attention.output.dense.weight"), T, d, d, hip.EPI_F32, y_drop, bias=self.view(p + "attention.output.dense.bias"))
                # ... and the LayerNorm that follows reads the sum where it is formed (one kernel; a frozen tower never writes the sum)
                hip.call("oneprot_dropout_add_layernorm_fwd", y_drop, x, s1 if save else None, self.view(p + "attention.output.LayerNorm.weight"),
                         self.view(p + "attention.output.LayerNorm.bias"), y16, y1, m1, r1, T, d, eps, p_h, self._drop_seed, self._drop_stream(drop_call, i, 1))
            else:
                hip.gemm_nt(ctx, self._w16(p + "attention.output.dense.weight"), T, d, d, hip.EPI_BIAS_RESID, s1, bias=self.view(p + "attention.output.dense.bias"),
                            aux=x)
                hip.layernorm_fwd(s1, self.view(p + "attention.output.LayerNorm.weight"), self.view(p + "attention.output.LayerNorm.bias"), T, d, eps,
                                  y16=y16, y32=y1, mean=m1, rstd=r1)
            hip.gemm_nt(y16, self._w16(p + "intermediate.dense.weight"), T, f, d, hip.EPI_BIAS_GELU, u, bias=self.view(p + "intermediate.dense.bias"), out1=z)
            if drop:
                hip.gemm_nt(u, self._w16(p + "output.dense.weight"), T, d, f, hip.EPI_F32, y_drop, bias=self.view(p + "output.dense.bias"))
                hip.call("oneprot_dropout_add_layernorm_fwd", y_drop, y1, s2 if save else None, self.view(p + "output.LayerNorm.weight"),
                         self.view(p + "output.LayerNorm.bias"), h_out, x_out, m2, r2, T, d, eps, p_h, self._drop_seed, self._drop_stream(drop_call, i, 2))
            else:
                hip.gemm_nt(u, self._w16(p + "output.dense.weight"), T, d, f, hip.EPI_BIAS_RESID, s2, bias=self.view(p + "output.dense.bias"), aux=y1)
                hip.layernorm_fwd(s2, self.view(p + "output.LayerNorm.weight"), self.view(p + "output.LayerNorm.bias"), T, d, eps,
                                  y16=h_out, y32=x_out, mean=m2, rstd=r2)
            if save:
                saved["layers"].append(st)
            x, h = x_out, h_out
        if save:
            saved["x_final"] = x
        return x, saved

    def backward_layers(self, saved, g, g16, gflat, on_ready=None):
        """g: fp32 [T,d] gradient w.r.t. the last layer's output (consumed), g16 unused (post-LN layers start with a LayerNorm backward);
        gflat: fp32 arena gradient (written).  Per layer, backwards (hf modeling_bert.py:354-417):
          y2 = LN2(s2), s2 = y1 + gelu(y1 W1^T + b1) W2^T + b2 ;  y1 = LN1(s1), s1 = x + attn(x) Wo^T + bo."""
        lay = saved["layout"]
        B, L = saved["B"], saved["L"]
        T, d, f, H, hd = B * L, self.d, self.f, self.H, self.hd
        dev = g.device
        cfg = self.config
        gv = lambda name: self.view(name, gflat)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        b16 = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
        ws_ln = torch.empty(hip.query("oneprot_layernorm_bwd_workspace", d), dtype=torch.uint8, device=dev)
        lora_raw, lora_tn = self._lora_backward_setup(saved, dev)
        ws_tn = self._tn_workspace(((3 * d, d), (f, d), (d, f), (d, d)) + lora_tn, dev)
        ws_at = lay.attn_workspace(H, dev)
        ds, ds16, gy = f32(T, d), b16(T, d), f32(T, d)
        dz, dctx, dqkv = b16(T, f), b16(T, d), b16(T, 3 * d)
        drop_call = saved.get("drop_call")                 # the forward ran hf's train-mode dropouts: every mask is regenerated from (seed, call, layer, site)
        if drop_call is not None:
            p_h, p_a = float(cfg.hidden_dropout_prob), float(cfg.attention_probs_dropout_prob)
            dm16 = b16(T, d)                                # gradient of a dense output = the pre-LN sum's gradient through that output's mask
        for i in reversed(range(self.n_layers)):
            st = saved["layers"][i]
            p = f"encoder.layer.{i}."
            # ---- LN2: ds = LN2'(g)  (fp32 + bf16 copy)
            hip.layernorm_bwd(g, 1, st["s2"], self.view(p + "output.LayerNorm.weight"), st["mean2"], st["rstd2"], ds, gv(p + "output.LayerNorm.weight"),
                              gv(p + "output.LayerNorm.bias"), ws_ln, T, d, dx16=ds16)
            # ---- FFN2 (weight + bias grads in one TN launch), then du * gelu'(z) in the dgrad epilogue
            do16 = ds16
            if drop_call is not None:
                hip.call("oneprot_dropout_bf16", ds16, dm16, T * d, p_h, self._drop_seed, self._drop_stream(drop_call, i, 2))
                do16 = dm16
            self._wgrad(do16, st["u"], T, d, f, gv(p + "output.dense.weight"), gv(p + "output.dense.bias"), ws_tn)
            hip.gemm_nt(do16, self._bf16_T[(i, "w2")], T, f, d, hip.EPI_GELU_BWD, dz, aux=st["z"])
            # ---- FFN1; gy = ds (residual branch) + dz W1
            self._wgrad(dz, st["y16"], T, f, d, gv(p + "intermediate.dense.weight"), gv(p + "intermediate.dense.bias"), ws_tn)
            hip.gemm_nt(dz, self._bf16_T[(i, "w1")], T, d, f, hip.EPI_BIAS_RESID, gy, aux=ds)
            # ---- LN1: ds = LN1'(gy)
            hip.layernorm_bwd(gy, 1, st["s1"], self.view(p + "attention.output.LayerNorm.weight"), st["mean1"], st["rstd1"], ds,
                              gv(p + "attention.output.LayerNorm.weight"), gv(p + "attention.output.LayerNorm.bias"), ws_ln, T, d, dx16=ds16)
            # ---- out-proj
            da16 = ds16
            if drop_call is not None:
                hip.call("oneprot_dropout_bf16", ds16, dm16, T * d, p_h, self._drop_seed, self._drop_stream(drop_call, i, 1))
                da16 = dm16
            self._wgrad(da16, st["ctx"], T, d, d, gv(p + "attention.output.dense.weight"), gv(p + "attention.output.dense.bias"), ws_tn)
            hip.gemm_nt(da16, self._bf16_T[(i, "o")], T, d, d, hip.EPI_BF16, dctx)
            # ---- attention (no rotary: cos/sin = null)
            lay.attn_bwd(st, dctx, hd ** -0.5, dqkv, ws_at, H, hd, drop=drop_call is not None and (p_a, self._drop_seed, self._drop_stream(drop_call, i, 0)))
            # ---- QKV projection; g = ds (residual branch) + dqkv Wqkv
            (o, n), (ob, nb) = self._qkv_spans(i)
            hip.gemm_tn(dqkv, st["x16"], T, 3 * d, d, gflat[o:o + n], gflat[ob:ob + nb], ws_tn)
            hip.gemm_nt(dqkv, self._bf16_T[(i, "qkv")], T, d, 3 * d, hip.EPI_BIAS_RESID, g, aux=ds)
            if lora_raw is not None:      # two-branch LoRA: adapter gradients, and g += mask * (du A) / keep
                self._lora_branch_backward(i, st["x16"], st["lora_u"], dqkv, T, saved["lora_call"], ws_tn, lora_raw, dh32=g)
            saved["layers"][i] = None
        if drop_call is not None:                          # x0 = dropout(LN(embeddings))
            hip.call("oneprot_dropout_f32", g, g, T * d, p_h, self._drop_seed, self._drop_stream(drop_call, -1, 0))
        self._embedding_backward(lay, g, gflat)
        if on_ready is not None:
            on_ready(0, self._total)

    def _embedding_backward(self, lay, g, gflat):
        """x0 = LN(word[id] + pos[l] + type[0]) (hf modeling_bert.py:53-108).  The pre-LN sum is re-gathered (torch indexing: data movement),
        LayerNorm statistics / backward and the table reductions are HIP kernels; equal token ids are summed in sorted order.  On a packed stream l is the
        position within the segment and the tail rows (pad ids, zero gradient rows) add nothing to any table."""
        cfg = self.config
        ids = lay.ids
        T, d, dev = lay.T, self.d, ids.device
        e = "embeddings."
        gv = lambda name: self.view(name, gflat)
        esum = (self.view(e + "word_embeddings.weight")[ids.reshape(-1)] + lay.pos_rows(self)
                + self.view(e + "token_type_embeddings.weight")[0]).contiguous()
        mean, rstd, y = torch.empty(T, device=dev), torch.empty(T, device=dev), torch.empty(T, d, device=dev)
        hip.layernorm_fwd(esum, self.view(e + "LayerNorm.weight"), self.view(e + "LayerNorm.bias"), T, d, cfg.layer_norm_eps, y32=y, mean=mean, rstd=rstd)
        de = torch.empty(T, d, device=dev)
        ws_ln = torch.empty(hip.query("oneprot_layernorm_bwd_workspace", d), dtype=torch.uint8, device=dev)
        hip.layernorm_bwd(g, 1, esum, self.view(e + "LayerNorm.weight"), mean, rstd, de, gv(e + "LayerNorm.weight"), gv(e + "LayerNorm.bias"), ws_ln, T, d)
        # position rows 0..n-1: sum over the batch (packed: over the segments that reach the row); token-type row 0: sum over positions of that
        dpos = gv(e + "position_embeddings.weight")
        n = lay.pos_bwd(de, dpos, d)
        hip.call("oneprot_rowsum_f32", dpos[:n], gv(e + "token_type_embeddings.weight")[0], n, d)
        # word rows: stable sort of the ids, one block per run of equal ids (padding_idx row gets no gradient, as nn.Embedding)
        sorted_ids, perm = torch.sort(ids.reshape(-1), stable=True)
        rows, counts = torch.unique_consecutive(sorted_ids, return_counts=True)
        starts = (torch.cumsum(counts, 0) - counts).contiguous()
        pad = cfg.pad_token_id if cfg.pad_token_id is not None else -1
        hip.call("oneprot_embed_scatter_sorted", de, perm.contiguous(), starts, rows.contiguous(), T, int(rows.numel()), d, pad, gv(e + "word_embeddings.weight"))

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, **_):
        """BertModel-compatible call returning .last_hidden_state; a packed input gives the stream's [T_pad, d] (tail rows: finite, meaningless)"""
        x, _ = self.run_layers(input_ids, save=False)
        return _Out(layout.of(self, input_ids).final_hidden(self, x))

    @classmethod
    def from_pretrained(cls, model_name_or_path, **_):
        cfg, path = resolve_bert_config(model_name_or_path)
        sd = load_weight_file(path)
        if sd is not None:
            sd = {(k[5:] if k.startswith("bert.") else k): v for k, v in sd.items() if not k.startswith("cls.")}
        model, missing, _ = cls._from_checkpoint(sd, model_name_or_path, "model.safetensors / pytorch_model.bin", ("pooler.", "extra."), cfg)
        if missing:
            raise OSError(f"checkpoint {model_name_or_path} lacks tensors: {missing[:5]}...")
        return model
