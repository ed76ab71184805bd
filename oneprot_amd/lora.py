"""peft-LoRA on the q / k / v projections of an arena tower (ESM, BERT): the adapters, their state-dict keys, the merged and the two-branch forms of
the fused QKV GEMM and their gradients -- and the plumbing both towers' layer loops share around that GEMM."""
import math
import warnings

import torch
import torch.nn as nn

from . import hip
from .arena import ArenaModule


class LoraArena(ArenaModule):
    """An arena whose q | k | v projections (HF names, encoder.layer.{i}.attention.self.*) can carry a LoRA adapter."""

    # ------------------------------------------------------------------------------------------------- LoRA (peft 0.5.0 semantics)
    # ref sequence_encoder.py:61-74 / text_encoder.py:39-52: get_peft_model(transformer, LoraConfig(r, lora_alpha, lora_dropout,
    # target_modules=[query,key,value], bias="all")).  peft's lora.Linear computes  y = x W^T + b + (alpha/r) * (dropout(x) A^T) B^T  with
    # A ~ kaiming_uniform(a=sqrt(5)), B = 0; only lora_A / lora_B and every parameter whose name contains "bias" stay trainable; the wrapped
    # model's keys gain the prefix "base_model.model." and the adapters are "<linear>.lora_{A,B}.default.weight".
    # Here: the adapters are two stacked parameters.  In eval mode (and with lora_dropout = 0) the bf16 GEMM operand of a target is the merged
    # W + (alpha/r) B A -- peft's forward at dropout 0 -- and the hand-written backward yields d(W_eff), from which dA = s B^T dW and
    # dB = s dW A^T follow.  In TRAIN mode with lora_dropout > 0 the two branches stay apart, as in peft: the fused QKV GEMM runs on the
    # K-concatenated operands [h | dropout(h) A^T] x [W | s B]^T (one launch, the rotary epilogue unchanged), the mask comes from a counter-based
    # generator (oneprot_dropout_bf16: a pure function of seed, call, layer, element) and is regenerated in the backward, where
    # du = dqkv (sB), dB = s dqkv^T u, dA = du^T dropout(h) and the layer-input gradient gains mask * (du A) / keep.
    # Either way the arena gradient is masked down to its "bias" entries (peft bias="all").
    LORA_TARGETS = ("query", "key", "value")

    def enable_lora(self, r, alpha, target_modules, dropout=0.0):
        targets = [t for t in self.LORA_TARGETS if t in list(target_modules)]
        if len(targets) != len(list(target_modules)):
            raise NotImplementedError(f"LoRA target modules {list(target_modules)}: only {list(self.LORA_TARGETS)} (the reference's list) are built")
        n, d = self.n_layers, self.d
        A = torch.empty(n, len(targets), r, d)
        A.uniform_(-1.0 / math.sqrt(d), 1.0 / math.sqrt(d))              # kaiming_uniform_(a=sqrt(5)) on [r, d]
        self.lora_A = nn.Parameter(A)
        self.lora_B = nn.Parameter(torch.zeros(n, len(targets), d, r))
        self._lora = dict(r=r, alpha=alpha, scaling=alpha / r, targets=targets, dropout=dropout)
        self._key_prefix = "base_model.model."                          # the keys of a PeftModel
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"lora_dropout must be in [0, 1), got {dropout}")
        self._seed_streams("_lora")
        for p in self.parameters():
            p.requires_grad = False
        self.lora_A.requires_grad = True
        self.lora_B.requires_grad = True
        self.flat.requires_grad = True                                   # bias="all": only the "bias" entries receive a gradient (mask below)
        idx = torch.cat([torch.arange(off, off + cnt) for name, (off, cnt, _) in self._spec.items() if "bias" in name])
        self.register_buffer("_lora_bias_index", idx, persistent=False)
        self._bf16_version = None

    def _qkv_spans(self, i):
        """((o, n), (ob, nb)): the arena ranges of layer i's fused q|k|v weight [3d, d] and bias [3d]"""
        p = f"encoder.layer.{i}.attention.self."
        return self.span(p + "query.weight", p + "value.weight"), self.span(p + "query.bias", p + "value.bias")

    def _lora_key(self, prefix, i, t, which):
        return f"{prefix}encoder.layer.{i}.attention.self.{t}.lora_{which}.default.weight"

    def _sd_hook(self, module, state_dict, prefix, local_metadata):
        super()._sd_hook(module, state_dict, prefix, local_metadata)
        if self._lora:
            base = prefix + self._key_prefix
            A, B = state_dict.pop(prefix + "lora_A"), state_dict.pop(prefix + "lora_B")
            for i in range(self.n_layers):
                for ti, t in enumerate(self._lora["targets"]):
                    state_dict[self._lora_key(base, i, t, "A")] = A[i, ti]
                    state_dict[self._lora_key(base, i, t, "B")] = B[i, ti]
        return state_dict

    def _load_hook(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        at = len(missing_keys)
        super()._load_hook(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        if self._lora:
            A, B, lost = self.lora_A.detach().clone(), self.lora_B.detach().clone(), []
            for i in range(self.n_layers):
                for ti, t in enumerate(self._lora["targets"]):
                    for which, dst in (("A", A), ("B", B)):
                        key = self._lora_key(prefix, i, t, which)
                        if key in state_dict:
                            dst[i, ti] = state_dict.pop(key).to(dst)
                        elif prefix + "lora_" + which not in state_dict:
                            lost.append(key)
            missing_keys[at:at] = lost                                   # reported ahead of the arena's own missing tensors
            state_dict.setdefault(prefix + "lora_A", A)
            state_dict.setdefault(prefix + "lora_B", B)

    def _refresh_bf16_mirror(self):
        two = self._lora_two_branch()
        if not super()._refresh_bf16_mirror((self.lora_A._version, self.lora_B._version, two) if self._lora else ()):
            return False
        if two:                          # train mode with lora_dropout: the mirror keeps the base weights, the adapters ride in the concatenated operands
            self._lora_refresh_branch_operands()
        elif self._lora:                 # merged operands W + (alpha/r) B A for the target projections
            for i in range(self.n_layers):
                w = self._qkv_effective_f32(i)
                o, n = self._qkv_spans(i)[0]
                hip.call("oneprot_cast_f32_to_bf16", w, self._bf16[o:o + n], n)
        return True

    def _transpose_qkv_weights(self):
        """the [d, 3d] transposed bf16 copies of the fused q|k|v weights (dgrad operand): one launch over the arena, or per layer from
        the LoRA-merged scratch"""
        d = self.d
        if not self._lora:
            return self._transpose_layer_weights("qkv", "encoder.layer.{i}.attention.self.query.weight", 3 * d, d)
        for i in range(self.n_layers):
            t = self._bf16_T.get((i, "qkv"))
            if t is None:
                t = self._bf16_T[(i, "qkv")] = torch.empty(d, 3 * d, dtype=torch.bfloat16, device=self.flat.device)
            hip.call("oneprot_transpose_cast_f32_to_bf16", self._qkv_effective_f32(i), t, 3 * d, d)

    def _qkv_effective_f32(self, i):
        """fp32 [3d, d] fused q|k|v weight of layer i as the GEMMs must see it: the arena view, or (LoRA) a scratch copy with (alpha/r) B A
        added to the target blocks."""
        o, n = self._qkv_spans(i)[0]
        w = self.flat.data[o:o + n]
        if not self._lora or self._lora_two_branch():
            return w
        d, r = self.d, self._lora["r"]
        if getattr(self, "_lora_scratch", None) is None or self._lora_scratch.device != w.device:
            self._lora_scratch = torch.empty(3 * d * d, device=w.device)
        tmp = self._lora_scratch
        tmp.copy_(w)
        for ti, t in enumerate(self._lora["targets"]):
            blk = self.LORA_TARGETS.index(t)
            hip.call("oneprot_sgemm", self.lora_B.data[i, ti], self.lora_A.data[i, ti], tmp[blk * d * d:(blk + 1) * d * d], d, d, r, 0, 1, self._lora["scaling"], 1)
        return tmp

    def _wgrad(self, dY, X, T, N, K, dW, db, ws):
        """weight + bias gradient of one Linear; under LoRA the base weight is frozen, so only the bias gradient (column sums of dY) is formed"""
        if self._lora:
            hip.call("oneprot_colsum_bf16", dY, db, ws, T, N, 0)
        else:
            hip.gemm_tn(dY, X, T, N, K, dW, db, ws)

    def lora_backward(self, gflat):
        """(dA, dB) and `gflat` reduced to its "bias" entries (peft bias="all").  Merged form: from the gradient w.r.t. the merged weights left in
        `gflat`; two-branch form: from the per-layer adapter gradients backward_layers left in self._lora_raw."""
        d, r, s_ = self.d, self._lora["r"], self._lora["scaling"]
        dA, dB = torch.empty_like(self.lora_A), torch.empty_like(self.lora_B)
        raw = getattr(self, "_lora_raw", None)
        if raw is not None:
            self._lora_raw = None
            dA_raw, dB_raw = raw                                             # [n, Rp, d], [n, 3d, Rp]; target ti at rows / columns ti * rp .. + r
            rp = self._lora_ops["rp"]
            for ti, t in enumerate(self._lora["targets"]):
                blk = self.LORA_TARGETS.index(t)
                dA[:, ti] = dA_raw[:, ti * rp:ti * rp + r]
                dB[:, ti] = s_ * dB_raw[:, blk * d:(blk + 1) * d, ti * rp:ti * rp + r]
        else:
            for i in range(self.n_layers):
                for ti, t in enumerate(self._lora["targets"]):
                    dW = self.view(f"encoder.layer.{i}.attention.self.{t}.weight", gflat)
                    hip.call("oneprot_sgemm", dW, self.lora_A.data[i, ti], dB[i, ti], d, r, d, 0, 0, s_, 0)        # dB = s dW A^T
                    hip.call("oneprot_sgemm", self.lora_B.data[i, ti], dW, dA[i, ti], r, d, d, 1, 1, s_, 0)        # dA = s B^T dW
        masked = torch.zeros_like(gflat)
        idx = self._lora_bias_index
        masked[idx] = gflat[idx]
        return dA, dB, masked

    # ---- LoRA in train mode with lora_dropout > 0: peft's two-branch form (see the comment above enable_lora)
    def _lora_two_branch(self):
        if not (bool(self._lora) and self._lora["dropout"] > 0 and self.training):
            return False
        if getattr(self, "_padded", False):      # head_dim 24 models run their QKV operands in a padded layout: the concatenated form is not built for it
            if not getattr(self, "_lora_pad_warned", False):
                self._lora_pad_warned = True
                warnings.warn("lora_dropout is not applied to this padded-head model (head_dim not in 16/32/64): the adapters run merged into the weights, "
                              "which is peft's forward at dropout 0 (INTEGRATION.md, 'Deviations')", stacklevel=3)
            return False
        return True

    def _lora_next_call(self):
        """a run_layers call in the two-branch form draws its id (its own masks; the backward regenerates them from (seed, call, layer)), else None"""
        return self._next_call("_lora") if self._lora_two_branch() else None

    def _qkv_forward(self, i, h, w_qkv, b_qkv, T, n_out, rope, q_scale, q, k, v, lora_call):
        """Layer i's fused QKV GEMM with the rotary / head-major epilogue: h [T, d] x w_qkv^T, or (lora_call not None) peft's two branches in one launch,
        [h | dropout(h) A^T] x [W | s B]^T with K = Kc.  Returns u, the adapter columns the backward needs, or None."""
        if lora_call is None:
            hip.gemm_nt(h, w_qkv, T, n_out, self.d, hip.EPI_QKV_ROPE, q, bias=b_qkv, out1=k, out2=v, rope=rope, q_scale=q_scale)
            return None
        xc, u = self._lora_branch_operand(i, h, T, lora_call)
        hip.gemm_nt(xc, self._lora_ops["Wc"][i], T, n_out, self._lora_ops["Kc"], hip.EPI_QKV_ROPE, q, bias=b_qkv, out1=k, out2=v, rope=rope, q_scale=q_scale)
        return u

    def _lora_backward_setup(self, saved, dev):
        """(adapter-gradient buffers, also left in self._lora_raw for lora_backward; their TN-workspace shapes) after a two-branch forward, else (None, ())"""
        if "lora_call" not in saved:
            return None, ()
        self._lora_raw = self._lora_raw_buffers(dev)
        return self._lora_raw, ((3 * self.d, self._lora_ops["Rp"]), (self._lora_ops["rp"], self.d))

    def _lora_refresh_branch_operands(self):
        """bf16 operands of the two-branch form for every layer: Wc [n, 3d, Kc] = [W | s B (block-diagonal over the targets) | 0] for the
        K-concatenated QKV GEMM, Acat [n, Rp, d] (the targets' A stacked, each padded to rp = ceil8(r) rows), AtT [n, targets, d, rp] and BsT [n, Rp, 3d] for the backward.
        Runs after every optimizer step (the adapters moved): the buffers are allocated once and refilled in place -- the frozen base weights as ONE
        strided copy out of the bf16 mirror (the q|k|v block sits at the same offset in every layer of the arena), the r-wide adapter columns by
        slice assignment; the zero padding is written once, at allocation."""
        lo, n, d, dev = self._lora, self.n_layers, self.d, self.flat.device
        r, nt, s_ = lo["r"], len(lo["targets"]), lo["scaling"]
        rp = -(-r // 8) * 8
        Rp = nt * rp
        Kc = -(-(d + Rp) // 128) * 128
        bf = torch.bfloat16
        ops = getattr(self, "_lora_ops", None)
        if ops is None or ops["Wc"].device != dev or ops["Kc"] != Kc or ops["rp"] != rp:
            ops = self._lora_ops = dict(rp=rp, Rp=Rp, Kc=Kc, Wc=torch.zeros(n, 3 * d, Kc, dtype=bf, device=dev), Acat=torch.zeros(n, Rp, d, dtype=bf, device=dev),
                                        AtT=torch.zeros(n, nt, d, rp, dtype=bf, device=dev), BsT=torch.zeros(n, Rp, 3 * d, dtype=bf, device=dev))
        o0, cnt = self._qkv_spans(0)[0]
        stride = self._qkv_spans(1)[0][0] - o0 if n > 1 else cnt
        assert cnt == 3 * d * d
        ops["Wc"][:, :, :d].copy_(torch.as_strided(self._bf16, (n, 3 * d, d), (stride, d, 1), o0))
        for ti, t in enumerate(lo["targets"]):
            blk = self.LORA_TARGETS.index(t)
            a16 = self.lora_A.data[:, ti].to(bf)                                  # [n, r, d]
            b16 = (s_ * self.lora_B.data[:, ti]).to(bf)                           # [n, d, r]
            ops["Acat"][:, ti * rp:ti * rp + r] = a16
            ops["AtT"][:, ti, :, :r] = a16.transpose(1, 2)
            ops["Wc"][:, blk * d:(blk + 1) * d, d + ti * rp:d + ti * rp + r] = b16
            ops["BsT"][:, ti * rp:ti * rp + r, blk * d:(blk + 1) * d] = b16.transpose(1, 2)

    def _lora_scratch_for(self, T, dev):
        sc = getattr(self, "_lora_branch_scratch", None)
        if sc is None or sc["key"] != (T, dev, self._lora_ops["Kc"]):
            sc = dict(key=(T, dev, self._lora_ops["Kc"]), hd=torch.empty(T, self.d, dtype=torch.bfloat16, device=dev),
                      ut=torch.empty(T, self._lora_ops["rp"], dtype=torch.bfloat16, device=dev),
                      Xc=torch.zeros(T, self._lora_ops["Kc"], dtype=torch.bfloat16, device=dev))      # columns past d + Rp stay zero
            self._lora_branch_scratch = sc
        return sc

    def _lora_stream(self, call_id, i, ti):
        """dropout stream of target ti in layer i of forward call call_id: peft gives every wrapped Linear its own dropout module, so q, k and v
        see independent masks of the same input"""
        return self._rng_stream(self.RNG_DOMAIN_LORA, (call_id * self.n_layers + i) * 4 + ti)

    def _lora_branch_operand(self, i, h, T, call_id):
        """A operand of layer i's QKV GEMM in the two-branch form: [h | dropout_q(h) A_q^T | dropout_k(h) A_k^T | dropout_v(h) A_v^T | 0] bf16
        [T, Kc]; also returns u = the adapter columns [T, Rp] (kept for the backward; the dropped inputs are regenerated there)."""
        ops, d = self._lora_ops, self.d
        rp, Rp = ops["rp"], ops["Rp"]
        sc = self._lora_scratch_for(T, h.device)
        u = torch.empty(T, Rp, dtype=torch.bfloat16, device=h.device)
        for ti in range(len(self._lora["targets"])):
            hip.call("oneprot_dropout_bf16", h, sc["hd"], T * d, float(self._lora["dropout"]), self._lora_seed, self._lora_stream(call_id, i, ti))
            hip.gemm_nt(sc["hd"], ops["Acat"][i, ti * rp:(ti + 1) * rp], T, rp, d, hip.EPI_BF16, sc["ut"])
            u[:, ti * rp:(ti + 1) * rp].copy_(sc["ut"])
        Xc = sc["Xc"]
        Xc[:, :d].copy_(h.view(T, d))
        Xc[:, d:d + Rp].copy_(u)
        return Xc, u

    def _lora_branch_backward(self, i, h, u, dqkv, T, call_id, ws_tn, raw, dh16=None, dh32=None):
        """adapter gradients of layer i into raw = (dA_raw [n, Rp, d], dB_raw [n, 3d, Rp]) and the branches' share of the layer-input gradient,
        sum_t mask_t * (du_t A_t) / keep, added into dh16 (bf16) or dh32 (fp32)."""
        ops, d = self._lora_ops, self.d
        rp, Rp, dev = ops["rp"], ops["Rp"], dqkv.device
        p_ = float(self._lora["dropout"])
        sc = self._lora_scratch_for(T, dev)
        du = torch.empty(T, Rp, dtype=torch.bfloat16, device=dev)
        hip.gemm_nt(dqkv, ops["BsT"][i], T, Rp, 3 * d, hip.EPI_BF16, du)
        hip.gemm_tn(dqkv, u, T, 3 * d, Rp, raw[1][i], None, ws_tn)            # dqkv^T u
        dhd = torch.empty(T, d, dtype=torch.bfloat16, device=dev)
        dut = sc["ut"]
        for ti in range(len(self._lora["targets"])):
            stream_id = self._lora_stream(call_id, i, ti)
            dut.copy_(du[:, ti * rp:(ti + 1) * rp])
            hip.call("oneprot_dropout_bf16", h, sc["hd"], T * d, p_, self._lora_seed, stream_id)                                  # the forward's dropout_t(h) again
            hip.gemm_tn(dut, sc["hd"], T, rp, d, raw[0][i, ti * rp:(ti + 1) * rp], None, ws_tn)      # du_t^T dropout_t(h)
            hip.gemm_nt(dut, ops["AtT"][i, ti], T, d, rp, hip.EPI_BF16, dhd)
            if dh16 is not None:
                hip.call("oneprot_dropout_bwd_add_bf16", dhd, dh16, T * d, p_, self._lora_seed, stream_id)
            else:
                hip.call("oneprot_dropout_bwd_add_f32", dhd, dh32, T * d, p_, self._lora_seed, stream_id)

    def _lora_raw_buffers(self, dev):
        ops = self._lora_ops
        return (torch.zeros(self.n_layers, ops["Rp"], self.d, device=dev), torch.zeros(self.n_layers, 3 * self.d, ops["Rp"], device=dev))
