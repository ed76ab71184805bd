"""The parameter arena every tower is built on: all parameters of an encoder in ONE fp32 tensor (`flat`, the only nn.Parameter) in the
order the kernels consume them, named tensors as views into it; a bf16 mirror (GEMM operands) plus transposed bf16 weight copies for the dgrad GEMMs, refreshed
when the arena's version counter changes (an optimizer step, a checkpoint load); the counter-based dropout streams are rng.py's.  Adapters are lora.py's (`LoraArena`)."""
import json
import os
import warnings
from collections import OrderedDict

import torch
import torch.nn as nn

from . import hip, rng


class ModelConfig:
    """Minimal stand-in for transformers.PretrainedConfig (attribute access + to_dict)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to_dict(self):
        return dict(self.__dict__)

    def __repr__(self):
        return f"ModelConfig({self.__dict__})"


def load_weight_file(path):
    """Tensors of a HF-style checkpoint directory (model.safetensors or pytorch_model.bin), or None."""
    if path is None:
        return None
    st = os.path.join(path, "model.safetensors")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        return load_file(st)
    pt = os.path.join(path, "pytorch_model.bin")
    if os.path.isfile(pt):
        return torch.load(pt, map_location="cpu", weights_only=True)
    return None


def _pad8(n):
    return (n + 7) // 8 * 8


class _Out:
    def __init__(self, last_hidden_state):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = None

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output)[i]


class ArenaModule(rng.StreamOwner, nn.Module):
    """Parameters of a whole encoder in one fp32 arena (`flat`) with named views, a bf16 mirror for the MFMA GEMMs, and
    state-dict hooks that expose / accept the HF key names."""

    RNG_DOMAIN_BERT, RNG_DOMAIN_LORA, RNG_DOMAIN_MSA = rng.DOMAINS["bert"], rng.DOMAINS["lora"], rng.DOMAINS["msa"]
    _lora = None              # no adapter (lora.LoraArena.enable_lora sets one); read on any tower by encoders.py and module.py

    def _init_arena(self):
        self._spec = OrderedDict()
        self._cursor = 0
        self._extra = OrderedDict()
        self._init_streams()

    def _finish_arena(self):
        self._total = self._cursor
        self.flat = nn.Parameter(torch.zeros(self._total))
        self.extra = nn.ParameterDict({k.replace(".", "__"): nn.Parameter(torch.zeros(s)) for k, s in self._extra.items()})
        self._register_state_dict_hook(self._sd_hook)
        self._register_load_state_dict_pre_hook(self._load_hook)
        self._bf16 = None
        self._bf16_T = {}
        self._bf16_version = None

    _norm_weight_suffixes = ("LayerNorm.weight",)      # the arena tensors reset_parameters fills with ones

    @torch.no_grad()
    def reset_parameters(self):
        """norm weights 1, biases 0, everything else normal(0, std) in arena order; returns std = config.initializer_range (0.02 where there is none)"""
        std = getattr(self.config, "initializer_range", 0.02)
        for name in self._spec:
            v = self.view(name)
            if name.endswith(self._norm_weight_suffixes):
                v.fill_(1.0)
            elif name.endswith(".bias"):
                v.zero_()
            else:
                v.normal_(0.0, std)
        return std

    def _transpose_layer_weights(self, key, name, R, C):
        """self._bf16_T[(i, key)] = bf16 [C, R] transposed copy of the fp32 [R, C] arena block that starts at tensor name.format(i=i), for
        every layer i, in ONE launch (the layers sit at a constant arena pitch); the copies are views of one [n_layers, C, R] buffer."""
        offs = [self._spec[name.format(i=i)][0] for i in range(self.n_layers)]
        pitch = offs[1] - offs[0] if self.n_layers > 1 else 0
        buf = self._bf16_T.get(("all", key))
        if buf is None:
            buf = self._bf16_T[("all", key)] = torch.empty(self.n_layers, C, R, dtype=torch.bfloat16, device=self.flat.device)
            for i in range(self.n_layers):
                self._bf16_T[(i, key)] = buf[i]
        w = self.flat.data
        if pitch >= 0 and all(o == offs[0] + i * pitch for i, o in enumerate(offs)):
            hip.call("oneprot_transpose_cast_f32_to_bf16_batched", w[offs[0]:], buf, R, C, pitch, R * C, self.n_layers)
        else:
            for i, o in enumerate(offs):
                hip.call("oneprot_transpose_cast_f32_to_bf16", w[o:o + R * C], buf[i], R, C)

    def _add(self, name, shape):
        n = 1
        for s in shape:
            n *= s
        self._spec[name] = (self._cursor, n, tuple(shape))
        self._cursor += _pad8(n)

    def view(self, name, src=None):
        off, n, shape = self._spec[name]
        src = self.flat if src is None else src
        if isinstance(src, nn.Parameter):
            src = src.data
        return src[off:off + n].view(shape)

    def span(self, first, last):
        """contiguous arena range covering tensors first..last (used for the fused QKV operand)"""
        o0 = self._spec[first][0]
        o1, n1, _ = self._spec[last]
        return o0, o1 + n1 - o0

    def named_views(self):
        return OrderedDict((k, self.view(k)) for k in self._spec)

    def _w16(self, name):
        return self.view(name, self._bf16)

    _key_prefix = ""          # what the emitted state-dict keys carry in front of the checkpoint's own names (lora.py: peft's wrapper prefix)
    _sd_extra_buffers = ()
    _load_ignore_suffixes = ()

    def _sd_hook(self, module, state_dict, prefix, local_metadata):
        flat = state_dict.pop(prefix + "flat")
        base = prefix + self._key_prefix
        for name in self._spec:
            state_dict[base + name] = self.view(name, flat)
        for k in list(self._extra):
            state_dict[base + k] = state_dict.pop(prefix + "extra." + k.replace(".", "__"))
        for key, fn in self._sd_extra_buffers:
            state_dict[base + key] = fn(self)
        return state_dict

    def _load_hook(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        peft = prefix + "base_model.model."
        for k in [k for k in state_dict if k.startswith(peft)]:          # a PeftModel's keys load into either form
            state_dict[prefix + k[len(peft):]] = state_dict.pop(k)
        flat = self.flat.detach().clone()
        for name, (off, n, shape) in self._spec.items():
            key = prefix + name
            if key in state_dict:
                t = state_dict.pop(key)
                if tuple(t.shape) != shape:
                    error_msgs.append(f"size mismatch for {key}: checkpoint {tuple(t.shape)} vs model {shape}")
                    continue
                flat[off:off + n] = t.reshape(-1).to(flat)
            elif prefix + "flat" not in state_dict:
                missing_keys.append(key)
        if prefix + "flat" not in state_dict:
            state_dict[prefix + "flat"] = flat
        for k in self._extra:
            key = prefix + k
            if key in state_dict:
                state_dict[prefix + "extra." + k.replace(".", "__")] = state_dict.pop(key)
        for key in [k for k in state_dict if k.startswith(prefix) and k.endswith(tuple(self._load_ignore_suffixes))] if self._load_ignore_suffixes else []:
            state_dict.pop(key)

    def _refresh_bf16_mirror(self, also=()):
        """returns True when the mirror was rebuilt: the arena changed, or what a subclass derives further operands from (`also`) did"""
        ver = (self.flat._version, self.flat.data_ptr()) + also
        if self._bf16_version == ver:
            return False
        dev = self.flat.device
        if self._bf16 is None or self._bf16.device != dev or self._bf16.numel() != self._total:
            self._bf16 = torch.empty(self._total, dtype=torch.bfloat16, device=dev)
            self._bf16_T = {}
        hip.call("oneprot_cast_f32_to_bf16", self.flat.data, self._bf16, self._total)
        self._bf16_version = ver
        return True

    @staticmethod
    def _tn_workspace(shapes, dev):
        """one workspace large enough for every (N, K) weight gradient of a backward pass (the split count, hence the slab size, differs per shape)"""
        return torch.empty(max(hip.query("oneprot_gemm_bf16_tn_workspace", N, K) for N, K in shapes), dtype=torch.uint8, device=dev)

    @classmethod
    def _from_checkpoint(cls, sd, name, expected, tolerated, *args, **kw):
        """The shared end of every from_pretrained: (cls(*args, **kw) with the tensors `sd` loaded, its missing keys outside the `tolerated` prefixes, the
        unexpected keys).  sd None (no weight file; `expected` names what was looked for): refused unless ONEPROT_ALLOW_RANDOM_INIT=1, then random weights."""
        if sd is None:
            if os.environ.get("ONEPROT_ALLOW_RANDOM_INIT", "0") != "1":
                raise OSError(f"no weights ({expected}) found for {name}; "
                              "set ONEPROT_ALLOW_RANDOM_INIT=1 to build a randomly initialised model of that architecture")
            warnings.warn(f"{name}: no weight file, using random initialisation")
        model = cls(*args, **kw)
        missing, unexpected = model.load_state_dict(sd, strict=False) if sd is not None else ([], [])
        return model, [m for m in missing if not m.startswith(tolerated)], unexpected

    def save_pretrained(self, path):
        """HF-style directory (config.json + model.safetensors) -- used by ref peft_checkpoint.py:20."""
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump({k: v for k, v in self.config.to_dict().items() if isinstance(v, (int, float, str, bool, type(None), list))}, f, indent=1)
        sd = {k: v.detach().cpu().contiguous().clone() for k, v in self.state_dict().items()}
        save_file(sd, os.path.join(path, "model.safetensors"))
