"""The small builders the GPU tests share: dtype shorthands, device generators and workspaces, packed-stream shapes with their rotary tables, and the
ESM checkpoint directories the towers load from."""
import functools
import gc
import json
import os

import torch

DEV = "cuda"
NAN = float("nan")
SEED_HI, STREAM_HI = (0x5EED << 32) | 0x1234ABCD, (0x3 << 60) | (0x2A << 32) | 0x91      # non-zero high words: both halves of the Philox key / counter


def bf(x):
    return x.to(torch.bfloat16)


def f64(x):
    return x.detach().cpu().double()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(shape, g, scale=1.0, shift=0.0, dtype=torch.float32):
    return (torch.randn(shape, generator=g, device=DEV) * scale + shift).to(dtype)


def free():
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ packed streams
def cu(lengths):
    c = [0]
    for n in lengths:
        c.append(c[-1] + n)
    return c


def pack_shape(lengths, pad_id=1):
    """(PackedTokens on the device, its padded stream length -- the sum rounded up to 256 --, the segment starts)"""
    from oneprot_amd.packing import PackedTokens
    p = PackedTokens.from_list([torch.full((n,), 5, dtype=torch.int64) for n in lengths], pad_id=pad_id).to(DEV)
    return p, p.T_pad, cu(lengths)


def rope_half(L, hd):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    f = torch.outer(torch.arange(L, dtype=torch.float32), inv)
    return f.cos(), f.sin()


def gathered_tables(lengths, T, hd):
    """[T, hd/2] rotary tables per token (position within its segment; tail: position 0)"""
    cos, sin = rope_half(max(lengths), hd)
    pos = torch.zeros(T, dtype=torch.long)
    for a, n in zip(cu(lengths)[:-1], lengths):
        pos[a:a + n] = torch.arange(n)
    return cos[pos].contiguous(), sin[pos].contiguous()


# ------------------------------------------------------------------------------------------------------------------ checkpoint directories
def esm_dir(tmp, name, layers, hidden, heads, ffn):
    path = os.path.join(str(tmp), name)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="esm", vocab_size=33, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=ffn), f)
    return path


def esm_dir_from_cfg(tmp, cfg, name="esm"):
    """the directory of a golden's `cfg` (tests/golden/esm_pair_*.pt)"""
    path = os.path.join(tmp, name)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="esm", vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"],
                       num_attention_heads=cfg["heads"], intermediate_size=cfg["ffn"], pad_token_id=cfg["pad"], mask_token_id=cfg["mask"],
                       layer_norm_eps=cfg["eps"], token_dropout=True, position_embedding_type="rotary", emb_layer_norm_before=False), f)
    return path


def golden_pair_module(golden_dir, tag, tmp_path, frozen_seq=False):
    """(the golden tests/golden/esm_pair_<tag>.pt, the sequence / struct_token module built from its config and loaded with its weights)"""
    os.environ.update(RANK="0", WORLD_SIZE="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.struct_token_encoder import StructTokenEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    g = torch.load(os.path.join(golden_dir, f"esm_pair_{tag}.pt"), weights_only=False)
    cfg = g["cfg"]
    p = esm_dir_from_cfg(str(tmp_path), cfg)
    seq = SequenceEncoder(p, output_dim=cfg["output_dim"], pooling_type="mean", proj_type="mlp", use_lora=False, frozen=frozen_seq)
    st = StructTokenEncoder(p, output_dim=cfg["output_dim"], pooling_type="mean", proj_type="linear", use_logit_scale=True, learnable_logit_scale=False)
    seq.load_state_dict(g["sd_seq"], strict=True)        # exact key compatibility with the reference's state dict
    st.load_state_dict(g["sd_st"], strict=True)
    module = OneProtLitModule(components={"sequence": seq, "struct_token": st}, optimizer=functools.partial(FusedAdam, lr=1e-3, weight_decay=0.0),
                              loss_fn="CLIP", use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(DEV)
    return g, module
