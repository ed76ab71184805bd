"""What the MSA test files share: the 2-layer model and its fair-esm checkpoint file, token and id builders, bf16-rounded qkv, the row / column kernel
launches and the case lists that more than one file walks."""
import argparse
import math
import os

import torch

DEV = torch.device("cuda:0")
F64 = torch.float64


def _ids(B, R, L, lens, rows, holes=()):
    """token-like ids [B, R, L]: 5 = token, 1 = pad; MSA b has lens[b] columns and rows[b] rows; holes: (b, r, l) single pads"""
    ids = torch.full((B, R, L), 5, dtype=torch.int64)
    for b in range(B):
        ids[b, :, lens[b]:] = 1
        ids[b, rows[b]:] = 1
    for b, r, l in holes:
        ids[b, r, l] = 1
    return ids


def _qkv(B, R, L, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * R * L, 3 * H * 64, generator=g).to(torch.bfloat16)


def _split(qkv, B, R, L, H):
    q, k, v = qkv.to(F64).view(B, R, L, 3, H * 64).unbind(3)
    return q, k, v


def _key_bias(ids):
    from oneprot_amd import hip
    kb = torch.empty(ids.numel(), dtype=torch.float32, device=DEV)
    hip.call("oneprot_key_padding_bias", ids.to(DEV), kb, ids.numel(), 1)
    return kb


def _row(qkv, ids, H):
    from oneprot_amd import hip
    B, R, L = ids.shape
    kb, qd = _key_bias(ids), qkv.to(DEV)
    S = torch.empty(B, H, L, L, dtype=torch.float32, device=DEV)
    ctx = torch.empty(B * R * L, H * 64, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_msa_row_scores", qd, kb, S, B, R, L, H, 64, 64 ** -0.5 / math.sqrt(R))
    ws = torch.empty(hip.query("oneprot_msa_row_context_workspace", B, R, L, H), dtype=torch.uint8, device=DEV)
    hip.call("oneprot_msa_row_context", S, qd, kb, ctx, ws, ws.numel(), B, R, L, H, 64)
    torch.cuda.synchronize()
    return S, ctx


def _col(qkv, ids, H):
    from oneprot_amd import hip
    B, R, L = ids.shape
    ctx = torch.empty(B * R * L, H * 64, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_msa_col_attn", qkv.to(DEV), _key_bias(ids), ctx, B, R, L, H, 64, 64 ** -0.5)
    torch.cuda.synchronize()
    return ctx


# (B, R, L, H), lens, rows, holes: the smallest shapes that cross every tile edge in L (16 / 32 / 64), take an odd trip count in R and reach L = 1024
ROW_CASES = [
    ((1, 1, 5, 1), [5], [1], ()),
    ((2, 3, 33, 2), [33, 20], [3, 2], ((0, 2, 7),)),                    # interior pad at (r = 2, i = 7) with row 0 not padded there: the q zeroing
    ((1, 50, 70, 2), [70], [50], ((0, 0, 66), (0, 0, 67), (0, 0, 68), (0, 0, 69))),      # row 0 shorter than the other rows: the key mask is row 0's
    ((2, 5, 130, 1), [130, 97], [5, 3], ()),
    ((1, 2, 257, 1), [250], [2], ()),
    ((1, 4, 1024, 1), [1000], [3], ()),
]


# ---------------------------------------------------------------------------------------------------------------- tower / encoder
ARCH = dict(layers=2, embed_dim=128, ffn_embed_dim=256, attention_heads=2, max_positions=160, embed_positions_msa=True)


def _checkpoint(tmp_path, seed=0, arch=ARCH, name="msa_tiny.pt", std=0.08):
    """a random model (by default the 2-layer ARCH) written as a fair-esm file (encoder.-prefixed keys, row / column swapped), so that the encoder is built
    through the loader"""
    from oneprot_amd.msa import MsaTransformer, config_from_args
    path = os.path.join(str(tmp_path), name)
    if not os.path.exists(path):
        torch.manual_seed(seed)
        tr = MsaTransformer(config_from_args(arch))
        with torch.no_grad():
            tr.flat.normal_(0.0, std)
            for k in tr._spec:
                if k.endswith("layer_norm.weight") or k.startswith("emb_layer_norm") and k.endswith("weight"):
                    tr.view(k).add_(1.0)
        sw = lambda k: k.replace("row", "\0").replace("column", "row").replace("\0", "column")
        torch.save({"args": argparse.Namespace(arch="msa_transformer", **arch), "model": {"encoder." + sw(k): v.clone() for k, v in tr.state_dict().items()}}, path)
    return path


def _tokens(B, R, L, lens, rows, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(4, 30, (B, R, L), generator=g)
    t[:, :, 0] = 0
    for b in range(B):
        t[b, :, lens[b]:] = 1
        t[b, rows[b]:] = 1
    return t


E2E = [((2, 5, 70), [70, 44], [5, 3]), ((1, 1, 40), [33], [1])]


def _tower(arch=ARCH):
    from oneprot_amd.msa import MsaTransformer, config_from_args
    return MsaTransformer(config_from_args(arch))


def _write_fair_esm_file(path, tr):
    sw = lambda k: k.replace("row", "\0").replace("column", "row").replace("\0", "column")
    torch.save({"args": argparse.Namespace(arch="msa_transformer", **ARCH), "model": {"encoder." + sw(k): v.clone() for k, v in tr.state_dict().items()}}, path)


def bf(t):
    return t.to(torch.bfloat16).to(F64)


GROUPED = ((3, 4, 50), [50, 31, 45], [2, 4, 3], 23)                     # _tokens arguments of test_tower_stages_one_msa_per_group
FFN_SELF_DIFFERENCE_GROUPED = 9.44e-3                                   # recomputed by tests/test_msa_cpu.py::test_ffn_gate_of_the_grouped_stage_test_is_the_measured_one
