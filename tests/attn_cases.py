"""Inputs, launches and gates the attention test files share (tests/test_attention_production_gpu.py, tests/test_attention_dropout_gpu.py)."""
import torch

from oneprot_amd import hip
from tests.cases import DEV, bf, gen, randn

CTX_GATE, LSE_GATE = (2 ** -7, 1e-2), (1e-4, 5e-3)                  # test_kernels_gpu.py test_attention_fwd_bwd
CTX_GATE_X, LSE_GATE_X = (2 ** -6, 1.5e-2), (2e-4, 2e-2)            # ... test_attention_fwd_nomax_overflow_underflow_net


def run_fwd(q, k, v, bias):
    B, H, L, hd = q.shape
    ctx = torch.full((B * L, H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)      # an unwritten row shows
    lse = torch.full((B, H, L), float("nan"), device=DEV)
    hip.call("oneprot_attn_fwd", q, k, v, bias, ctx, lse, B, H, L, hd)
    return ctx, lse


def extreme_rows(q, k, slabs, g):
    """the construction of test_attention_fwd_nomax_overflow_underflow_net in the flat slabs `slabs` of q / k [B, H, L, hd] (in place): keys 4 u + noise,
    query row i = alpha_i u + noise, so row i's scores sit near one of -400, -200, 0, 45, 70, 200, 400 (log2 units).  Returns bool [B, H]."""
    B, H, L, hd = q.shape
    u = torch.randn(hd, generator=g, device=DEV)
    u = u / u.norm()
    kinds = torch.tensor([-400.0, -200.0, 0.0, 45.0, 70.0, 200.0, 400.0], device=DEV)
    n = len(slabs)
    alpha = kinds[torch.randint(0, len(kinds), (n, L), generator=g, device=DEV)] / 4.0               # k ~ 4 u, so q = alpha u gives q.k ~ 4 alpha = the kind
    idx = torch.tensor(slabs, device=DEV)
    q.view(B * H, L, hd)[idx] = bf(alpha[..., None] * u + 0.3 * torch.randn(n, L, hd, generator=g, device=DEV))
    k.view(B * H, L, hd)[idx] = bf(u * 4.0 + 0.05 * torch.randn(n, L, hd, generator=g, device=DEV))
    sc = q.view(B * H, L, hd)[idx].float() @ k.view(B * H, L, hd)[idx].float().transpose(-1, -2)
    assert float(sc.max()) > 300 and float(sc.min()) < -300
    is_x = torch.zeros(B * H, dtype=torch.bool, device=DEV)
    is_x[idx] = True
    return is_x.view(B, H)


def fwd_inputs(B, H, L, hd, seed):
    g = gen(seed)
    q = randn((B, H, L, hd), g, 0.7 * hip.LOG2E, dtype=torch.bfloat16)      # the kernels take q x log2(e) (scores in log2 units)
    k = randn((B, H, L, hd), g, 1.0, dtype=torch.bfloat16)
    v = randn((B, H, L, hd), g, 1.0, dtype=torch.bfloat16)
    return q, k, v
