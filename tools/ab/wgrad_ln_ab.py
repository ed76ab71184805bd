#!/usr/bin/env python3
"""Development tool (GPU): the CUs to give the LayerNorm role of oneprot_gemm_tn_ln_bwd (csrc/gemm_tn.hip), per weight-gradient shape of the cfg-2 step.
Every timed launch runs behind n dense bf16 GEMM launches (the mechanism of in_step_probe.py: the chip then sits at the clock a sustained MFMA stream leaves it,
burst clocks mislead).  Per shape: the two separate launches (weight gradient on all CUs, then LayerNorm backward), and per R the fused launch, the weight
gradient alone on the CUs the fused launch leaves it (oneprot_cu_reserve = R: the same token splits), and the LayerNorm role alone (the fused launch with a
256-column weight gradient: a tenth of the matrix work, over long before the rows are) -- so that a loss names its owner.
usage: wgrad_ln_ab.py [iters] [gemms in front]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from oneprot_amd import hip
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_front = int(sys.argv[2]) if len(sys.argv) > 2 else 4
T, d, f = 256 * 512, 640, 2560
g = torch.Generator(device="cuda").manual_seed(0)
rb = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
A, W = rb(T, f), rb(d, f)
o0 = torch.empty(T, d, dtype=torch.bfloat16, device="cuda")
front = lambda: hip.call("oneprot_gemm_bf16_nt", A, W, T, d, f, f, f, hip.EPI_BF16, None, o0, None, None, None, None, None, 1.0, 0, 0, 0)
X, dy = rb(T, d), rb(T, d)
x = torch.randn(T, d, device="cuda", generator=g)
gamma, mean, rstd = torch.ones(d, device="cuda"), torch.zeros(T, device="cuda"), torch.ones(T, device="cuda")
gacc, g16 = torch.zeros(T, d, device="cuda"), torch.empty(T, d, dtype=torch.bfloat16, device="cuda")
dg, db = torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
ws_ln = torch.empty(hip.query("oneprot_layernorm_bwd_workspace", d), dtype=torch.uint8, device="cuda")


def timed(fn):
    fn(); torch.cuda.synchronize()
    tot = 0.0
    for _ in range(iters):
        for _ in range(n_front):
            front()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        tot += e0.elapsed_time(e1)
    return tot / iters * 1e3


print(f"us per launch, mean of {iters}, each behind {n_front} dgrad GEMMs (K = 2560); T = {T}, d = {d}")
for name, N in (("FFN-1 [2560, 640]", 2560), ("QKV [1920, 640]", 1920)):
    dY = A if N == f else rb(T, N)
    dW, dbias = torch.empty(N, d, device="cuda"), torch.empty(N, device="cuda")
    dWs, dbs = torch.empty(256, d, device="cuda"), torch.empty(256, device="cuda")
    ws = torch.empty(max(hip.query("oneprot_gemm_bf16_tn_workspace", N, d), hip.query("oneprot_gemm_bf16_tn_workspace", 256, d)), dtype=torch.uint8, device="cuda")
    tn = lambda: hip.gemm_tn(dY, X, T, N, d, dW, dbias, ws)
    ln = lambda: hip.layernorm_bwd(dy, 0, x, gamma, mean, rstd, gacc, dg, db, ws_ln, T, d, add_to=gacc, dx16=g16)
    fused = lambda R: hip.gemm_tn_ln_bwd(dY, X, T, N, d, dW, dbias, ws, dy, x, gamma, mean, rstd, gacc, dg, db, ws_ln, R, add_to=gacc, dx16=g16)
    rows_only = lambda R: hip.call("oneprot_gemm_tn_ln_bwd", dY, X, T, 256, d, N, d, dWs, dbs, ws, ws.numel(), 0, dy, x, gamma, mean, rstd, gacc, gacc, g16, dg, db,
                                   ws_ln.view(torch.float32), 0, R)
    hip.query("oneprot_cu_reserve", 0)
    t_tn, t_ln, t_pair = timed(tn), timed(ln), timed(lambda: (tn(), ln()))
    print(f"{name}: weight gradient {t_tn:6.1f} | LayerNorm backward {t_ln:6.1f} | the two launches {t_pair:6.1f}", flush=True)
    for R in (32, 48, 56, 64, 80):
        t_f = timed(lambda: fused(R))
        hip.query("oneprot_cu_reserve", R)
        t_m = timed(tn)
        hip.query("oneprot_cu_reserve", 0)
        t_r = timed(lambda: rows_only(R))
        print(f"   R {R:3d}: fused {t_f:6.1f} ({t_f - t_pair:+6.1f}) | matrix role alone {t_m:6.1f} | row role alone {t_r:6.1f}", flush=True)
