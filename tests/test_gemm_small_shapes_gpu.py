"""The GEMM family at the shapes around the big contractions: LoRA's adapter launches (N or K of 8 .. 48), leading dimensions that differ from the
logical width, the fp32 sgemm over its K-slice loop and at the production calls, one layer's two-branch adapter chain stage by stage, and the
QKV/RoPE epilogue for sequences shorter than one 8-row epilogue pass.

References are fp64 torch on the CPU from the same bf16-rounded inputs (fp32 inputs for sgemm), computed once per case and shared by the
block shapes / variants that run it.  Every output starts as NaN, so an element that is never written fails its comparison (the comparisons
are written so that NaN fails).  Strided operands are column slices of wider matrices that are NaN outside the slice and have 64 NaN rows
behind them: a read outside the slice shows as NaN in the result and stays inside the allocation.

Tolerances are those of test_kernels_gpu.py (test_gemm_nt_epilogues, test_gemm_tn, test_gemm_qkv_rope_epilogue), K and M scaling unchanged:
bf16 outputs rtol 2^-7 / atol 2e-2, fp32 outputs rtol 1e-4 / atol 1e-3 sqrt(K / 64), weight gradients rtol 1e-4 / atol 2e-3 sqrt(M / 64).
sgemm is an fp32 fmaf chain and gets the dot-product bound |C - ref| <= (K + 2) u (|alpha| |A| |B| + |C_in|), u = 2^-24 (K roundings of the
chain, one of alpha * acc, one of the add to C; holds for any summation order)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oneprot_amd import hip  # noqa: E402
from oracle import oneprot_oracle as O  # noqa: E402
from tests import gemm_forms  # noqa: E402
from tests.cases import bf, esm_dir, f64, nans  # noqa: E402
from tests.gate import close  # noqa: E402
from tests.philox_ref import dropout_threshold, philox_keep  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF = torch.bfloat16
GUARD_ROWS = 64


def tol_f32(K):
    return 1e-4, 1e-3 * math.sqrt(K / 64)


def tol_tn(M):
    return 1e-4, 2e-3 * math.sqrt(M / 64)


TOL_BF16 = (2 ** -7, 2e-2)


# all 17 forced block shapes / all 5 weight-gradient variants (the lists test_kernels_gpu.py uses: tests/gemm_forms.py)
@pytest.fixture(params=gemm_forms.ids(gemm_forms.NT_SHAPES), ids=gemm_forms.names(gemm_forms.NT_SHAPES))
def gemm_shape(request):
    hip.query("oneprot_gemm_force_shape", request.param)
    yield request.param
    hip.query("oneprot_gemm_force_shape", -1)


@pytest.fixture(params=gemm_forms.ids(gemm_forms.TN_VARIANTS), ids=gemm_forms.names(gemm_forms.TN_VARIANTS))
def tn_variant(request):
    hip.query("oneprot_gemm_tn_variant", request.param)
    yield request.param
    hip.query("oneprot_gemm_tn_variant", -1)


def gemm_nt(A, W, M, N, K, lda, ldb, epi, bias, out0, out1=None, out2=None, aux=None, cos=None, sin=None, q_scale=1.0, L=0, H=0, hd=0):
    hip.call("oneprot_gemm_bf16_nt", A, W, M, N, K, lda, ldb, epi, bias, out0, out1, out2, aux, cos, sin, q_scale, L, H, hd)


def strided(X, ld, off=0):
    """X [R, C] (CPU) as columns [off, off + C) of a NaN matrix [R + GUARD_ROWS, ld] on the device.  Returns the operand to hand to the C ABI with
    leading dimension ld: the wide tensor itself, or (column offset) the flat arena from element `off` on -- both contiguous."""
    R, C = X.shape
    assert off % 8 == 0 and off + C <= ld
    arena = torch.full((R + GUARD_ROWS, ld), NAN, dtype=X.dtype)
    arena[:R, off:off + C] = X
    arena = arena.to(DEV)
    return arena if off == 0 else arena.view(-1)[off:]


# ====================================================================================================== 1. NT GEMM, narrow N and thin K
@functools.lru_cache(maxsize=None)
def _nt_case(M, N, K, seed=3):
    g = torch.Generator().manual_seed(seed + 7 * N + K)
    A = bf(torch.randn(M, K, generator=g))
    W = bf(torch.randn(N, K, generator=g) * (1.0 if K <= 24 else 0.1))      # thin K: one dropped product is far above the tolerance
    bias = torch.randn(N, generator=g) * 0.5
    resid = torch.randn(M, N, generator=g)
    ref = A.double() @ W.double().t()
    return A, W, bias, resid, ref


# the down-projection u (N = rp), du (N = Rp), dh (K = rp) of LoRA's two-branch form; (136, 24): K below one 32-wide MFMA step and no multiple of 16
NARROW_NT = [(8, 320), (8, 640), (16, 1280), (24, 1920), (48, 960), (320, 8), (640, 8), (1280, 16), (136, 24)]


@pytest.mark.parametrize("N,K", NARROW_NT)
@pytest.mark.parametrize("M", [300, 2304])      # a partial row tile in every block shape; >= 2048 rows: `auto` takes the heuristic's branches, not shape 0
def test_gemm_nt_narrow(M, N, K, gemm_shape):
    A, W, bias, _, ref = _nt_case(M, N, K)
    Ad, Wd, bd = A.to(DEV), W.to(DEV), bias.to(DEV)
    out = nans(M, N, dtype=BF)
    gemm_nt(Ad, Wd, M, N, K, K, K, hip.EPI_BF16, None, out)                  # as the host calls it: no bias
    close(out, ref, *TOL_BF16, "EPI_BF16")
    outf = nans(M, N)
    gemm_nt(Ad, Wd, M, N, K, K, K, hip.EPI_F32, bd, outf)                    # the bias read at the gn < N edge
    close(outf, ref + bias.double(), *tol_f32(K), "EPI_F32 + bias")


# ====================================================================================================== 2. NT GEMM with strides
#              M     N     K    lda   ldb  column offset of A
STRIDED_NT = [(300, 136, 72, 80, 136, 0),
              (1024, 640, 640, 704, 1280, 0),       # whole tiles, lda % 64 == 0: the ping-pong, register-staged and 8-phase forms take it
              (1024, 640, 640, 648, 648, 0),        # forms that need lda % 64 == 0 decline it: the fallback must be right
              (256, 320, 128, 192, 136, 0),
              (512, 512, 128, 192, 136, 0),         # whole 256 x 256 tiles: the register-staged and the 256 x 256 8-phase and direct-store forms, with strides
              (2304, 1920, 640, 1280, 640, 640)]


@pytest.mark.parametrize("M,N,K,lda,ldb,off", STRIDED_NT)
def test_gemm_nt_strided(M, N, K, lda, ldb, off, gemm_shape):
    A, W, bias, resid, ref = _nt_case(M, N, K, seed=4)
    As, Ws, bd = strided(A, lda, off), strided(W, ldb), bias.to(DEV)
    out = nans(M, N, dtype=BF)
    gemm_nt(As, Ws, M, N, K, lda, ldb, hip.EPI_BF16, bd, out)
    close(out, ref + bias.double(), *TOL_BF16, "EPI_BF16, strided")
    x = resid.to(DEV, copy=True)
    gemm_nt(As, Ws, M, N, K, lda, ldb, hip.EPI_BIAS_RESID, bd, x, aux=x)      # in place, as the layers run it
    close(x, ref + bias.double() + resid.double(), *tol_f32(K), "EPI_BIAS_RESID in place, strided")


def _ln_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = bf(torch.randn(M, K, generator=g))
    W = bf(torch.randn(N, K, generator=g) * 0.1)
    bias = torch.randn(N, generator=g) * 0.5
    resid = torch.randn(M, N, generator=g) * 2.0 + 0.3
    gamma, beta = 1.0 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    xr = A.double() @ W.double().t() + bias.double() + resid.double()
    mu = xr.mean(-1, keepdim=True)
    var = ((xr - mu) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + 1e-5)
    hr = (xr - mu) * rstd * gamma.double() + beta.double()
    return A, W, bias, resid, gamma, beta, xr, mu[:, 0], rstd[:, 0], hr


def test_gemm_resid_ln_strided():
    """oneprot_gemm_bf16_nt_resid_ln with lda != K: equal bits to the dense call on a contiguous copy, and both against fp64 (tolerances of
    test_gemm_resid_layernorm_fused)"""
    M, N, K, lda = 256, 640, 640, 704
    A, W, bias, resid, gamma, beta, xr, mu, rstd, hr = _ln_case(M, N, K, 41)
    Wd = W.to(DEV)
    Wp = torch.empty(N * K, dtype=BF, device=DEV)
    hip.call("oneprot_gemm_ln_pack_weight", Wd, Wp, N, K)
    bd, rd, gd, btd = bias.to(DEV), resid.to(DEV), gamma.to(DEV), beta.to(DEV)
    outs = []
    for Aop, ld in ((strided(A, lda), lda), (A.to(DEV), K)):
        x, h, mean, rs = nans(M, N), nans(M, N, dtype=BF), nans(M), nans(M)
        hip.call("oneprot_gemm_bf16_nt_resid_ln", Aop, Wp, M, N, K, ld, bd, rd, x, gd, btd, 1e-5, h, mean, rs)
        outs.append((x, h, mean, rs))
    for name, a, b in zip(("x", "h", "mean", "rstd"), *outs):
        assert torch.equal(a, b), f"{name}: strided call differs from the dense call"
    x, h, mean, rs = outs[0]
    close(x, xr, *tol_f32(K), "x = A W^T + bias + resid")
    close(mean, mu, 1e-4, 1e-4 * math.sqrt(K / 64), "mean")
    close(rs, rstd, 1e-3, 1e-5, "rstd")
    close(h, hr, *TOL_BF16, "h = LayerNorm(x)")


def test_gemm_resid_ln8_strided():
    """oneprot_gemm_bf16_nt_resid_ln8 with lda != K and ldb != K: equal bits to the dense call on contiguous copies, and both against fp64
    (tolerances of test_gemm_resid_layernorm_across_work_groups against fp32 torch)"""
    M, N, K, lda, ldb = 768, 320, 128, 192, 136
    assert hip.query("oneprot_gemm_resid_ln8_eligible", M, N, K) != 0
    A, W, bias, resid, gamma, beta, xr, mu, rstd, hr = _ln_case(M, N, K, 42)
    bd, rd, gd, btd = bias.to(DEV), resid.to(DEV), gamma.to(DEV), beta.to(DEV)
    outs = []
    for Aop, Wop, la, lb in ((strided(A, lda), strided(W, ldb), lda, ldb), (A.to(DEV), W.to(DEV), K, K)):
        x, h, st = nans(M, N), nans(M, N, dtype=BF), nans(2, M)
        hip.call("oneprot_gemm_bf16_nt_resid_ln8", Aop, Wop, M, N, K, la, lb, bd, rd, x, gd, btd, 1e-5, h, st, *hip.sched_workspace(M))
        outs.append((x, h, st))
    assert hip.sched_error() == 0
    for name, a, b in zip(("x", "h", "stats"), *outs):
        assert torch.equal(a, b), f"{name}: strided call differs from the dense call"
    x, h, st = outs[0]
    close(x, xr, 2e-5, 3e-4, "x_out")
    close(h, hr, 2 ** -7, 4e-3, "h")
    close(st[0], mu, 1e-5, 1e-4, "mean")
    close(st[1], rstd, 1e-4, 0.0, "rstd")


# ====================================================================================================== 3. TN GEMM, narrow and strided
#            M     N     K    ldy   ldx  column offset of dY
TN_CASES = [(1500, 960, 24, 960, 24, 0), (4096, 1920, 24, 1920, 24, 0), (777, 48, 960, 48, 960, 0),          # dqkv^T u (K = Rp), du_t^T dropout(h) at Rp = 48
            (1500, 8, 320, 8, 320, 0), (4096, 8, 640, 8, 640, 0), (4096, 16, 1280, 16, 1280, 0),             # du_t^T dropout(h): a tile with 8 / 16 live rows
            (300, 136, 72, 144, 80, 0),
            (4096, 640, 640, 1920, 704, 640),      # the k block of a dqkv: whole 128 x 128 tiles and whole stages (the register-staged variant's fast fill)
            (6144, 640, 640, 1920, 704, 640),      # the same with 24 token splits x 6 tiles: enough work items for the 8-phase form (partial last n tile), with strides
            (5000, 1920, 640, 1928, 648, 0)]


@functools.lru_cache(maxsize=None)
def _tn_case(M, N, K):
    g = torch.Generator().manual_seed(6 + N + K)
    dY = bf(torch.randn(M, N, generator=g))
    X = bf(torch.randn(M, K, generator=g))
    return dY, X, dY.double().t() @ X.double(), dY.double().sum(0)


@pytest.mark.parametrize("M,N,K,ldy,ldx,off", TN_CASES)
def test_gemm_tn_narrow_and_strided(M, N, K, ldy, ldx, off, tn_variant):
    dY, X, ref, cs = _tn_case(M, N, K)
    dYs = strided(dY, ldy, off) if (ldy != N or off) else dY.to(DEV)
    Xs = strided(X, ldx) if ldx != K else X.to(DEV)
    need = hip.query("oneprot_gemm_bf16_tn_workspace", N, K)
    guard = 4096
    w = torch.zeros(need + guard, dtype=torch.uint8, device=DEV)
    w[need:] = 0xA5
    rtol, atol = tol_tn(M)
    for with_db in (True, False):
        dW = nans(N, K)
        db = nans(N) if with_db else None
        hip.call("oneprot_gemm_bf16_tn", dYs, Xs, M, N, K, ldy, ldx, dW, db, w, need, 0)
        close(dW, ref, rtol, atol, f"dW, dbias {with_db}")
        first, first_db = f64(dW), (f64(db) if with_db else None)
        if with_db:
            close(db, cs, 1e-4, 1e-2, "fused bias gradient")
        hip.call("oneprot_gemm_bf16_tn", dYs, Xs, M, N, K, ldy, ldx, dW, db, w, need, 1)
        close(dW, first + ref, rtol, atol, f"dW accumulated, dbias {with_db}")
        if with_db:
            close(db, first_db + cs, 1e-4, 1e-2, "bias gradient accumulated")
    assert bool((w[need:] == 0xA5).all()), "wrote past the workspace"


# ====================================================================================================== 4. sgemm
U32 = 2.0 ** -24


def _sgemm_check(M, N, K, tA, bkn, alpha, accumulate, seed=7):
    g = torch.Generator().manual_seed(seed + M + 3 * N + 5 * K)
    A = torch.randn(M, K, generator=g)
    Bm = torch.randn(K, N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    alpha32 = float(np.float32(alpha))                                      # what the C ABI receives
    Ad = (A.t().contiguous() if tA else A).to(DEV)
    Bd = (Bm if bkn else Bm.t().contiguous()).to(DEV)
    C = C0.to(DEV, copy=True) if accumulate else nans(M, N)
    hip.call("oneprot_sgemm", Ad, Bd, C, M, N, K, tA, bkn, alpha, accumulate)
    cin = C0.double() if accumulate else torch.zeros(M, N, dtype=torch.float64)
    ref = alpha32 * (A.double() @ Bm.double()) + cin
    bound = (K + 2) * U32 * (abs(alpha32) * (A.double().abs() @ Bm.double().abs()) + cin.abs())
    close(C, ref, 0.0, bound, f"sgemm {M}x{N}x{K} tA {tA} b_is_kn {bkn} alpha {alpha} accumulate {accumulate}")


LAYOUTS = [(0, 0), (0, 1), (1, 1), (1, 0)]


@pytest.mark.parametrize("tA,bkn", LAYOUTS)
@pytest.mark.parametrize("K", [1, 8, 63, 64, 65, 128, 129, 640])      # one 64-deep slice and its edges, two and three slices (the prefetch under the multiply), ten
def test_sgemm_k_slices(K, tA, bkn):
    for accumulate in (0, 1):
        _sgemm_check(70, 130, K, tA, bkn, 0.5 if accumulate else -1.75, accumulate)


@pytest.mark.parametrize("tA,bkn", LAYOUTS)
@pytest.mark.parametrize("N", [1, 63, 64, 65])
@pytest.mark.parametrize("M", [1, 63, 64, 65])
def test_sgemm_tile_edges(M, N, tA, bkn):
    for accumulate in (0, 1):
        _sgemm_check(M, N, 130, tA, bkn, 0.5 if accumulate else -1.75, accumulate)


@pytest.mark.parametrize("M,N,K,tA,bkn,alpha,accumulate", [
    (256, 1024, 640, 0, 0, 1.0, 0),             # projection head
    (256, 256, 1024, 0, 0, 1 / 0.07, 0),        # logits
    (256, 2048, 1024, 0, 0, 1 / 0.07, 0),       # logits against gathered features
    (1024, 640, 256, 1, 1, 1.0, 0),             # head weight gradient
    (256, 640, 1024, 0, 1, 1.0, 0),             # head input gradient
    (640, 640, 8, 0, 1, 2.0, 1),                # LoRA merge W += s B A
    (640, 8, 640, 0, 0, 1.0, 0),                # dB = s dW A^T
    (8, 640, 640, 1, 1, 1.0, 0),                # dA = s B^T dW
    (1, 1, 262144, 0, 0, 1.0, 0)])              # dot product over a whole weight
def test_sgemm_production_calls(M, N, K, tA, bkn, alpha, accumulate):
    _sgemm_check(M, N, K, tA, bkn, alpha, accumulate, seed=9)


# ====================================================================================================== 5. one layer's adapter branch
@pytest.mark.parametrize("hidden,r", [(320, 4), (320, 12), (640, 8)])      # rp = 8, 16, 8; Kc = 384, 384, 768
def test_lora_two_branch_layer_stage_by_stage(hidden, r, tmp_path, monkeypatch):
    """The chain of esm.py's two-branch LoRA form for one layer -- dropout, down-projection, the K-concatenated QKV operand, du, dB, dA, the masked
    add into dh -- each stage against fp64 from the previous stage's own bf16 output (errors do not compound), masks drawn on the CPU from the
    generator's definition (tests/philox_ref.py)."""
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    from oneprot_amd.encoders import SequenceEncoder
    torch.manual_seed(31)
    d, T, p_, i, call, n_layers = hidden, 576, 0.25, 1, 5, 2
    alpha = 3 * r // 2                                                     # scaling 1.5
    enc = SequenceEncoder(esm_dir(tmp_path, "esm", n_layers, d, 20, 2 * d), output_dim=128, pooling_type="mean", proj_type="linear", use_lora=True, lora_r=r,
                          lora_alpha=alpha, lora_dropout=p_).to(DEV).train()
    tr = enc.transformer
    with torch.no_grad():
        tr.flat.normal_(0, 0.05)
        tr.lora_A.mul_(3.0)
        tr.lora_B.normal_(0, 0.08)
    rp = -(-r // 8) * 8
    Rp, s_ = 3 * rp, alpha / r
    Kc = -(-(d + Rp) // 128) * 128
    assert tr._lora_two_branch()

    # ---- refresh: Wc = [W | s B (block-diagonal over the targets) | 0], Acat = the targets' A stacked (rp rows each), AtT = A_t^T, BsT = (s B_t)^T
    tr._refresh_bf16_mirror()
    tr._lora_refresh_branch_operands()
    ops = tr._lora_ops
    assert (ops["rp"], ops["Rp"], ops["Kc"]) == (rp, Rp, Kc)
    a16, b16 = tr.lora_A.data.cpu().to(BF), (s_ * tr.lora_B.data.cpu()).to(BF)      # [n, 3, r, d], [n, 3, d, r]
    W16 = torch.stack([tr.flat.data[o:o + cnt].view(3 * d, d).cpu().to(BF) for o, cnt in
                       (tr.span(f"encoder.layer.{j}.attention.self.query.weight", f"encoder.layer.{j}.attention.self.value.weight") for j in range(n_layers))])
    Wc = torch.zeros(n_layers, 3 * d, Kc, dtype=BF); Acat = torch.zeros(n_layers, Rp, d, dtype=BF)
    AtT = torch.zeros(n_layers, 3, d, rp, dtype=BF); BsT = torch.zeros(n_layers, Rp, 3 * d, dtype=BF)
    Wc[:, :, :d] = W16
    for ti in range(3):
        Acat[:, ti * rp:ti * rp + r] = a16[:, ti]
        AtT[:, ti, :, :r] = a16[:, ti].transpose(1, 2)
        Wc[:, ti * d:(ti + 1) * d, d + ti * rp:d + ti * rp + r] = b16[:, ti]
        BsT[:, ti * rp:ti * rp + r, ti * d:(ti + 1) * d] = b16[:, ti].transpose(1, 2)
    for name, want in (("Wc", Wc), ("Acat", Acat), ("AtT", AtT), ("BsT", BsT)):
        assert torch.equal(ops[name].cpu(), want), f"{name} after the refresh (padding included)"
    assert float(b16.float().abs().max()) > 0 and float(a16.float().abs().max()) > 0

    # ---- forward operand
    g = torch.Generator().manual_seed(100 + d + r)
    h = bf(torch.randn(T, d, generator=g))
    hd_ = h.to(DEV)
    thr, scale = dropout_threshold(p_)
    keep = [torch.from_numpy(philox_keep(T * d, p_, tr._lora_seed, tr._lora_stream(call, i, ti))).view(T, d) for ti in range(3)]
    hdrop = [torch.where(keep[ti], h.float() * float(scale), torch.zeros(())).to(BF) for ti in range(3)]      # bf16(mask * h / keep), the kernel's arithmetic
    for ti in range(3):
        assert abs(float(keep[ti].float().mean()) - (1 - p_)) < 0.01
        got = nans(T, d, dtype=BF)
        hip.call("oneprot_dropout_bf16", hd_, got, T * d, p_, tr._lora_seed, tr._lora_stream(call, i, ti))
        assert torch.equal(got.cpu(), hdrop[ti]), f"dropout of target {ti} against the CPU Philox mask"
    Xc, u = tr._lora_branch_operand(i, hd_, T, call)
    assert tuple(Xc.shape) == (T, Kc) and tuple(u.shape) == (T, Rp)
    assert torch.equal(Xc[:, :d], hd_)
    assert torch.equal(Xc[:, d:d + Rp], u)
    assert float(Xc[:, d + Rp:].float().abs().max()) == 0.0
    uc = u.cpu()
    for ti in range(3):
        close(uc[:, ti * rp:ti * rp + r], hdrop[ti].double() @ a16[i, ti].double().t(), *TOL_BF16, f"u of target {ti}")
        if rp > r:
            assert float(uc[:, ti * rp + r:(ti + 1) * rp].float().abs().max()) == 0.0, "pad columns of u"

    # ---- concatenated product: [h | u | 0] [W | s B | 0]^T = h W^T + sum_t u_t (s B_t)^T
    cat = f64(Xc) @ f64(ops["Wc"][i]).t()
    two = h.double() @ W16[i].double().t()
    for ti in range(3):
        two[:, ti * d:(ti + 1) * d] += uc[:, ti * rp:ti * rp + r].double() @ b16[i, ti].double().t()
    close(cat, two, 1e-12, 1e-9, "concatenated operands against the two branches (fp64)")
    y = nans(T, 3 * d)
    gemm_nt(Xc, ops["Wc"][i], T, 3 * d, Kc, Kc, Kc, hip.EPI_F32, None, y)
    close(y, cat, *tol_f32(Kc), "kernel product at K = Kc")

    # ---- backward
    dq = bf(torch.randn(T, 3 * d, generator=g) * 0.5)
    dqd = dq.to(DEV)
    ws_tn = tr._tn_workspace(((3 * d, Rp), (rp, d)), DEV)
    dh0 = bf(torch.randn(T, d, generator=g))
    du = nans(T, Rp, dtype=BF)      # the same launch as _lora_branch_backward's first: its own bf16 intermediate
    gemm_nt(dqd, ops["BsT"][i], T, Rp, 3 * d, 3 * d, 3 * d, hip.EPI_BF16, None, du)
    duc = du.cpu()
    close(duc, dq.double() @ BsT[i].double().t(), *TOL_BF16, "du = dqkv (s B)")
    terms = []                       # mask_t * (du_t A_t) / keep from the kernel's own bf16 du_t A_t
    for ti in range(3):
        if rp > r:
            assert float(duc[:, ti * rp + r:(ti + 1) * rp].float().abs().max()) == 0.0, "pad columns of du"
        dut = du[:, ti * rp:(ti + 1) * rp].contiguous()
        dhd = nans(T, d, dtype=BF)
        gemm_nt(dut, ops["AtT"][i, ti], T, d, rp, rp, rp, hip.EPI_BF16, None, dhd)
        close(dhd, duc[:, ti * rp:(ti + 1) * rp].double() @ AtT[i, ti].double().t(), *TOL_BF16, f"du_t A_t of target {ti}")
        terms.append(torch.where(keep[ti], f64(dhd) * float(scale), torch.zeros((), dtype=torch.float64)))
    inc = sum(terms)
    mag = dh0.double().abs() + sum(t.abs() for t in terms)
    raws = []
    for form in ("dh16", "dh32"):
        raw = tuple(torch.full_like(b, NAN) for b in tr._lora_raw_buffers(DEV))
        dh = (dh0 if form == "dh16" else dh0.float()).to(DEV, copy=True)
        tr._lora_branch_backward(i, hd_, u, dqd, T, call, ws_tn, raw, **{form: dh})
        assert bool(torch.isnan(raw[0][1 - i]).all()) and bool(torch.isnan(raw[1][1 - i]).all()), "another layer's gradients were touched"
        close(raw[1][i], dq.double().t() @ uc.double(), *tol_tn(T), "dB_raw = dqkv^T u")
        for ti in range(3):
            rows = raw[0][i, ti * rp:(ti + 1) * rp]
            close(rows, duc[:, ti * rp:(ti + 1) * rp].double().t() @ hdrop[ti].double(), *tol_tn(T), f"dA_raw rows of target {ti}")
            if rp > r:
                assert float(rows[r:].abs().max()) == 0.0, "pad rows of dA_raw"
        # three sequential adds; every partial sum is at most `mag` in size and is rounded to the gradient's format (unit roundoff 2^-8 for bf16: 8 significand bits,
        # 2^-24 for fp32), the fp32 product and add inside each step contribute 2 * 2^-24 more: |error| <= ((1 + e)^3 - 1) mag
        e = (2.0 ** -8 if form == "dh16" else 2.0 ** -24) + 2 * 2.0 ** -24
        close(dh, dh0.double() + inc, 0.0, ((1 + e) ** 3 - 1) * mag + 1e-30, f"{form} += sum_t mask_t (du_t A_t) / keep")
        raws.append(raw)
    assert torch.equal(raws[0][0][i], raws[1][0][i]) and torch.equal(raws[0][1][i], raws[1][1][i])


# ====================================================================================================== 6. RoPE epilogue, short sequences
@functools.lru_cache(maxsize=None)
def _rope_case(B, L, H, hd, K):
    d = H * hd
    M, N = B * L, 3 * d
    g = torch.Generator().manual_seed(5 + L + hd)
    A = bf(torch.randn(M, K, generator=g))
    W = bf(torch.randn(N, K, generator=g) * 0.1)
    if K != d:                                                   # the two-branch launch: [h | u | 0] x [W | s B | 0]^T with K = Kc
        A[:, d + 24:] = 0
        W[:, d + 24:] = 0
    bias = torch.randn(N, generator=g) * 0.5
    cos, sin = O.rope_tables(1026, hd)                           # as production holds them: 1026 positions
    y = (A.double() @ W.double().t() + bias.double()).view(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    c, s = cos[:L].double(), sin[:L].double()
    return A, W, bias, cos[:, : hd // 2].contiguous(), sin[:, : hd // 2].contiguous(), O.apply_rope(y[0] * hd ** -0.5, c, s), O.apply_rope(y[1], c, s), y[2].contiguous()


# L < 8: one 8-row step of the staged epilogue crosses several sequence boundaries (L = 1: eight); L = 8, 9: the edge where a single wrap suffices;
# (2, 130, 20, 32) at K = 768: the shape of the two-branch launch, K = Kc != d
@pytest.mark.parametrize("B,L,H,hd,K", [(40, 1, 4, 16, 64), (24, 3, 2, 32, 64), (16, 5, 2, 32, 64), (20, 7, 4, 16, 64), (9, 8, 2, 32, 64), (7, 9, 2, 64, 128),
                                        (2, 130, 20, 32, 768)])
def test_gemm_qkv_rope_short_sequences(B, L, H, hd, K, gemm_shape):
    d = H * hd
    M, N = B * L, 3 * d
    A, W, bias, cosh, sinh, qr, kr, vr = _rope_case(B, L, H, hd, K)
    n, G = B * H * L * hd, 4096
    bufs = [nans(G + n + G, dtype=BF) for _ in range(3)]         # NaN guard bands in front of and behind q, k and v
    q, k, v = (b[G:] for b in bufs)
    gemm_nt(A.to(DEV), W.to(DEV), M, N, K, K, K, hip.EPI_QKV_ROPE, bias.to(DEV), q, k, v, None, cosh.to(DEV), sinh.to(DEV), hd ** -0.5, L, H, hd)
    for name, b, ref in (("q", bufs[0], qr), ("k", bufs[1], kr), ("v", bufs[2], vr)):
        assert bool(torch.isnan(b[:G]).all()) and bool(torch.isnan(b[G + n:]).all()), f"{name}: wrote outside the output"
        close(b[G:G + n].view(B, H, L, hd), ref, *TOL_BF16, name)
