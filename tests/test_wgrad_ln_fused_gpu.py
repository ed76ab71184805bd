"""oneprot_gemm_tn_ln_bwd: a weight gradient and a LayerNorm backward in one launch on disjoint CUs (csrc/gemm_tn.hip: k_gemm_tn8_ln).

The launch must compute what the two entry points it replaces compute: dx and its bf16 copy bit for bit (the row body is shared, csrc/ln_bwd_row.h), dW and
dbias bit for bit what oneprot_gemm_bf16_tn gives under a CU reserve of the LayerNorm role's size (same token splits, same fixed-order slab sum), dgamma and
dbeta in another partial order (one partial per role work-group) against fp64.  Shapes: whole tiles; a partial last n-tile with token units that do not divide
by the splits; three token units (most matrix work items own none, fewer rows than LayerNorm-role waves); the 8M width (another NV of the row body).  The
tower case runs EsmTransformer.backward_layers with the fused launches and with the separate ones from one saved forward."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oneprot_amd import hip  # noqa: E402
from tests.cases import DEV, free, gen, randn  # noqa: E402
from tests.gate import close  # noqa: E402

F64 = torch.float64
GUARD = 4096
CASES = [(2048, 2560, 640), (2080, 1920, 640), (96, 2560, 640), (1024, 1280, 320)]


def _guarded(nbytes):
    w = torch.zeros(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    w[nbytes:] = 0xA5
    return w


def _intact(w, nbytes):
    return bool((w[nbytes:] == 0xA5).all())


@functools.lru_cache(maxsize=1)
def _case(M, N, K):
    """inputs, fp64 references and the outputs of the two separate entry points for one shape; computed once, never written again"""
    free()
    g = gen(M + N + K)
    c = dict(dY=randn((M, N), g, 0.5, dtype=torch.bfloat16), X=randn((M, K), g, 0.5, dtype=torch.bfloat16), dy=randn((M, K), g, dtype=torch.bfloat16),
             x=randn((M, K), g, 2.0, 0.5), gamma=randn(K, g, 0.2, 1.0), add=randn((M, K), g))
    c["mean"], c["rstd"] = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    hip.call("oneprot_layernorm_fwd", c["x"], 0, c["gamma"], torch.zeros(K, device=DEV), None, torch.empty(M, K, device=DEV), c["mean"], c["rstd"], M, K, 1e-5)
    c["dW64"] = c["dY"].to(F64).t() @ c["X"].to(F64)
    c["db64"] = c["dY"].to(F64).sum(0)
    xh = (c["x"].to(F64) - c["mean"].to(F64)[:, None]) * c["rstd"].to(F64)[:, None]
    c["dg64"], c["dbeta64"] = (c["dy"].to(F64) * xh).sum(0), c["dy"].to(F64).sum(0)
    w = torch.empty(hip.query("oneprot_layernorm_bwd_workspace", K), dtype=torch.uint8, device=DEV)
    for key, add in (("plain", None), ("inplace", c["add"])):
        dx = add.clone() if add is not None else torch.full((M, K), float("nan"), device=DEV)
        dx16 = torch.full((M, K), float("nan"), dtype=torch.bfloat16, device=DEV)
        dg, db = torch.empty(K, device=DEV), torch.empty(K, device=DEV)
        hip.call("oneprot_layernorm_bwd", c["dy"], 0, None, 0, c["x"], 0, c["gamma"], c["mean"], c["rstd"], dx if add is not None else None, dx, dx16, dg, db, w, M, K, 0)
        c[key] = (dx, dx16)
    return c


def _separate_tn(c, M, N, K, reserve):
    need = hip.query("oneprot_gemm_bf16_tn_workspace", N, K)
    w = torch.empty(need, dtype=torch.uint8, device=DEV)
    dW, db = torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    try:
        hip.query("oneprot_cu_reserve", reserve)
        hip.call("oneprot_gemm_bf16_tn", c["dY"], c["X"], M, N, K, N, K, dW, db, w, need, 0)
    finally:
        hip.query("oneprot_cu_reserve", hip.cu_reserve_wanted())
    return dW, db


def _fused(c, M, N, K, R, add):
    """one fused launch on NaN-filled outputs and guarded workspaces: (dW, dbias, dx, dx16, dgamma, dbeta)"""
    need = hip.query("oneprot_gemm_bf16_tn_workspace", N, K)
    need_ln = R * 2 * K * 4      # what the header asks for: ln_cus * 2 * K floats
    w, wl = _guarded(need), _guarded(need_ln)
    dW, db = torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    dx = add.clone() if add is not None else torch.full((M, K), float("nan"), device=DEV)
    dx16 = torch.full((M, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    dg, dbeta = torch.full((K,), float("nan"), device=DEV), torch.full((K,), float("nan"), device=DEV)
    hip.call("oneprot_gemm_tn_ln_bwd", c["dY"], c["X"], M, N, K, N, K, dW, db, w, need, 0, c["dy"], c["x"], c["gamma"], c["mean"], c["rstd"],
             dx if add is not None else None, dx, dx16, dg, dbeta, wl.view(torch.float32), 0, R)
    assert _intact(w, need), "wrote past the weight-gradient workspace"
    assert _intact(wl, need_ln), "wrote past the LayerNorm partials"
    return dW, db, dx, dx16, dg, dbeta


def _role_sizes(N):
    return sorted({hip.WGRAD_LN_CUS.get(N, 64), 64})      # the chosen size for this N, and 64


@pytest.mark.parametrize("M,N,K", CASES)
def test_fused_launch_equals_the_two_entry_points(M, N, K):
    c = _case(M, N, K)
    for R in _role_sizes(N):
        tag = f"({M}, {N}, {K}) R {R}"
        sep_dW, sep_db = _separate_tn(c, M, N, K, R)
        first = None
        for key, add in (("inplace", c["add"]), ("plain", None)):
            dW, db, dx, dx16, dg, dbeta = _fused(c, M, N, K, R, add)
            # the tolerances of test_gemm_tn_under_cu_reserve (tests/test_production_sizes_gpu.py)
            e1 = close(dW, c["dW64"], 1e-4, 2e-3 * math.sqrt(M / 64), f"dW {tag} {key}")
            e2 = close(db, c["db64"], 1e-4, 2e-2, f"dbias {tag} {key}")
            # tests/test_kernels_gpu.py:77-78  close(dg, gr.grad, 1e-4, 1e-3, "ln bwd dgamma") / close(db, br.grad, 1e-4, 1e-3, "ln bwd dbeta")
            e3 = close(dg, c["dg64"], 1e-4, 1e-3, f"dgamma {tag} {key}")
            e4 = close(dbeta, c["dbeta64"], 1e-4, 1e-3, f"dbeta {tag} {key}")
            print(f"{tag} {key}: max err dW {e1:.3e} dbias {e2:.3e} dgamma {e3:.3e} dbeta {e4:.3e}; dW bits equal {torch.equal(dW, sep_dW)}, dbias {torch.equal(db, sep_db)}, "
                  f"dx {torch.equal(dx, c[key][0])}, dx16 {torch.equal(dx16, c[key][1])}")
            assert torch.equal(dW, sep_dW), f"dW {tag} {key}: not the bits of oneprot_gemm_bf16_tn under oneprot_cu_reserve({R})"
            assert torch.equal(db, sep_db), f"dbias {tag} {key}: not the bits of oneprot_gemm_bf16_tn under oneprot_cu_reserve({R})"
            assert torch.equal(dx, c[key][0]), f"dx {tag} {key}: not the bits of oneprot_layernorm_bwd"
            assert torch.equal(dx16, c[key][1]), f"dx16 {tag} {key}: not the bits of oneprot_layernorm_bwd"
            if first is None:
                first = (dW, db, dg, dbeta)
                again = _fused(c, M, N, K, R, add)      # two calls, equal bits
                assert all(torch.equal(a, b) for a, b in zip(again, (dW, db, dx, dx16, dg, dbeta))), f"{tag}: two calls differ"
            else:      # add_to does not reach the parameter gradients
                assert all(torch.equal(a, b) for a, b in zip(first, (dW, db, dg, dbeta))), f"{tag}: parameter gradients depend on add_to"


def test_ineligible_shape_returns_the_error_and_writes_nothing():
    M, N, K = 2048, 2560, 576
    assert hip.query("oneprot_gemm_tn_ln_bwd_eligible", M, N, K) == 0
    g = gen(5)
    dY, X, dy = (randn(s, g, 0.5, dtype=torch.bfloat16) for s in ((M, N), (M, K), (M, K)))
    x, gamma, mean, rstd = randn((M, K), g), randn(K, g, 0.2, 1.0), torch.zeros(M, device=DEV), torch.ones(M, device=DEV)
    need = hip.query("oneprot_gemm_bf16_tn_workspace", N, K)
    w, wl = _guarded(need), _guarded(64 * 2 * K * 4)
    w[:need] = 0xA5
    wl[:64 * 2 * K * 4] = 0xA5
    outs = [torch.full(s, float("nan"), device=DEV) for s in ((N, K), (N,), (M, K), (K,), (K,))]
    dx16 = torch.full((M, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(hip.HipKernelError, match="returned -1"):
        hip.call("oneprot_gemm_tn_ln_bwd", dY, X, M, N, K, N, K, outs[0], outs[1], w, need, 0, dy, x, gamma, mean, rstd, None, outs[2], dx16, outs[3], outs[4],
                 wl.view(torch.float32), 0, 64)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs + [dx16])
    assert bool((w == 0xA5).all()) and bool((wl == 0xA5).all())
    # a role size the decode cannot keep, or one that leaves the matrix role less than its 64-CU floor, is refused the same way on a served shape
    c = _case(96, 2560, 640)
    for R in (0, 12, 256):
        with pytest.raises(hip.HipKernelError, match="returned -1"):
            _fused(c, 96, 2560, 640, R, None)


def test_tower_backward_with_and_without_the_fused_launches(monkeypatch):
    """backward_layers of a two-layer d = 640 tower from one saved forward, ONEPROT_WGRAD_LN=1 against =0: only the FFN-1 / QKV weight and bias gradients and the
    LayerNorm gamma / beta gradients may move (summation order), every activation gradient -- hence every other tensor -- keeps its bits"""
    from oneprot_amd.esm import ESM_DEFAULTS, EsmTransformer, ModelConfig
    free()
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.delenv("ONEPROT_CU_RESERVE", raising=False)
    monkeypatch.delenv("ONEPROT_WGRAD_LN_CUS", raising=False)
    torch.manual_seed(11)
    cfg = dict(ESM_DEFAULTS)
    cfg.update(hidden_size=640, num_hidden_layers=2, num_attention_heads=20, intermediate_size=2560)
    tr = EsmTransformer(ModelConfig(**cfg), add_pooling_layer=False).to(DEV).train()
    B, L, d = 4, 128, 640
    T = B * L
    ids = torch.randint(4, 24, (B, L), generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        _, saved = tr.run_layers(ids, save=True)
    g0 = randn((T, d), gen(17), 0.05)
    launches = []
    real = hip.gemm_tn_ln_bwd
    monkeypatch.setattr(hip, "gemm_tn_ln_bwd", lambda *a, **k: (launches.append(a[3]), real(*a, **k))[1])
    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("ONEPROT_WGRAD_LN", flag)
        gflat = torch.zeros(tr._total, device=DEV)
        n0 = len(launches)
        with torch.no_grad():
            tr.backward_layers(dict(saved, layers=list(saved["layers"])), g0.clone(), g0.to(torch.bfloat16), gflat)
        assert len(launches) - n0 == (4 if flag == "1" else 0), "two fused launches per layer when on, none when off"
        outs[flag] = gflat
    moved = ("attention.self.query.", "attention.self.key.", "attention.self.value.", "intermediate.dense.", ".LayerNorm.")
    n_moved = 0
    for name, (off, n, shape) in tr._spec.items():
        a, b = outs["1"][off:off + n], outs["0"][off:off + n]
        if name.startswith("encoder.layer.") and any(m in name for m in moved):
            n_moved += 1
            if "LayerNorm" in name:
                close(a, b, 1e-4, 1e-3, name)                            # two fp32 orders of one sum: twice the kernel tolerance is not needed, one holds
            elif name.endswith("bias"):
                close(a, b, 1e-4, 2e-2, name)
            else:
                close(a, b, 1e-4, 2e-3 * math.sqrt(T / 64), name)
        else:
            assert torch.equal(a, b), f"{name}: moved with ONEPROT_WGRAD_LN"
    assert n_moved == 2 * (6 + 2 + 4)
    assert bool(torch.isfinite(outs["0"]).all()) and float(tr.view("embeddings.word_embeddings.weight", outs["1"]).abs().max()) > 0
