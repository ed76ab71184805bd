"""Kernels at the sizes the training step runs (bench.py: cfg-2 T = 256 x 512 rows at d = 640, cfg-4 BERT 65 536 rows at d = 768, cfg-5 d = 1280,
an Adam arena of ~150 M parameters) against fp64 torch on the GPU, computed from the inputs the kernel sees (bf16-rounded where it reads bf16).

Many launchers cap their grid and turn into grid-stride loops (LayerNorm 4096 x 4 rows, LayerNorm backward 1024 blocks and 1024 partials, the elementwise
kernels 4096 x 256, the reductions 1024 x 1024, Adam 8192 x 1024, the casts 8192 x 1024, the dropout kernels 4096 x 256 x 8 elements), and the TN weight-
gradient GEMM picks its token splits from the CUs left by oneprot_cu_reserve: every case here is past such a cap or under a reserve.  The dropout masks
are compared element by element with an independent Philox4x32-10 (tests/philox_ref.py, pinned on the Random123 known answers in test_philox_ref_cpu.py).

Tolerances follow from fp32 arithmetic: eps32 = 2^-24 ~ 6e-8 per rounding.  A per-row LayerNorm over d <= 1280 carries a few roundings of its d-term
sums (1e-5, as in test_kernels_gpu.py); a column sum over T rows in fixed-order partials drifts like eps32 * sqrt(#terms) * sqrt(#partials) * term size,
for which 1e-5 * sqrt(T) * rms(term) keeps a margin of ten or more.  Every deliberate error these tests guard against (a lost grid-stride pass, a lost
partial, a mask indexed by thread) is an O(1) fraction of the result, far above them."""
import math

import pytest
import torch

from tests import philox_ref as PR

pytestmark = pytest.mark.gpu

from oneprot_amd import hip  # noqa: E402
from tests.cases import DEV, SEED_HI, STREAM_HI, free, gen, randn, ws  # noqa: E402
from tests.gate import close  # noqa: E402

F64 = torch.float64
def colsum_atol(terms_rms, n):
    """fp32 fixed-order sum of n terms of rms `terms_rms`: rounding drift ~ eps32 * n^(1/2 ... 3/4) * rms; 1e-5 * sqrt(n) * rms bounds it with margin"""
    return 1e-5 * math.sqrt(n) * float(terms_rms) + 1e-30


def _ln_ref(x64, gamma64, beta64, eps):
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x64 - mean) * rstd * gamma64 + beta64, mean.squeeze(-1), rstd.squeeze(-1)


def _ln_bwd_ref(dy64, x64, gamma64, mean64, rstd64):
    xh = (x64 - mean64[:, None]) * rstd64[:, None]
    g = dy64 * gamma64
    dx = rstd64[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy64 * xh).sum(0), dy64.sum(0), (dy64 * xh).pow(2).mean().sqrt(), dy64.pow(2).mean().sqrt()


# ================================================================================================================== 1. row kernels
@pytest.mark.parametrize("T,d", [(131072, 640), (65536, 768), (32768, 1280)])
def test_layernorm_fwd_bwd_production_rows(T, d):
    """k_layernorm_fwd past its 4096 x 4-row grid, k_layernorm_bwd + k_ln_reduce with all 1024 partials each covering many rows; fp32 and bf16 x; every
    dy_mode; add_to separate and in place; the bf16 dx copy; dgamma / dbeta overwritten and accumulated -- against fp64 sums over all rows"""
    g = gen(T + d)
    eps = 1e-5
    gamma, beta = randn(d, g, 0.2, 1.0), randn(d, g, 0.2)
    gamma64, beta64 = gamma.to(F64), beta.to(F64)
    w = ws(hip.query("oneprot_layernorm_bwd_workspace", d))
    for x_bf16 in (0, 1):
        x = randn((T, d), g, 2.0, 0.5, torch.bfloat16 if x_bf16 else torch.float32)
        x64 = x.to(F64)
        yb, yf = torch.empty(T, d, dtype=torch.bfloat16, device=DEV), torch.empty(T, d, device=DEV)
        mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
        hip.call("oneprot_layernorm_fwd", x, x_bf16, gamma, beta, yb, yf, mean, rstd, T, d, eps)
        y64, m64, r64 = _ln_ref(x64, gamma64, beta64, eps)
        close(yf, y64, 1e-5, 1e-5, f"ln fwd f32 (x bf16 {x_bf16})")
        close(yb, y64, 2 ** -8, 1e-6, f"ln fwd bf16 copy (x bf16 {x_bf16})")      # one bf16 rounding of the fp32 value
        close(mean, m64, 1e-5, 1e-6, "mean")
        close(rstd, r64, 1e-5, 0.0, "rstd")
        del yb, yf, y64
        # dy_mode 1 (fp32 dy), separate add_to, fresh dgamma / dbeta
        dy = randn((T, d), g)
        add = randn((T, d), g)
        dx, dx16 = torch.empty(T, d, device=DEV), torch.empty(T, d, dtype=torch.bfloat16, device=DEV)
        dg, db = torch.full((d,), 7.0, device=DEV), torch.full((d,), -3.0, device=DEV)
        hip.call("oneprot_layernorm_bwd", dy, 1, None, 0, x, x_bf16, gamma, mean, rstd, add, dx, None, dg, db, w, T, d, 0)
        dx64, dg64, db64, rg, rb = _ln_bwd_ref(dy.to(F64), x64, gamma64, m64, r64)
        close(dx, dx64 + add.to(F64), 1e-4, 1e-4, "ln bwd dx (dy f32, add_to)")
        close(dg, dg64, 1e-5, colsum_atol(rg, T), "ln bwd dgamma (dy f32)")
        close(db, db64, 1e-5, colsum_atol(rb, T), "ln bwd dbeta (dy f32)")
        # dy_mode 0 (bf16 dy), in place on the residual gradient, bf16 copy of dx, accumulated into the previous dgamma / dbeta
        dyb = dy.to(torch.bfloat16)
        dx2 = add.clone()
        hip.call("oneprot_layernorm_bwd", dyb, 0, None, 0, x, x_bf16, gamma, mean, rstd, dx2, dx2, dx16, dg, db, w, T, d, 1)
        dx64b, dg64b, db64b, rg, rb = _ln_bwd_ref(dyb.to(F64), x64, gamma64, m64, r64)
        close(dx2, dx64b + add.to(F64), 1e-4, 1e-4, "ln bwd dx (dy bf16, in place)")
        assert torch.equal(dx16, dx2.to(torch.bfloat16)), "bf16 dx copy is not the rounding of the fp32 dx"
        close(dg, dg64 + dg64b, 1e-5, 2 * colsum_atol(rg, T), "ln bwd dgamma accumulated")
        close(db, db64 + db64b, 1e-5, 2 * colsum_atol(rb, T), "ln bwd dbeta accumulated")
        del dy, dyb, add, dx2, dx64, dx64b
        # dy_mode 2: dy[t] = dpool[t / L] * wrow[t] (the pooled-gradient broadcast), no add_to
        L = 512
        dpool = randn((T // L, d), g)
        wrow = torch.rand(T, generator=g, device=DEV) / L
        hip.call("oneprot_layernorm_bwd", dpool, 2, wrow, L, x, x_bf16, gamma, mean, rstd, None, dx, dx16, dg, db, w, T, d, 0)
        dyp = dpool.to(F64).repeat_interleave(L, 0) * wrow.to(F64)[:, None]
        dx64, dg64, db64, rg, rb = _ln_bwd_ref(dyp, x64, gamma64, m64, r64)
        close(dx, dx64, 1e-4, 1e-4 * float(dx64.abs().max()), "ln bwd dx (pooled broadcast)")
        close(dg, dg64, 1e-5, colsum_atol(rg, T), "ln bwd dgamma (pooled broadcast)")
        close(db, db64, 1e-5, colsum_atol(rb, T), "ln bwd dbeta (pooled broadcast)")
        del x, x64, dx, dx16, dyp, dx64
        free()


def _packed_lengths(g, target, n_min):
    """segment lengths 1 .. 1026 (the ESM maximum), a few of each edge, summing to just under `target` with at least n_min segments"""
    lens = [1, 2, 1026, 1025, 64, 65, 255, 256, 257]
    while sum(lens) < target - 600:
        lens.append(int(torch.randint(1, 560, (1,), generator=g)))
    lens.append(target - 40 - sum(lens))
    assert len(lens) >= n_min and all(1 <= n <= 1026 for n in lens)
    return lens


@pytest.mark.parametrize("d", [480, 640, 1280])
def test_packed_layernorm_pooling_production_stream(d):
    """oneprot_lnpool_packed_fwd / _bwd (the packed stream's final LayerNorm + pooling) and the attention1d form (lnpool -> attnpool_packed -> layernorm_bwd)
    on a 65 536-row stream of > 200 segments: pooled rows, per-row statistics, dx (exact zeros on the tail rows), dgamma / dbeta over all rows"""
    gcpu = torch.Generator().manual_seed(d)
    lens = _packed_lengths(gcpu, 65536, 200)
    N = len(lens)
    T = -(-sum(lens) // 256) * 256 + 256                      # a tail of more than one block of rows
    cu_l = [0]
    for n in lens:
        cu_l.append(cu_l[-1] + n)
    cu = torch.tensor(cu_l, dtype=torch.int32, device=DEV)
    seg = torch.repeat_interleave(torch.arange(N, device=DEV), torch.tensor(lens, device=DEV))
    ids = torch.full((T,), 1, dtype=torch.int64, device=DEV)
    ids[:cu_l[-1]] = torch.randint(4, 24, (cu_l[-1],), generator=gcpu).to(DEV)
    g = gen(d)
    eps = 1e-5
    x = randn((T, d), g, 1.5, 0.3)
    gamma, beta = randn(d, g, 0.2, 1.0), randn(d, g, 0.2)
    pw, pb = randn(d, g, 0.1), randn(1, g, 0.1)
    dpool = randn((N, d), g)
    w = ws(hip.query("oneprot_layernorm_bwd_workspace", d))
    real = cu_l[-1]
    lens64 = torch.tensor(lens, dtype=F64, device=DEV)
    for mode in ("mean", "cls", "attention1d"):
        xr = x.to(F64).requires_grad_(True)
        gr, br, pwr, pbr = (t.to(F64).requires_grad_(True) for t in (gamma, beta, pw, pb))
        h = torch.nn.functional.layer_norm(xr, (d,), gr, br, eps)
        hs = h[:real]
        if mode == "mean":
            ref = torch.zeros(N, d, dtype=F64, device=DEV).index_add(0, seg, hs) / lens64[:, None]
        elif mode == "cls":
            ref = hs[cu[:-1].long()]
        else:
            s = hs @ pwr + pbr
            s.retain_grad()
            smax = torch.zeros(N, dtype=F64, device=DEV).scatter_reduce(0, seg, s.detach(), "amax", include_self=False)
            e = torch.exp(s - smax[seg])
            a = e / torch.zeros(N, dtype=F64, device=DEV).index_add(0, seg, e)[seg]
            ref = torch.zeros(N, d, dtype=F64, device=DEV).index_add(0, seg, a[:, None] * hs)
        (ref * dpool.to(F64)).sum().backward()
        pooled = torch.empty(N, d, device=DEV)
        mean, rstd, wrow = (torch.full((T,), 5.0, device=DEV) for _ in range(3))
        dx = torch.full((T, d), 9.0, device=DEV)
        dx16 = torch.full((T, d), 9.0, dtype=torch.bfloat16, device=DEV)
        dg, db = torch.empty(d, device=DEV), torch.empty(d, device=DEV)
        if mode == "attention1d":
            hidden = torch.empty(T, d, device=DEV)
            hip.call("oneprot_lnpool_packed_fwd", x, ids, cu, 1, gamma, beta, pooled, mean, rstd, wrow, hidden, N, T, d, eps, 0)
            close(hidden, h.detach(), 1e-5, 1e-5, "packed hidden")
            attn = torch.empty(T, device=DEV)
            hip.call("oneprot_attnpool_packed_fwd", hidden, ids, cu, 1, pw, pb, pooled, attn, N, max(lens), d)
            dh = torch.full((T, d), 9.0, device=DEV)
            dw, dbias = torch.empty(d, device=DEV), torch.empty(1, device=DEV)
            hip.call("oneprot_attnpool_packed_bwd", hidden, attn, cu, pw, dpool, dw, dbias, dh, ws(hip.query("oneprot_attnpool_bwd_workspace", N, d)),
                     N, T, max(lens), d)
            assert bool((dh[real:] == 0).all()), "attention1d: tail rows of dhidden are not exactly zero"
            hip.call("oneprot_layernorm_bwd", dh, 1, None, 0, x, 0, gamma, mean, rstd, None, dx, dx16, dg, db, w, T, d, 0)
            # the softmax weights carry __expf's relative error (~1e-6 over this range of scores) on top of the fp32 sums over <= 1026 rows
            close(dw, pwr.grad, 1e-4, colsum_atol(1.0, real) * float(pwr.grad.abs().max()), "attention1d dw")
            # sum_l ds_l vanishes per segment: the kernel's value is rounding noise of the sum of |ds| terms
            close(dbias, pbr.grad, 1e-4, colsum_atol(float(s.grad.pow(2).mean().sqrt()), real), "attention1d dbias")
            prt = 1e-4
        else:
            hip.call("oneprot_lnpool_packed_fwd", x, ids, cu, 1, gamma, beta, pooled, mean, rstd, wrow, None, N, T, d, eps, 0 if mode == "mean" else 1)
            hip.call("oneprot_lnpool_packed_bwd", dpool, cu, wrow, x, gamma, mean, rstd, dx, dx16, dg, db, w, N, T, d)
            prt = 1e-5
        close(pooled, ref.detach(), prt, 1e-5, f"packed pooled ({mode})")
        _, m64, r64 = _ln_ref(x.to(F64), gamma.to(F64), beta.to(F64), eps)
        close(mean, m64, 1e-5, 1e-6, f"packed mean ({mode})")
        close(rstd, r64, 1e-5, 0.0, f"packed rstd ({mode})")
        assert bool((wrow[real:] == 0).all()), f"{mode}: tail rows carry a pooling weight"
        assert bool((dx[real:] == 0).all()) and bool((dx16[real:] == 0).all()), f"{mode}: tail rows of dx are not exactly zero"
        # dx per row: cancellation inside rstd * (g - mean(g) - xhat mean(g xhat)) leaves errors of a few eps32 * d^(1/2) of the row's largest term
        close(dx[:real], xr.grad[:real], 1e-4, 4e-5 * float(xr.grad.abs().max()), f"packed dx ({mode})")
        xh = (x.to(F64) - m64[:, None]) * r64[:, None]
        ref_dg, ref_db = gr.grad, br.grad
        term = float(dpool.abs().max()) * (1.0 if mode != "mean" else 1.0 / min(lens))
        close(dg, ref_dg, 1e-5, colsum_atol(term * float(xh.abs().max()), real), f"packed dgamma ({mode})")
        close(db, ref_db, 1e-5, colsum_atol(term, real), f"packed dbeta ({mode})")
        del xr, h, hs, ref, xh
        free()


def test_dropout_add_layernorm_fwd_production_rows():
    """oneprot_dropout_add_layernorm_fwd at 40 000 rows of d = 768 (BERT hidden dropout + residual + LayerNorm; the grid caps at 4096 x 4 rows): the sum
    bit for bit against the independent Philox mask, the LayerNorm against fp64"""
    T, d, p, eps = 40000, 768, 0.1, 1e-12
    g = gen(768)
    x, resid = randn((T, d), g), randn((T, d), g)
    gamma, beta = randn(d, g, 0.1, 1.0), randn(d, g, 0.1)
    keep = torch.from_numpy(PR.philox_keep(T * d, p, SEED_HI, STREAM_HI)).to(DEV).view(T, d)
    _, scale = PR.dropout_threshold(p)
    s_ref = torch.where(keep, x * float(scale), torch.zeros((), device=DEV)) + resid
    s, y16, y = torch.empty_like(x), torch.empty(T, d, dtype=torch.bfloat16, device=DEV), torch.empty_like(x)
    m, r = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
    hip.call("oneprot_dropout_add_layernorm_fwd", x, resid, s, gamma, beta, y16, y, m, r, T, d, eps, p, SEED_HI, STREAM_HI)
    assert torch.equal(s, s_ref), f"sum differs from resid + Philox dropout(x) at {int((s != s_ref).sum())} elements"
    y64, m64, r64 = _ln_ref(s_ref.to(F64), gamma.to(F64), beta.to(F64), eps)
    close(y, y64, 1e-5, 1e-5, "dropout+LN fp32")
    close(y16, y64, 2 ** -8, 1e-6, "dropout+LN bf16")
    close(m, m64, 1e-5, 1e-6, "dropout+LN mean")
    close(r, r64, 1e-5, 0.0, "dropout+LN rstd")


def test_bert_embed_fwd_production_rows():
    """oneprot_bert_embed_fwd at B x L = 128 x 512 (65 536 rows, past the 16 384-row grid) with the BERT-base table: LayerNorm(word[id] + pos[l] + type0);
    ids out of [0, vocab) read row 0, pad ids (0) embed like any other token"""
    B, L, d, V, eps = 128, 512, 768, 30522, 1e-12
    g = gen(30522)
    ids = torch.randint(1, V, (B, L), generator=g, device=DEV)
    ids[:, 0] = 101
    ids[5, 300:] = 0
    ids[127, 1:] = 0
    ids[3, 17], ids[100, 511], ids[64, 2] = -1, V, V + 12345
    word, pos, type0 = randn((V, d), g, 0.05), randn((512, d), g, 0.05), randn(d, g, 0.05)
    gamma, beta = randn(d, g, 0.1, 1.0), randn(d, g, 0.1)
    xf, xb = torch.empty(B * L, d, device=DEV), torch.empty(B * L, d, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_bert_embed_fwd", ids, word, pos, type0, gamma, beta, xf, xb, B, L, d, V, eps)
    idc = torch.where((ids >= 0) & (ids < V), ids, torch.zeros_like(ids)).view(-1)
    e64 = word.to(F64)[idc] + pos.to(F64).repeat(B, 1) + type0.to(F64)
    y64, _, _ = _ln_ref(e64, gamma.to(F64), beta.to(F64), eps)
    close(xf, y64, 1e-5, 1e-5, "bert embed fp32")
    close(xb, y64, 2 ** -8, 1e-6, "bert embed bf16")


@pytest.mark.parametrize("mode", [0, 1], ids=["mean", "cls"])
def test_pool_fwd_bwd_ragged(mode):
    """oneprot_pool_fwd / _bwd (pooling of an already normalised tower output, BERT) at (256, 256, 768) with ragged padding, the bf16 gradient copy"""
    B, L, d, pad = 256, 256, 768, 0
    g = gen(256 + mode)
    ids = torch.randint(1, 30000, (B, L), generator=g, device=DEV)
    lens = torch.randint(1, L + 1, (B,), generator=g, device=DEV)
    lens[0], lens[1], lens[2] = 1, L, L - 1
    ids[torch.arange(L, device=DEV)[None, :] >= lens[:, None]] = pad
    x = randn((B, L, d), g)
    pooled = torch.empty(B, d, device=DEV)
    hip.call("oneprot_pool_fwd", x, ids, pad, pooled, B, L, d, mode)
    valid = (ids != pad).to(F64)
    if mode == 0:
        wt = valid / valid.sum(1, keepdim=True)
    else:
        wt = torch.zeros(B, L, dtype=F64, device=DEV)
        wt[:, 0] = 1.0
    ref = (x.to(F64) * wt[:, :, None]).sum(1)
    close(pooled, ref, 1e-5, 1e-6, "pool fwd")                # a sum of <= 256 rows per column
    dp = randn((B, d), g)
    gx, g16 = torch.full((B, L, d), 9.0, device=DEV), torch.empty(B, L, d, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_pool_bwd", dp, ids, pad, gx, g16, B, L, d, mode)
    gref = dp.to(F64)[:, None, :] * wt[:, :, None]
    close(gx, gref, 2e-7, 0.0, "pool bwd")                    # dp * fl(1/n): two roundings
    assert torch.equal(g16, gx.to(torch.bfloat16))
    assert bool((gx[wt == 0] == 0).all()), "pool bwd writes a gradient on padding"


def test_embed_scatter_sorted_and_rowsum_bert_backward_shapes():
    """The BERT embedding backward at B x L = 128 x 512, d = 768, vocab 30522 (bert.py): oneprot_embed_scatter_sorted over the stable sort of the ids (the
    padding row is skipped and keeps what it held), oneprot_rowsum_f32 for the position rows (sum over the batch) and the token-type row"""
    B, L, d, V, pad = 128, 512, 768, 30522, 0
    T = B * L
    g = gen(317)
    ids = torch.randint(0, 2000, (B, L), generator=g, device=DEV)         # a small id range: runs of up to ~80 equal ids
    ids[:, 0] = 101
    ids[7, 100:] = pad
    ids[9, 3] = V - 1
    de = randn((T, d), g)
    sorted_ids, perm = torch.sort(ids.reshape(-1), stable=True)
    rows, counts = torch.unique_consecutive(sorted_ids, return_counts=True)
    starts = (torch.cumsum(counts, 0) - counts).contiguous()
    table = torch.full((V, d), 3.25, device=DEV)
    hip.call("oneprot_embed_scatter_sorted", de, perm.contiguous(), starts, rows.contiguous(), T, int(rows.numel()), d, pad, table)
    ref = torch.zeros(V, d, dtype=F64, device=DEV).index_add(0, ids.reshape(-1), de.to(F64))
    used = torch.zeros(V, dtype=torch.bool, device=DEV)
    used[rows] = True
    used[pad] = False
    close(table[used], ref[used], 1e-5, colsum_atol(1.0, int(counts.max())), "scatter sorted")
    assert bool((table[~used] == 3.25).all()), "rows no token used (or the skipped padding row) were written"
    dpos = torch.full((L + 3, d), -1.0, device=DEV)
    hip.call("oneprot_rowsum_f32", de, dpos[:L], B, L * d)
    ref_pos = de.to(F64).view(B, L * d).sum(0).view(L, d)
    close(dpos[:L], ref_pos, 1e-5, colsum_atol(1.0, B), "rowsum over the batch")
    assert bool((dpos[L:] == -1.0).all())
    tt = torch.empty(d, device=DEV)
    hip.call("oneprot_rowsum_f32", dpos[:L], tt, L, d)
    close(tt, dpos[:L].to(F64).sum(0), 1e-5, colsum_atol(float(dpos[:L].pow(2).mean().sqrt()), L), "rowsum token type")


def test_esm_embed_bwd_production_rows():
    """oneprot_esm_embed_bwd at B x L = 256 x 512 (cfg-2) with the token-dropout row scale: ~4000 tokens per vocabulary row through the 512 chunk partials"""
    B, L, d, V = 256, 512, 640, 33
    g = gen(33)
    ids = torch.randint(4, 24, (B, L), generator=g, device=DEV)
    ids[:, 0] = 0
    ids[10, 200:] = 1
    ids[torch.rand(B, L, generator=g, device=DEV) < 0.02] = 32
    dx = randn((B * L, d), g)
    rs = torch.rand(B, generator=g, device=DEV) + 0.5
    dt = torch.full((V, d), 0.5, device=DEV)
    hip.call("oneprot_esm_embed_bwd", ids, dx, rs, dt, ws(hip.query("oneprot_esm_embed_bwd_workspace", B * L, d, V)), B, L, d, V, 1, 32, 1, 1)
    flat = ids.reshape(-1)
    keep = (flat != 1) & (flat != 32)
    contrib = dx.to(F64) * rs.to(F64).repeat_interleave(L)[:, None]
    ref = torch.zeros(V, d, dtype=F64, device=DEV).index_add(0, flat[keep], contrib[keep]) + 0.5
    cnt = int(torch.bincount(flat[keep]).max())
    close(dt, ref, 1e-5, colsum_atol(1.5, cnt), "esm embed bwd (accumulated)")


# ================================================================================================================== 2. elementwise, reductions, optimiser
N_EW = 5 * (1 << 20) + 77                                      # past 4096 x 256 = 1 048 576 five times over, not a multiple of 256


def test_elementwise_kernels_past_their_grid():
    g = gen(5)
    x = randn(N_EW, g, 2.0)
    x[:7] = 0.0
    x64 = x.to(F64)
    y = torch.empty_like(x)
    hip.call("oneprot_gelu_f32", x, y, N_EW)
    cdf = 0.5 * (1 + torch.erf(x64 / math.sqrt(2)))
    close(y, x64 * cdf, 1e-5, 1e-6, "gelu")                   # erff: a few ulp
    dy = randn(N_EW, g)
    hip.call("oneprot_gelu_bwd_f32", x, dy, y, N_EW)
    pdf = torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
    close(y, dy.to(F64) * (cdf + x64 * pdf), 1e-4, 1e-5, "gelu bwd")    # __expf in the pdf term
    # L1 backward: dx (+)= coef * upstream * sign(x) -- exact in fp32
    coef = 0.37
    up = torch.tensor([1.75], device=DEV)
    sgn = torch.sign(x)
    for accumulate in (0, 1):
        for upstream in (None, up):
            base = randn(N_EW, g)
            out = base.clone()
            hip.call("oneprot_l1_bwd", x, out, N_EW, coef, upstream, accumulate)
            c = torch.tensor(coef, device=DEV) * (upstream[0] if upstream is not None else 1.0)
            want = c * sgn
            if accumulate:
                want = base + want
            assert torch.equal(out, want), f"l1_bwd accumulate={accumulate} upstream={upstream is not None}: {int((out != want).sum())} elements differ"
    # x *= s[0]
    s = torch.tensor([-0.8125], device=DEV)
    z = x.clone()
    hip.call("oneprot_scale_by_device_scalar", z, N_EW, s)
    assert torch.equal(z, x * s[0])
    # additive key-padding bias
    ids = torch.randint(0, 5, (N_EW,), generator=g, device=DEV)
    bias = torch.full((N_EW,), 3.0, device=DEV)
    hip.call("oneprot_key_padding_bias", ids, bias, N_EW, 1)
    assert torch.equal(bias, torch.where(ids == 1, torch.tensor(torch.finfo(torch.float32).min, device=DEV), torch.zeros((), device=DEV)))


def _arena_numel():
    import os
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    enc = SequenceEncoder("facebook/esm2_t30_150M_UR50D", output_dim=1024, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
    n = enc.transformer.flat.numel()
    del enc
    return n


@pytest.fixture(scope="module")
def arena_numel():
    return _arena_numel()


@pytest.mark.parametrize("size", ["1", "2", "3", "1048577", "arena"])
def test_reductions_past_their_grid(size, arena_numel):
    """sumsq, abs_sum and dot (k_reduce_stage1, 1024 x 256 threads x float4, then k_final_sum) from 1 element to the 150M arena, n % 4 != 0 everywhere; the
    tail elements past the last float4 are large so that losing them cannot hide in rounding; `out` is accumulated into"""
    n = arena_numel + 3 - arena_numel % 4 if size == "arena" else int(size)
    assert n % 4
    g = gen(n)
    x = randn(n, g)
    x[n - n % 4:] = 30.0
    y = x * (torch.rand(n, generator=g, device=DEV) + 0.5)           # x . y: non-negative terms, like sumsq
    w = ws(hip.query("oneprot_sumsq_workspace"))
    x64 = x.to(F64)
    # fp32: each thread sums up to ~150 float4 groups in order, then 256-wide block and 1024-partial sums: relative drift well under 1e-5 for
    # non-negative terms (the tail of 30.0s is ~1e-4 of the arena sum and all of it for n <= 3)
    rt = 1e-5
    out = torch.tensor([1.5], device=DEV)
    hip.call("oneprot_sumsq", x, n, out, w)
    close(out[0], 1.5 + (x64 * x64).sum(), rt, 0.0, f"sumsq n={n}")
    out = torch.tensor([-2.0], device=DEV)
    hip.call("oneprot_abs_sum", x, out, w, n, 0.25)
    close(out[0], -2.0 + 0.25 * x64.abs().sum(), rt, 0.0, f"abs_sum n={n}")
    out = torch.tensor([4.0], device=DEV)
    hip.call("oneprot_dot_f32", x, y, out, w, n, 0.5)
    close(out[0], 4.0 + 0.5 * (x64 * y.to(F64)).sum(), rt, 0.0, f"dot n={n}")
    del x, y, x64
    free()


def test_adam_past_its_grid():
    """k_adam over 9 437 188 parameters (past 8192 x 256 x 4 = 8 388 608), three steps, weight decay and a device grad scale, against fp64 Adam arithmetic"""
    n = 9437188
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 0.01
    g = gen(9)
    p = randn(n, g)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p64, m64, v64 = p.to(F64), torch.zeros(n, dtype=F64, device=DEV), torch.zeros(n, dtype=F64, device=DEV)
    for step in (1, 2, 3):
        gr = randn(n, g, 3.0)
        gs = torch.tensor([0.5 + 0.1 * step], device=DEV)
        hip.call("oneprot_adam_step", p, gr, m, v, n, lr, b1, b2, eps, wd, step, gs)
        gg = gr.to(F64) * float(gs) + wd * p64
        m64 = b1 * m64 + (1 - b1) * gg
        v64 = b2 * v64 + (1 - b2) * gg * gg
        p64 = p64 - lr / (1 - b1 ** step) * m64 / (torch.sqrt(v64) / math.sqrt(1 - b2 ** step) + eps)
        # fp32 state: a rounding of p per step (6e-8 |p|) plus the update's own few-eps32 relative error (times lr): as test_optimizer_kernels
        close(p, p64, 1e-5, 2e-6, f"adam p step {step}")
        close(m, m64, 1e-5, 1e-6, f"adam m step {step}")
        close(v, v64, 1e-5, 1e-6, f"adam v step {step}")


def test_cast_f32_to_bf16_past_its_grid():
    n = 8388608 + 4 * 12345                                    # past 8192 x 256 x 4
    x = randn(n, gen(8), 3.0)
    x[-4:] = torch.tensor([65504.5, -1e-30, float("inf"), 3.0e38], device=DEV)
    y = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_cast_f32_to_bf16", x, y, n)
    assert torch.equal(y.view(torch.int16), x.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("B", [256, 2048])
@pytest.mark.parametrize("negative_only", [0, 1])
def test_siglip_block_large(B, negative_only):
    """oneprot_siglip_fwd_bwd (host bias) and _dev (device bias) at B up to 2048 with logits up to +-100: loss and dloss/dlogit against fp64"""
    g = gen(B + negative_only)
    logits = (torch.rand(B, B, generator=g, device=DEV) * 200 - 100)
    logits[torch.arange(B), torch.arange(B)] = torch.linspace(-100, 100, B, device=DEV)
    bias = -2.5
    z = logits.to(F64) + bias
    label = -torch.ones(B, B, dtype=F64, device=DEV)
    if not negative_only:
        label[torch.arange(B), torch.arange(B)] = 1.0
    zz = label * z
    loss_ref = -torch.nn.functional.logsigmoid(zz).sum() / B
    grad_ref = -label * torch.sigmoid(-zz) / B
    for dev_bias in (False, True):
        lg = logits.clone()
        loss = torch.tensor([0.75], device=DEV)
        rw = torch.empty(B, device=DEV)
        if dev_bias:
            hip.call("oneprot_siglip_fwd_bwd_dev", lg, loss, rw, B, torch.tensor([bias], device=DEV), negative_only)
        else:
            hip.call("oneprot_siglip_fwd_bwd", lg, loss, rw, B, bias, negative_only)
        # __expf carries ~|z| eps32 relative error at |z| <= 100; the loss is a sum of non-negative terms (B row sums of B terms each)
        close(loss[0], 0.75 + loss_ref, 2e-5, 0.0, f"siglip loss dev_bias={dev_bias}")
        close(lg, grad_ref, 2e-5, 1e-12 / B, f"siglip dlogits dev_bias={dev_bias}")


# ================================================================================================================== 3. dropout masks against Philox
N_DROP = 9000000                                               # past 4096 x 256 x 8 = 8 388 608 elements, a multiple of 8


@pytest.fixture(scope="module")
def philox_mask():
    p = 0.1
    keep = torch.from_numpy(PR.philox_keep(N_DROP, p, SEED_HI, STREAM_HI)).to(DEV)
    _, scale = PR.dropout_threshold(p)
    return p, keep, float(scale)


def test_dropout_masks_equal_philox(philox_mask):
    """every Philox dropout kernel applies exactly the reference mask, element for element, past one grid pass"""
    p, keep, scale = philox_mask
    n = N_DROP
    g = gen(11)
    zero = torch.zeros((), device=DEV)
    x = randn(n, g)
    x[x == 0] = 1.0
    xb = x.to(torch.bfloat16)
    # bf16 forward: kept = bf16(x * scale), dropped = 0
    y = torch.empty_like(xb)
    hip.call("oneprot_dropout_bf16", xb, y, n, p, SEED_HI, STREAM_HI)
    assert torch.equal(y, torch.where(keep, xb.float() * scale, zero).to(torch.bfloat16)), "dropout_bf16"
    # fp32 forward and its residual form (the select keeps the sum unfused: bit for bit, as test_dropout_f32_and_its_residual_form)
    yf = torch.empty_like(x)
    hip.call("oneprot_dropout_f32", x, yf, n, p, SEED_HI, STREAM_HI)
    ref = torch.where(keep, x * scale, zero)
    assert torch.equal(yf, ref), f"dropout_f32: {int((yf != ref).sum())} elements differ"
    resid = randn(n, g)
    hip.call("oneprot_dropout_add_f32", x, resid, yf, n, p, SEED_HI, STREAM_HI)
    assert torch.equal(yf, ref + resid), "dropout_add_f32"
    # both backward-add forms: onto zeros the result IS the masked, scaled gradient (exact); onto a live gradient, to one rounding of the sum
    d16 = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_dropout_bwd_add_bf16", xb, d16, n, p, SEED_HI, STREAM_HI)
    assert torch.equal(d16, torch.where(keep, xb.float() * scale, zero).to(torch.bfloat16)), "dropout_bwd_add_bf16 mask"
    d32 = torch.zeros(n, device=DEV)
    hip.call("oneprot_dropout_bwd_add_f32", xb, d32, n, p, SEED_HI, STREAM_HI)
    assert torch.equal(d32, torch.where(keep, xb.float() * scale, zero)), "dropout_bwd_add_f32 mask"
    base = randn(n, g)
    d32 = base.clone()
    hip.call("oneprot_dropout_bwd_add_f32", xb, d32, n, p, SEED_HI, STREAM_HI)
    close(d32, base.to(F64) + torch.where(keep, xb.to(F64) * scale, zero.to(F64)), 2e-7, 1e-6, "dropout_bwd_add_f32 onto a gradient")   # <= 2 roundings
    d16 = base.to(torch.bfloat16)
    hip.call("oneprot_dropout_bwd_add_bf16", xb, d16, n, p, SEED_HI, STREAM_HI)
    close(d16, base.to(torch.bfloat16).to(F64) + torch.where(keep, xb.to(F64) * scale, zero.to(F64)), 2 ** -8, 1e-6, "dropout_bwd_add_bf16 onto a gradient")


def test_attention_dropout_keep_equals_reference():
    """oneprot_attn_dropout_keep (the mask the attention DROP kernels regenerate per element) past its 8192 x 256 grid: 4 x 12 x 277^2 = 3.7 M elements"""
    B, H, L, p = 4, 12, 277, 0.1
    keep = torch.empty(B, H, L, L, dtype=torch.uint8, device=DEV)
    hip.call("oneprot_attn_dropout_keep", keep, B, H, L, p, SEED_HI, STREAM_HI)
    ref = torch.from_numpy(PR.attn_keep(B, H, L, p, SEED_HI, STREAM_HI)).to(DEV)
    assert torch.equal(keep.bool(), ref), f"{int((keep.bool() != ref).sum())} of {ref.numel()} keep bits differ"


# ================================================================================================================== 4. TN GEMM under a CU reserve
# cfg-2 weight gradients at T = 256 x 512 (QKV, out-projection, FFN-1, FFN-2), the 650M FFN-2 weight gradient, and ragged token counts
@pytest.mark.parametrize("M,N,K", [(131072, 1920, 640), (131072, 640, 640), (131072, 2560, 640), (131072, 640, 2560), (65536, 1280, 5120),
                                   (98336, 1920, 640), (77777, 640, 2560)])
def test_gemm_tn_under_cu_reserve(M, N, K):
    """oneprot_gemm_bf16_tn with oneprot_cu_reserve 0, 16, 64 and 200 (the last reaches the 64-CU floor): the reserve changes the token splits and with them
    the summation order; dW and dbias against fp64 from the same bf16 operands, nothing written past the workspace"""
    g = gen(M + N + K)
    dY = randn((M, N), g, 0.5, dtype=torch.bfloat16)
    X = randn((M, K), g, 0.5, dtype=torch.bfloat16)
    ref = dY.to(F64).t() @ X.to(F64)
    rb = dY.to(F64).sum(0)
    need = hip.query("oneprot_gemm_bf16_tn_workspace", N, K)
    guard = 4096
    w = torch.zeros(need + guard, dtype=torch.uint8, device=DEV)
    w[need:] = 0xA5
    dW, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    try:
        for reserve in (0, 16, 64, 200):
            hip.query("oneprot_cu_reserve", reserve)
            dW.fill_(float("nan"))
            db.fill_(float("nan"))
            hip.call("oneprot_gemm_bf16_tn", dY, X, M, N, K, N, K, dW, db, w, need, 0)
            assert bool((w[need:] == 0xA5).all()), f"reserve {reserve}: wrote past the workspace"
            # (fp32 accumulation over M products of two bf16 values: the tolerance of test_gemm_tn_large_m_every_width)
            close(dW, ref, 1e-4, 2e-3 * math.sqrt(M / 64), f"tn dW reserve {reserve}")
            close(db, rb, 1e-4, 2e-2, f"tn dbias reserve {reserve}")
    finally:
        hip.query("oneprot_cu_reserve", hip.cu_reserve_wanted())
