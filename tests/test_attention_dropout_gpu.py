"""Attention with probability dropout (oneprot_attn_fwd_dropout / oneprot_attn_bwd_dropout: k_attn_fwd<HD, true>, k_attn_bwd_dq<HD, true>,
k_attn_bwd_dkv<HD, true>) per element against fp64 torch on the GPU, computed from the bf16 inputs the kernels read and the mask that
oneprot_attn_dropout_keep exports (pinned to an independent hash by test_attention_dropout_keep_equals_reference).

Why: the BERT text tower runs these three kernels on every train-mode step (p 0.1, H 12, hd 64, L 256), and they regenerate one mask from three
register layouts (forward and dQ: a lane holds 1 query x 16 keys; dK / dV: 16 queries x 1 key).  test_attention_probability_dropout_fwd_bwd stops at
B * H = 6, three lengths, hd 32 / 64, p 0.1, a key bias always present, one norm over the launch.  Here: hd 16 / 32 / 64, ten slabs (bh 8 and 9 sit in
the second, half-empty group of eight of decode_block), 18 lengths on both sides of a 32-key tile, a 128-row block and a 256-key chunk, the tower's own
slab shape with bh up to 35, keep rates from none to 0.9, every optional argument, +-400 scores under a mask, rotary tables -- and every single mask bit
of each of the three kernels read back exactly.

Inputs as fwd_inputs of tests/test_attention_production_gpu.py (q ~ 0.7 log2 e N(0, 1), k, v ~ N(0, 1), bf16); seed and stream SEED_HI / STREAM_HI
(non-zero high words: both halves reach attn_drop_make).  Batch element 0 is unpadded, batch element 1 masks its last L // 5 keys (-inf for odd L, the
most negative float for even L).  Every output starts as NaN.

Gates (per element and per slab, never over a launch); scale = 65536 / (65536 - thr16), thr16 = round(65536 p):
  ctx   (2^-7, 1e-2 scale): the non-dropout gate (2^-7, 1e-2) of test_attention_fwd_bwd with its absolute part times scale, because every term of the row
        sum is multiplied by scale.  A CPU emulation (P rounded to bf16, masked, accumulated in fp64, output rounded to bf16; hd 16 / 64, L <= 513,
        p 0.1 / 0.5 / 0.9) stays inside it and breaks the unscaled 1e-2 at p 0.9.
  lse   (1e-4, 5e-3) against fp64, and bit for bit the lse of oneprot_attn_fwd on its split kernel (the row sum comes from the unmasked P).
  +-400 scores: ctx (2^-6, 1.5e-2 scale), lse (2e-4, 2e-2) -- test_attention_fwd_nomax_overflow_underflow_net.
  dq / dk / dv at p 0.1: per slab rel_err < 2e-2, per element (5e-2, 5e-2 max|ref| of the slab) -- tests/test_attention_production_gpu.py.
  dq / dk / dv at other p: the same with the absolute term times scale.  The fp64 reference with the kernels' roundings alone (P, keep P scale and dS
        rounded to bf16 before their products; CPU, fp64 otherwise, same construction of the inputs) against the plain fp64 reference, as a fraction of
        the gate -- worst slab rel_err / 2e-2, then worst element / its bound -- for dq, dk, dv:
          (2, 5, 257, 64)  p 0      0.092 / 0.048   0.087 / 0.035   0.074 / 0.029      (2, 5, 129, 16)  p 0      0.105 / 0.048   0.095 / 0.032   0.089 / 0.039
                           p 0.1    0.098 / 0.050   0.091 / 0.046   0.095 / 0.045                       p 0.1    0.104 / 0.053   0.092 / 0.055   0.096 / 0.032
                           p 0.25   0.095 / 0.031   0.089 / 0.029   0.097 / 0.028                       p 0.25   0.108 / 0.049   0.094 / 0.025   0.093 / 0.044
                           p 0.5    0.097 / 0.030   0.089 / 0.022   0.078 / 0.018                       p 0.5    0.109 / 0.023   0.103 / 0.021   0.086 / 0.021
                           p 0.9    0.100 / 0.005   0.101 / 0.006   0.100 / 0.006                       p 0.9    0.109 / 0.008   0.097 / 0.005   0.096 / 0.006
        (p 1e-6 is p 0.)  All far below half the gate, so the gates stand as they are.
  Rows whose valid keys are all dropped (p 0.9 at L 33; p 0.1 at L 1 / 2): ctx exactly 0.

Where the gradient reference reads ctx.  The backward forms dS = P (keep scale dP - delta) with delta = rowsum(dO ctx) from the bf16 ctx it is handed,
and that rounding (2^-9 |dO| |ctx| per row) enters dq and dk as P delta_err, which unlike the other roundings does not shrink with the gradient:
  L = 1, 2: one key has no gradient w.r.t. its score (the fp64 dq and dk are identically 0 at L = 1) and two keys at these scores are saturated; the same
        emulation with the bf16 ctx in delta is at rel_err 0.08 / 0.42 / 21.5 of the fp64 dq for hd 16 / 32 / 64 at L = 2.
  +-400 scores: the keys of extreme_rows are 4 u + 0.05 noise, and sum_k P delta_err k = delta_err (4 u + ...) is 80 times what sum_k dS k keeps of its
        terms; the emulation is at rel_err 0.033 ... 0.068 of the fp64 dq in such slabs.
In these two cases (and only there) the reference is the closed form of the same gradient, bwd_ref_reading_ctx, with delta from the ctx the call is
handed -- an input of the backward like q and k; that the closed form with the fp64 ctx IS the autograd gradient is asserted to 1e-9 on the spot, and the
ctx itself is held to fp64 by the forward gates.  The gates stay the same, except for dq in slabs with +-400 scores: there the roundings alone (table
above; same inputs' construction) reach rel_err 0.0157 ... 0.0257 per slab and 0.38 ... 0.66 of the element bound, more than half the gate, because the
32 roundings of dS in a tile multiply the common 4 u of the keys; following the rule for unmeasured gates that gate is twice the emulation's worst:
rel_err < 5.2e-2 and (6.6e-2, 6.6e-2 max|ref|).  dk and dv of those slabs (0.0008 ... 0.0054; 0.17 of the element bound) and every ordinary slab of the
same launches keep (2e-2; 5e-2, 5e-2).

Mask read-back (q = 0: every score 0, P = 1 / L exactly, lse = ln L): unit vectors in v (forward), dO (dK / dV kernel) and k (dQ kernel) make each output
element a function of ONE mask bit -- nonzero iff kept for ctx and dV, one of two values a gap q_scale scale / L apart for dQ (decoded to the nearer,
which must be within a quarter of the gap).  All B H L^2 bits of each kernel must equal the exported mask.

Mutations (scratch copies, one at a time, value / in-bounds index changes only, never committed).  NOT yet run on a GPU: the counts are of this file's 80
cases against the CPU emulation of the three kernels with the same change made in the emulation; "old" = test_attention_probability_dropout_fwd_bwd:
  1 attn_keep_bits_k with query and key swapped (dK / dV see the transposed mask)         68 cases fail (all but L 1, thr16 = 0 and the cases without a reference)
  2 forward: key0 = t * 32 without kc0                                                    23 fail (every case with L > 256); old: caught at (1, 2, 300, 64)
  3 dQ kernel: sl.head for sl.bh                                                          70 fail (all but thr16 = 0, B = 1, no reference)
  4 dK / dV kernel: dr.scale dropped from pm                                              71 fail (all but thr16 = 0, no reference)
  5 forward: 4 * h -> 0 in attn_keep_bits_q                                               65 fail (all but L <= 2 -- keys 4 .. 7 do not exist --, thr16 = 0, no reference)
  6 bh & 7 to the hash in the three DROP kernels                                          69 fail (all but thr16 = 0, B * H <= 6, no reference); old has B * H <= 6
("no reference": test_dropout_refused_arguments and test_dropout_optional_arguments_determinism_stream compare launches with each other.)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oneprot_amd import hip  # noqa: E402
from oracle import oneprot_oracle as O  # noqa: E402
from tests import philox_ref as PR  # noqa: E402
from tests.attn_cases import CTX_GATE, CTX_GATE_X, LSE_GATE, LSE_GATE_X, extreme_rows, fwd_inputs, run_fwd  # noqa: E402    (2^-7, 1e-2), (2^-6, 1.5e-2) x scale; (1e-4, 5e-3), (2e-4, 2e-2)
from tests.attn_ref import bhld, bwd_ref, bwd_ref_reading_ctx, fwd_ref, rot_half  # noqa: E402
from tests.cases import DEV, SEED_HI, STREAM_HI, bf, gen, randn, ws  # noqa: E402
from tests.gate import close  # noqa: E402

F64 = torch.float64
NEG_MIN = torch.finfo(torch.float32).min
NAN = float("nan")

EDGE_LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 777]


def thr_scale(p):
    """thr16 and the scale of kept probabilities as attn_drop_make forms them in fp32"""
    thr, scale = PR.dropout_threshold(p)
    return thr, float(scale)


def drop_bias(B, L):
    """fp32 [B, L]: batch element 0 unpadded; the others mask their last L // 5 keys, -inf or the most negative float (the header admits either)"""
    bias = torch.zeros(B, L)
    for b in range(1, B):
        if L >= 5:
            bias[b, L - L // 5:] = float("-inf") if (L + b) % 2 == 0 else NEG_MIN          # b = 1: -inf for odd L
    return bias.to(DEV)


def export_keep(B, H, L, p, seed=SEED_HI, stream=STREAM_HI):
    keep = torch.full((B, H, L, L), 7, dtype=torch.uint8, device=DEV)
    hip.call("oneprot_attn_dropout_keep", keep, B, H, L, p, seed, stream)
    assert int(keep.max()) <= 1
    return keep.bool()


def run_fwd_drop(q, k, v, bias, p, seed=SEED_HI, stream=STREAM_HI, with_lse=True):
    B, H, L, hd = q.shape
    ctx = torch.full((B * L, H * hd), NAN, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, L), NAN, device=DEV) if with_lse else None
    hip.call("oneprot_attn_fwd_dropout", q, k, v, bias, ctx, lse, B, H, L, hd, p, seed, stream)
    return ctx, lse


def run_fwd_split(q, k, v, bias):
    """oneprot_attn_fwd on k_attn_fwd<HD, false>: the body the dropout forward shares"""
    hip.query("oneprot_attn_force_fwd_path", 0)
    try:
        return run_fwd(q, k, v, bias)
    finally:
        hip.query("oneprot_attn_force_fwd_path", -1)


def run_bwd_drop(q, k, v, bias, ctx, dctx, lse, p, q_scale, cosd=None, sind=None, seed=SEED_HI, stream=STREAM_HI):
    """dq, dk, dv as [3, B, H, L, hd] (views of the bf16 dqkv the call wrote over NaN)"""
    B, H, L, hd = q.shape
    dqkv = torch.full((B * L, 3 * H * hd), NAN, dtype=torch.bfloat16, device=DEV)
    w = ws(hip.query("oneprot_attn_bwd_workspace", B, H, L))
    hip.call("oneprot_attn_bwd_dropout", q, k, v, bias, ctx, dctx, lse, cosd, sind, q_scale, dqkv, w, B, H, L, hd, p, seed, stream)
    return dqkv.view(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)


def run_bwd_split(q, k, v, bias, ctx, dctx, lse, q_scale):
    B, H, L, hd = q.shape
    dqkv = torch.full((B * L, 3 * H * hd), NAN, dtype=torch.bfloat16, device=DEV)
    w = ws(hip.query("oneprot_attn_bwd_workspace", B, H, L))
    hip.query("oneprot_attn_force_bwd_path", 0)
    try:
        hip.call("oneprot_attn_bwd", q, k, v, bias, ctx, dctx, lse, None, None, q_scale, dqkv, w, B, H, L, hd)
    finally:
        hip.query("oneprot_attn_force_bwd_path", -1)
    return dqkv.view(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)


GRAD_GATE = (2e-2, 5e-2, 5e-2)                  # per slab rel_err; per element (rtol, atol / max|ref of the slab|)
GRAD_GATE_XQ = (5.2e-2, 6.6e-2, 6.6e-2)         # dq of a slab with +-400 scores: twice the emulation's figures (the file's docstring)


def grad_gates(got, ref, name, atol_scale=1.0, xslab=None, gate_x=GRAD_GATE):
    """got / ref [B, H, rows, hd]: per slab rel_err < 2e-2 and |err| <= 5e-2 |ref| + 5e-2 atol_scale max|ref of the slab|; gate_x in the slabs of xslab"""
    got = got.to(F64)
    if xslab is None:
        xslab = torch.zeros(ref.shape[:2], dtype=torch.bool, device=ref.device)
    g = [torch.where(xslab, torch.tensor(gate_x[i], dtype=F64, device=ref.device), torch.tensor(GRAD_GATE[i], dtype=F64, device=ref.device)) for i in range(3)]
    rel = (got - ref).flatten(2).norm(dim=-1) / (ref.flatten(2).norm(dim=-1) + 1e-20)
    print(f"{name}: worst slab rel_err {float(torch.nan_to_num(rel, nan=9.9).max()):.3e}" + (f", with +-400 scores {float(torch.nan_to_num(rel[xslab], nan=9.9).max()):.3e}" if bool(xslab.any()) else ""))
    ok = rel < g[0]
    assert bool(ok.all()), f"{name}: rel err {float(torch.nan_to_num(rel, nan=9.9)[~ok].max()):.3e} in slab {tuple(int(i) for i in (~ok).nonzero()[0])}"
    close(got, ref, g[1][:, :, None, None], (g[2] * atol_scale * ref.abs().flatten(2).amax(-1))[..., None, None], name)


def slab_gate(gate, gate_x, xslab, mult=1.0):
    """(rtol, atol) as [B, H, 1, 1]: gate_x in the slabs of the bool [B, H] xslab, gate elsewhere; the absolute part times mult"""
    f = lambda i, m: torch.where(xslab, torch.tensor(gate_x[i] * m, dtype=F64, device=DEV), torch.tensor(gate[i] * m, dtype=F64, device=DEV))[:, :, None, None]
    return f(0, 1.0), f(1, mult)


def check_case(q, k, v, bias, dctx, p, cosd=None, sind=None, xslab=None, atol_scale=1.0, tag=""):
    """forward and backward of one set of inputs against fp64 under the file's gates; returns (ctx, lse, grads [3, B, H, L, hd], keep)"""
    B, H, L, hd = q.shape
    thr, scale = thr_scale(p)
    q_scale = hd ** -0.5
    keep = export_keep(B, H, L, p)
    if xslab is None:
        xslab = torch.zeros(B, H, dtype=torch.bool, device=DEV)
    ctx, lse = run_fwd_drop(q, k, v, bias, p)
    o_ref, lse_ref = fwd_ref(q, k, v, bias, keep, scale)
    got_ctx = bhld(ctx, B, H, L, hd)
    rt, at = slab_gate(CTX_GATE, CTX_GATE_X, xslab, scale)
    close(got_ctx, o_ref, rt, at, f"ctx [b, h, l, d] {tag}")
    rt, at = slab_gate(LSE_GATE, LSE_GATE_X, xslab)
    close(lse, lse_ref, rt[..., 0], at[..., 0], f"lse [b, h, l] {tag}")
    valid = (bias > -1.0e30) if bias is not None else torch.ones(B, L, dtype=torch.bool, device=DEV)
    dead = ~(keep & valid[:, None, None, :]).any(-1)                                       # [B, H, L]: rows whose valid keys are all dropped
    assert bool((got_ctx[dead] == 0).all()), f"{tag}: a ctx row with every key dropped is not exactly zero"
    # the row sum and the lse are those of the plain forward: the two are one body
    ctx0, lse0 = run_fwd_split(q, k, v, bias)
    assert torch.equal(lse, lse0), f"{tag}: the undropped lse differs from oneprot_attn_fwd's"
    if thr == 0:
        assert torch.equal(ctx, ctx0), f"{tag}: thr16 = 0 is no dropout, ctx must be oneprot_attn_fwd's"
    cos = sin = None
    if cosd is not None:
        cos, sin = torch.cat([cosd, cosd], -1).to(F64), torch.cat([sind, sind], -1).to(F64)      # the fp32 tables the kernel reads
    got = run_bwd_drop(q, k, v, bias, ctx, dctx, lse, p, q_scale, cosd, sind)
    assert bool(torch.isfinite(got.float()).all()), f"{tag}: non-finite or unwritten gradient"
    refs = bwd_ref(q, k, v, bias, dctx, q_scale, cos, sin, keep, scale)
    if L <= 2 or bool(xslab.any()):
        # (the file's docstring) the gradient is small against 2^-9 |dO| |ctx| here: delta from the bf16 ctx the call is handed, as the kernels form it
        closed = bwd_ref_reading_ctx(q, k, v, bias, o_ref, dctx, keep, scale, q_scale, cos, sin)
        for a, b in zip(closed, refs):
            assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max()) + 1e-12, "the closed form is not the autograd gradient"
        refs = bwd_ref_reading_ctx(q, k, v, bias, got_ctx.to(F64), dctx, keep, scale, q_scale, cos, sin)
    for i, name in enumerate(("dq", "dk", "dv")):
        grad_gates(got[i], refs[i], f"{name} {tag}", atol_scale, xslab, GRAD_GATE_XQ if i == 0 else GRAD_GATE)
    if bias is not None and bool((~valid).any()):
        assert float(got[1:].float().abs().amax((0, 2, 4))[~valid].max()) == 0.0, f"{tag}: dK / dV of a masked key is not exactly zero"
    return ctx, lse, got, keep, (ctx0, lse0), refs


def make_case(B, H, L, hd, seed, padded=True):
    q, k, v = fwd_inputs(B, H, L, hd, seed)
    dctx = randn((B * L, H * hd), gen(seed + 1), 1.0, dtype=torch.bfloat16)
    return q, k, v, (drop_bias(B, L) if padded else None), dctx


# ====================================================================================================== 1. edge matrix
@pytest.mark.parametrize("L", EDGE_LENGTHS)
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_dropout_edge_lengths_ten_slabs(hd, L):
    """B 2, H 5 (ten slabs: bh 8 and 9 in the half-empty second group of eight), p 0.1: ctx, lse, dq, dk, dv against fp64 per element / per slab"""
    B, H = 2, 5
    q, k, v, bias, dctx = make_case(B, H, L, hd, 7000 + 3 * L + hd)
    check_case(q, k, v, bias, dctx, 0.1, tag=f"L {L} hd {hd}")


# ====================================================================================================== 2. the text tower's slab shape
def test_dropout_text_tower_slab_shape():
    """B 3, H 12, L 256, hd 64, p 0.1: the slab BERT-base runs at L 256 (one work-group per (slab, block): the batch need not be the bench's), bh up to 35"""
    B, H, L, hd = 3, 12, 256, 64
    q, k, v, bias, dctx = make_case(B, H, L, hd, 7101)
    check_case(q, k, v, bias, dctx, 0.1, tag="B 3 H 12 L 256 hd 64")


# ====================================================================================================== 3. keep rates
SWEEP_SHAPES = [(2, 5, 257, 64), (2, 5, 129, 16)]


@pytest.mark.parametrize("p", [0.0, 1e-6, 0.25, 0.5, 0.9])
@pytest.mark.parametrize("B,H,L,hd", SWEEP_SHAPES)
def test_dropout_keep_rates(B, H, L, hd, p):
    """p 0 and 1e-6 (thr16 = 0: no dropout, ctx bit for bit the plain forward's) to 0.9 (scale 10); the gradient gates' absolute term times scale.
    At thr16 = 0 the split backward of oneprot_attn_bwd computes the same function (not the same bits: -delta enters through a bf16-split MFMA step
    there and through VALU here) and is held to the same fp64 reference under the same gates."""
    thr, scale = thr_scale(p)
    assert (thr == 0) == (p < 2.0 ** -17)
    q, k, v, bias, dctx = make_case(B, H, L, hd, 7200 + L)
    ctx, lse, got, keep, _, refs = check_case(q, k, v, bias, dctx, p, atol_scale=scale, tag=f"p {p} L {L} hd {hd}")
    assert abs(float(keep.float().mean()) - (1.0 - thr / 65536.0)) < 0.01
    if thr == 0:
        assert bool(keep.all())
        plain = run_bwd_split(q, k, v, bias, ctx, dctx, lse, hd ** -0.5)
        for i, name in enumerate(("dq", "dk", "dv")):
            grad_gates(plain[i], refs[i], f"oneprot_attn_bwd {name} p {p} L {L} hd {hd}")


@pytest.mark.parametrize("B,H,L,hd", SWEEP_SHAPES)
def test_dropout_refused_arguments(B, H, L, hd):
    """p < 0, p = 1, NaN, and 0.999995 (rounds to thr16 = 65536: nothing kept) are refused by all three entry points, as is hd 48; nothing is written"""
    def calls(hd_, p):
        q, k, v, bias, dctx = make_case(B, H, L, hd_, 7300)
        ctx = torch.full((B * L, H * hd_), NAN, dtype=torch.bfloat16, device=DEV)
        lse = torch.full((B, H, L), NAN, device=DEV)
        dqkv = torch.full((B * L, 3 * H * hd_), NAN, dtype=torch.bfloat16, device=DEV)
        keep = torch.full((B, H, L, L), 7, dtype=torch.uint8, device=DEV)
        w = ws(hip.query("oneprot_attn_bwd_workspace", B, H, L))
        yield "fwd", lambda: hip.call("oneprot_attn_fwd_dropout", q, k, v, bias, ctx, lse, B, H, L, hd_, p, SEED_HI, STREAM_HI), ctx
        yield "bwd", lambda: hip.call("oneprot_attn_bwd_dropout", q, k, v, bias, q.new_zeros(B * L, H * hd_), dctx, lse.new_zeros(B, H, L), None, None, hd_ ** -0.5,
                                      dqkv, w, B, H, L, hd_, p, SEED_HI, STREAM_HI), dqkv
        if hd_ == hd:
            yield "keep", lambda: hip.call("oneprot_attn_dropout_keep", keep, B, H, L, p, SEED_HI, STREAM_HI), keep

    for p in (-0.1, 1.0, NAN, 0.999995):
        if p == 0.999995:
            assert int(torch.tensor(p, dtype=torch.float32) * 65536.0 + 0.5) == 65536          # fp32, as attn_drop_make rounds it
        for name, fn, out in calls(hd, p):
            with pytest.raises(hip.HipKernelError):
                fn()
            assert bool((out == 7).all() if out.dtype == torch.uint8 else torch.isnan(out.float()).all()), f"{name} p {p}: a refused call wrote its output"
    for name, fn, out in calls(48, 0.1):
        with pytest.raises(hip.HipKernelError):
            fn()
        assert bool(torch.isnan(out.float()).all()), f"{name} hd 48: a refused call wrote its output"


def test_dropout_rows_with_every_key_dropped():
    """p 0.9 at L 33 and hd 32: about 3 % of the rows keep none of their keys; their ctx is exactly 0 (asserted in check_case) and the gradients hold"""
    B, H, L, hd, p = 2, 5, 33, 32, 0.9
    q, k, v, bias, dctx = make_case(B, H, L, hd, 7400)
    ctx, lse, got, keep, _, _ = check_case(q, k, v, bias, dctx, p, atol_scale=thr_scale(p)[1], tag="p 0.9 L 33")
    dead = ~(keep & (bias > -1.0e30)[:, None, None, :]).any(-1)
    assert int(dead.sum()) >= 3, "the case holds no row with every key dropped"
    assert float(got[0][dead].float().abs().max()) == 0.0, "dq of a row with every key dropped (dS = P (0 - 0))"


# ====================================================================================================== 4. exact identities
@pytest.mark.parametrize("B,H,L,hd", SWEEP_SHAPES + [(2, 5, 300, 32)])
def test_dropout_optional_arguments_determinism_stream(B, H, L, hd):
    """lse = NULL gives the same ctx bits; key_bias = NULL the bits of an all-zero bias, forward and backward; two launches are bit-equal; another stream_id
    (and another seed) changes ctx.  (The lse and thr16 = 0 identities with oneprot_attn_fwd are asserted in every case of check_case.)"""
    p, q_scale = 0.1, hd ** -0.5
    q, k, v, bias, dctx = make_case(B, H, L, hd, 7500 + hd)
    ctx, lse = run_fwd_drop(q, k, v, bias, p)
    assert not bool(torch.isnan(ctx.float()).any()) and not bool(torch.isnan(lse).any())
    ctx2, lse2 = run_fwd_drop(q, k, v, bias, p)
    assert torch.equal(ctx2, ctx) and torch.equal(lse2, lse), "two launches of the forward differ"
    ctx3, _ = run_fwd_drop(q, k, v, bias, p, with_lse=False)
    assert torch.equal(ctx3, ctx), "lse = NULL changes ctx"
    for other in (dict(stream=STREAM_HI + 1), dict(stream=STREAM_HI ^ (1 << 40)), dict(seed=SEED_HI ^ (1 << 33))):
        ctx4, lse4 = run_fwd_drop(q, k, v, bias, p, **other)
        assert torch.equal(lse4, lse) and not torch.equal(ctx4, ctx), f"{other}: the mask must change and the lse must not"
    g1 = run_bwd_drop(q, k, v, bias, ctx, dctx, lse, p, q_scale)
    g2 = run_bwd_drop(q, k, v, bias, ctx, dctx, lse, p, q_scale)
    assert not bool(torch.isnan(g1.float()).any()) and torch.equal(g1, g2), "two launches of the backward differ"
    zero = torch.zeros(B, L, device=DEV)
    ctx_z, lse_z = run_fwd_drop(q, k, v, zero, p)
    ctx_n, lse_n = run_fwd_drop(q, k, v, None, p)
    assert torch.equal(ctx_n, ctx_z) and torch.equal(lse_n, lse_z), "key_bias = NULL is not an all-zero bias (forward)"
    assert not torch.equal(ctx_n, ctx)
    g_z = run_bwd_drop(q, k, v, zero, ctx_z, dctx, lse_z, p, q_scale)
    g_n = run_bwd_drop(q, k, v, None, ctx_z, dctx, lse_z, p, q_scale)
    assert not bool(torch.isnan(g_z.float()).any()) and torch.equal(g_n, g_z), "key_bias = NULL is not an all-zero bias (backward)"


# ====================================================================================================== 5. every mask bit of every kernel
def _unit_window(shape, w0, n):
    """zeros [B, H, L, hd] with x[:, :, w0 + j, j] = 1 for j < n"""
    x = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    j = torch.arange(n, device=DEV)
    x[:, :, w0 + j, j] = 1.0
    return x


@pytest.mark.parametrize("L,hd,p", [(33, 16, 0.1), (129, 32, 0.1), (257, 64, 0.1), (513, 16, 0.1), (257, 64, 0.5)])
def test_dropout_mask_bits_of_all_three_kernels(L, hd, p):
    B, H = 2, 5
    shape = (B, H, L, hd)
    thr, scale = thr_scale(p)
    q_scale = hd ** -0.5
    keep = export_keep(B, H, L, p)
    assert abs(float(keep.float().mean()) - (1.0 - thr / 65536.0)) < 0.01 and not bool(keep.all())
    g = gen(7600 + L)
    q0 = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    k_any, v_any = randn(shape, g, 1.0, dtype=torch.bfloat16), randn(shape, g, 1.0, dtype=torch.bfloat16)
    unit = scale / L                                                  # keep * scale * P with P = 1 / L
    windows = [(w0, min(hd, L - w0)) for w0 in range(0, L, hd)]
    assert len(windows) <= 33

    def unit_values(x, what):
        nz = x[x != 0].to(F64)
        assert bool(((nz - unit).abs() <= 2 ** -7 * unit).all()), f"{what}: a kept element is not scale / L = {unit:.6g}"

    # forward: v[k_j, :] = e_j on a window of keys  =>  ctx[q, j] = keep[q, k_j] scale / L
    seen = torch.zeros_like(keep)
    for w0, n in windows:
        ctx, lse = run_fwd_drop(q0, k_any, _unit_window(shape, w0, n), None, p)
        c = bhld(ctx, B, H, L, hd)
        assert bool(torch.isfinite(c.float()).all()) and bool((c[..., n:] == 0).all())
        close(lse, torch.full((B, H, L), math.log(L), dtype=F64, device=DEV), *LSE_GATE, f"lse = ln L, window {w0}")
        unit_values(c, f"ctx, key window {w0}")
        seen[:, :, :, w0:w0 + n] = c[..., :n] != 0
    bad = seen != keep
    assert not bool(bad.any()), f"forward: {int(bad.sum())} mask bits differ, first (b, h, q, k) = {tuple(int(i) for i in bad.nonzero()[0])}"

    # dK / dV kernel: dO[q_j, :] = e_j on a window of queries  =>  dV[k, j] = keep[q_j, k] scale / L
    ctx, lse = run_fwd_drop(q0, k_any, v_any, None, p)
    seen = torch.zeros_like(keep)
    for w0, n in windows:
        dctx = _unit_window(shape, w0, n).permute(0, 2, 1, 3).reshape(B * L, H * hd).contiguous()
        dv = run_bwd_drop(q0, k_any, v_any, None, ctx, dctx, lse, p, q_scale)[2]
        assert bool(torch.isfinite(dv.float()).all()) and bool((dv[..., n:] == 0).all())
        unit_values(dv, f"dV, query window {w0}")
        seen[:, :, w0:w0 + n, :] = (dv[..., :n] != 0).transpose(-1, -2)
    bad = seen != keep
    assert not bool(bad.any()), f"dK / dV kernel: {int(bad.sum())} mask bits differ, first (b, h, q, k) = {tuple(int(i) for i in bad.nonzero()[0])}"

    # dQ kernel: k[k_j, :] = e_j on a window of keys, v[k, :] = e_0, dO[q, :] = e_0  =>  dQ[q, j] = q_scale (keep[q, k_j] scale - delta_q) / L
    e0 = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    e0[..., 0] = 1.0
    dctx = e0.permute(0, 2, 1, 3).reshape(B * L, H * hd).contiguous()
    ctx, lse = run_fwd_drop(q0, k_any, e0, None, p)                    # (k does not matter to a forward with q = 0)
    delta = bhld(ctx, B, H, L, hd)[..., 0].to(F64)[..., None]         # [B, H, L, 1]: rowsum(dO * ctx) as the kernel forms it
    kept_v, drop_v, gap = q_scale * (scale - delta) / L, q_scale * (0.0 - delta) / L, q_scale * scale / L
    seen = torch.zeros_like(keep)
    for w0, n in windows:
        dq = run_bwd_drop(q0, _unit_window(shape, w0, n), e0, None, ctx, dctx, lse, p, q_scale)[0]
        assert bool(torch.isfinite(dq.float()).all()) and bool((dq[..., n:] == 0).all())
        d = dq[..., :n].to(F64)
        dk_, dd_ = (d - kept_v).abs(), (d - drop_v).abs()
        far = torch.minimum(dk_, dd_) >= gap / 4
        assert not bool(far.any()), f"dQ, key window {w0}: {int(far.sum())} elements are neither value, worst {float(torch.minimum(dk_, dd_).max()):.3e} of a gap {gap:.3e}"
        seen[:, :, :, w0:w0 + n] = dk_ < dd_
    bad = seen != keep
    assert not bool(bad.any()), f"dQ kernel: {int(bad.sum())} mask bits differ, first (b, h, q, k) = {tuple(int(i) for i in bad.nonzero()[0])}"


# ====================================================================================================== 6. extreme scores under a mask
@pytest.mark.parametrize("B,H,L,hd", [(2, 5, 300, 64), (2, 5, 512, 32)])
def test_dropout_extreme_scores(B, H, L, hd):
    """the +-400 rows of extreme_rows in slabs of both groups of eight (the forward rescales its accumulators while the masked copy of P is live), the
    other slabs ordinary and under the ordinary gates"""
    q, k, v, bias, dctx = make_case(B, H, L, hd, 7700 + L)
    xslab = extreme_rows(q, k, [1, 4, 6, 8, 9], gen(7701 + L))
    check_case(q, k, v, bias, dctx, 0.1, xslab=xslab, tag=f"extreme L {L} hd {hd}")


# ====================================================================================================== 7. rotary tables
@pytest.mark.parametrize("B,H,L,hd", [(2, 3, 45, 32), (1, 2, 70, 64)])
def test_dropout_bwd_rope_chain(B, H, L, hd):
    """oneprot_attn_bwd_dropout with rotary tables: dqkv is the gradient w.r.t. the un-rotated, un-scaled projections (test_attention_bwd_rope_chain with
    the mask), against fp64 autograd through the rotation"""
    g = gen(7800 + L)
    ylin = torch.randn(3, B, H, L, hd, generator=g, device=DEV)
    cos, sin = O.rope_tables(L, hd)
    cosd, sind = cos[:, : hd // 2].contiguous().to(DEV), sin[:, : hd // 2].contiguous().to(DEV)
    c, s = torch.cat([cosd, cosd], -1), torch.cat([sind, sind], -1)
    rot = lambda x: x * c + rot_half(x) * s
    q = bf(rot(ylin[0] * hd ** -0.5) * hip.LOG2E)
    k, v = bf(rot(ylin[1])), bf(ylin[2])
    dctx = randn((B * L, H * hd), g, 1.0, dtype=torch.bfloat16)
    check_case(q, k, v, drop_bias(B, L), dctx, 0.1, cosd=cosd, sind=sind, tag=f"rope L {L} hd {hd}")
