"""Attention and the persistent NT GEMM at the launch sizes of the training step (bench.py cfg-2: q / k / v [256, 20, 512, 32], FFN-1 131072 x 2560 x 640),
against fp64 torch on the GPU computed from the bf16-rounded inputs the kernel reads, in chunks of a few batch elements / 8192 GEMM rows.

Why: k_attn_fwd3 / k_attn_fwd3w are one persistent work-group per CU; a work-group WALKS several (b, h) slabs and everything delicate about them -- the
LDS-DMA of slab n + 1 into the other half of the LDS, slab n + 1's q fragments and key bias (another batch element), the deferred stores of slab n - 1, the
chunk stream of the hd-64 form that runs across slab boundaries, the per-slab redo marks -- only runs when a work-group has at least two slabs, i.e. with
B * H > 256.  The other kernel tests stop at B * H = 128 or compare such a launch with itself.  The same holds for k_gemm8 beyond three tiles per work-group
and for the packed (varlen) kernels beyond H = 2.

Gates are the project's own (tests/test_kernels_gpu.py, tests/test_packed_gpu.py: the same kernels against fp32 torch), applied per slab / per segment /
per row chunk, never over a whole launch:
  ctx (2^-7, 1e-2), lse (1e-4, 5e-3); with +-400 scores (2^-6, 1.5e-2) / (2e-4, 2e-2); dq / dk / dv rel_err < 2e-2 and (5e-2, 5e-2 max|ref|) per slab;
  the GEMM epilogues as test_gemm_nt_epilogues / test_gemm_qkv_rope_epilogue; varlen forward 3e-2 abs ctx, 1e-2 lse per segment.
Reference-free on top: a slab's arithmetic does not depend on where in a walk it runs, so the big launch equals, bit for bit, the same inputs launched
in batch slices small enough that every work-group has one slab; work queues equal static lists bit for bit.

Key padding: one pattern per batch element from a seeded generator (PATTERNS); the seed is searched on the host so that, along the static walks
(bh = xcd * per_xcd + slot, + nslot, ...), at least three quarters of the neighbouring slabs differ in pattern and an unpadded slab is directly followed
by the two-key one and the reverse.

Mutations these tests were run against (one at a time, value / in-bounds index changes only; "parent" = the attention / GEMM / packed tests of
tests/test_kernels_gpu.py + tests/test_packed_gpu.py as they were before this file; a test that consumes a wrong forward -- the backward cases, the QKV chain
-- fails with it):
  1 k_attn_fwd3: the next slab's bias piece read from the current slab's batch element (nxt / H -> bh / H)
      here: bench launch, all 12 slab-count cases, forced path 1, extreme hd 32, QKV chain (+ 7 backward cases); parent: no kernel test, two packed-vs-padded step tests
  2 k_attn_fwd3: the deferred stores of query block 1 skipped from the third slab of a walk on (slab_no >= 2)
      here: bench launch, 513 / 520 slabs, forced path 1, extreme hd 32, QKV chain (NaN rows); parent: only the co-residency test (queues vs static lists on uninitialised outputs)
  3 k_attn_fwd3: bh_end one short for the last XCD
      here: every k_attn_fwd3 case (NaN rows of the last slab; the sched error word, sticky, then fails the later queue cases too); parent: co-residency test, five step tests
  4 k_attn_fwd3w: the redo mark written at bh - 1 for slabs that are not first in their walk
      here: extreme scores hd 64, both lengths, and the launch of REDO_SLABS slabs; parent: nothing
  5 k_attn_varlen_bwd_dkv: lse / delta read without the head offset for head >= 2
      here: all three packed cases (dk of head 2, rel err above 80); parent: no kernel test (H = 2), four packed step tests
  6 k_gemm8: accumulators of a work-group's 8th and later tiles start at 0.25 instead of 0 (the zero_acc() behind the epilogue), static lists only
      here: FFN-1 at 131072 and 131328 rows, the 650M FFN-1, the QKV GEMM; parent: the two queue-vs-static comparisons
    the same in both modes: here the same four, against fp64 (gelu off by 0.29, q by 0.10); parent: only the co-residency test (the queues hand a disturbed launch other tiles)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oneprot_amd import hip  # noqa: E402
from oneprot_amd.packing import PackedTokens  # noqa: E402
from oracle import oneprot_oracle as O  # noqa: E402
from tests import attn_ref as AR  # noqa: E402
from tests.attn_cases import CTX_GATE, CTX_GATE_X, LSE_GATE, LSE_GATE_X, extreme_rows, fwd_inputs, run_fwd  # noqa: E402,F401
from tests.attn_ref import rot_half  # noqa: E402
from tests.cases import DEV, bf, cu as cu_of, free, gathered_tables, gen, randn, ws  # noqa: E402
from tests.gate import close  # noqa: E402

F64 = torch.float64
NEG_MIN = torch.finfo(torch.float32).min
REDO_SLABS = 32768                                                  # csrc/attention.hip: slabs the hd-64 persistent kernel keeps marks for

def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ====================================================================================================== key padding along the walks
PATTERNS = ("none", 2, 33, 389, 256, 479, 511, "hole")             # valid length, or: keys 64 .. 127 masked and the rest valid
P_NONE, P_TWO = 0, 1


def walks(nbh, n_cu):
    """the static slab lists of k_attn_fwd3 / k_attn_fwd3w: work-group (xcd, slot) walks xcd * per_xcd + slot, + nslot, ... inside its XCD's eighth"""
    per_xcd = (nbh + 7) // 8
    nslot = max(1, min(n_cu // 8, per_xcd))
    out = []
    for x in range(8):
        end = min(nbh, (x + 1) * per_xcd)
        for s in range(nslot):
            w = list(range(x * per_xcd + s, end, nslot))
            if w:
                out.append(w)
    return out


def _walk_condition(ids, H, wk):
    pairs = [(ids[a // H], ids[b // H]) for w in wk for a, b in zip(w[:-1], w[1:])]
    differ = sum(1 for a, b in pairs if a != b)
    return bool(pairs) and 4 * differ >= 3 * len(pairs) and (P_NONE, P_TWO) in pairs and (P_TWO, P_NONE) in pairs and len(set(ids)) == len(PATTERNS)


def pick_patterns(B, H, n_cu, seed0=1000):
    """pattern index per batch element from torch.Generator(seed); the first seed >= seed0 for which the condition on the walks holds"""
    wk = walks(B * H, n_cu)
    for seed in range(seed0, seed0 + 20000):
        ids = torch.randint(0, len(PATTERNS), (B,), generator=torch.Generator().manual_seed(seed)).tolist()
        if _walk_condition(ids, H, wk):
            return ids
    raise AssertionError(f"no seed gives the padding patterns the walks of B = {B}, H = {H} need")


def key_bias(ids, L):
    """fp32 [B, L]: 0 valid; masked keys -inf (even batch elements) or the most negative float (odd ones) -- the header admits either"""
    bias = torch.zeros(len(ids), L)
    for b, p in enumerate(ids):
        neg = float("-inf") if b % 2 == 0 else NEG_MIN
        pat = PATTERNS[p]
        if pat == "none":
            continue
        if pat == "hole":
            lo, hi = (64, 128) if L > 128 else (L // 4, L // 2)
            bias[b, lo:hi] = neg
        else:
            bias[b, min(pat, L):] = neg
    return bias.to(DEV)


def padded_case(B, H, L):
    ids = pick_patterns(B, H, _n_cu())
    assert _walk_condition(ids, H, walks(B * H, _n_cu()))
    return key_bias(ids, L)


# ====================================================================================================== fp64 references
def attn_ref(q, k, v, bias, b0, b1):
    """fp64 softmax(q k^T ln 2 + bias) v of batch elements [b0, b1): ctx as [(b1 - b0) * L, H * hd] and lse [b1 - b0, H, L]; q is in log2 units"""
    H, L, hd = q.shape[1:]
    o, lse = AR.fwd_ref(q[b0:b1], k[b0:b1], v[b0:b1], None if bias is None else bias[b0:b1])
    return o.permute(0, 2, 1, 3).reshape((b1 - b0) * L, H * hd), lse


def check_fwd(outs, q, k, v, bias, extreme=None, tag=""):
    """every (name, ctx, lse) of `outs` against fp64, a chunk of batch elements at a time (scores of a chunk <= 1 GB); element-wise gates, so per slab.
    extreme: bool [B, H], slabs that hold +-400 scores and are held to the gates of the extreme-score test; every other slab to the ordinary ones"""
    B, H, L, hd = q.shape
    bc = max(1, int(1.0e9 // (H * L * L * 8)))
    for b0 in range(0, B, bc):
        b1 = min(B, b0 + bc)
        o_ref, lse_ref = attn_ref(q, k, v, bias, b0, b1)
        x = extreme[b0:b1] if extreme is not None else torch.zeros(b1 - b0, H, dtype=torch.bool, device=DEV)
        gate = lambda g, gx: [torch.where(x, torch.tensor(gx[i], dtype=F64, device=DEV), torch.tensor(g[i], dtype=F64, device=DEV)) for i in range(2)]
        (c_rt, c_at), (l_rt, l_at) = gate(CTX_GATE, CTX_GATE_X), gate(LSE_GATE, LSE_GATE_X)
        for name, ctx, lse in outs:
            close(ctx[b0 * L:b1 * L].view(b1 - b0, L, H, hd), o_ref.view(b1 - b0, L, H, hd), c_rt[:, None, :, None], c_at[:, None, :, None],
                  f"ctx {tag} {name} [b, l, h, d] from b0 = {b0}")
            close(lse[b0:b1], lse_ref, l_rt[:, :, None], l_at[:, :, None], f"lse {tag} {name} [b, h, l] from b0 = {b0}")
        del o_ref, lse_ref


class tiles_mode:
    """static slab / tile lists (False) or the work queues of the sched workspace (True); the process-wide setting restored as test_kernels_gpu.py does"""

    def __init__(self):
        self.ws = hip.sched_workspace(131072)

    def set(self, dynamic):
        hip.query("oneprot_dynamic_tiles", self.ws[0] if dynamic else None, self.ws[1] if dynamic else 0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        hip.query("oneprot_dynamic_tiles", self.ws[0] if hip.dynamic_tiles_wanted() else None, self.ws[1])
        return False


def sliced_fwd(q, k, v, bias, nb):
    """the same inputs launched nb batch elements at a time (nb * H <= 256: every work-group has one slab)"""
    B, H, L, hd = q.shape
    assert nb * H <= 256
    ctx = torch.full((B * L, H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, L), float("nan"), device=DEV)
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        hip.call("oneprot_attn_fwd", q[b0:b0 + n], k[b0:b0 + n], v[b0:b0 + n], bias[b0:b0 + n], ctx[b0 * L:(b0 + n) * L], lse[b0:b0 + n], n, H, L, hd)
    return ctx, lse


# ====================================================================================================== A. forward where work-groups walk several slabs
def test_fwd_bench_launch_hd32():
    """A.1 + A.6: hd 32, L 512, B 256, H 20 -- 5120 slabs, 20 per work-group of k_attn_fwd3 -- static lists and work queues against fp64 per slab, the two
    bit for bit equal, and bit for bit equal to the same inputs launched 12 batch elements (240 slabs: one per work-group) at a time"""
    B, H, L, hd = 256, 20, 512, 32
    bias = padded_case(B, H, L)
    q, k, v = fwd_inputs(B, H, L, hd, 101)
    with tiles_mode() as tm:
        tm.set(False)
        ctx, lse = run_fwd(q, k, v, bias)
        ctx_s, lse_s = sliced_fwd(q, k, v, bias, 12)
        tm.set(True)
        ctx_d, lse_d = run_fwd(q, k, v, bias)
        ctx_d2, lse_d2 = run_fwd(q, k, v, bias)
    assert hip.sched_error() == 0
    check_fwd([("static", ctx, lse), ("queues", ctx_d, lse_d)], q, k, v, bias, tag="bench launch")
    assert torch.equal(ctx_d, ctx) and torch.equal(lse_d, lse), "work queues differ from static lists"
    assert torch.equal(ctx_d2, ctx) and torch.equal(lse_d2, lse), "second launch on the work queues"
    bad = (ctx_s != ctx).view(B, L, H, hd).any(-1).any(1) | (lse_s != lse).any(-1)
    assert not bad.any(), f"{int(bad.sum())} slabs depend on their place in a walk, first (b, h) = {tuple(int(i) for i in bad.nonzero()[0])}"
    free()


@pytest.mark.parametrize("hd", [32, 16])
@pytest.mark.parametrize("B,H", [(257, 1), (263, 1), (512, 1), (171, 3), (13, 20), (26, 20)])
def test_fwd_slab_counts_at_the_edges_of_the_decomposition(B, H, hd):
    """A.2 + A.6: B * H = 257 (33 slabs per XCD, the last XCD holds 26: one work-group of each of the others walks two slabs), 263, 512, 513 = 171 x 3 (B * H
    not a multiple of 8; one work-group per XCD with three slabs); H = 1 puts consecutive batch elements into one walk.  None of these products has a
    factor 20, so H = 20 runs at its nearest neighbours 260 = 13 x 20 and 520 = 26 x 20.  L 512, 479, 257, 64, 33 (at short L waves without queries still
    move their share of the next slab).  Static lists against fp64; work queues bit for bit the same."""
    for L in (512, 479, 257, 64, 33):
        bias = padded_case(B, H, L)
        q, k, v = fwd_inputs(B, H, L, hd, 7 * B + H + L + hd)
        with tiles_mode() as tm:
            tm.set(False)
            ctx, lse = run_fwd(q, k, v, bias)
            tm.set(True)
            ctx_d, lse_d = run_fwd(q, k, v, bias)
        assert hip.sched_error() == 0
        check_fwd([("static", ctx, lse)], q, k, v, bias, tag=f"B {B} H {H} L {L} hd {hd}")
        assert torch.equal(ctx_d, ctx) and torch.equal(lse_d, lse), f"L {L}: work queues differ from static lists"
    free()


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("B,H,L,hd", [(171, 3, 479, 32), (64, 20, 300, 64)])
def test_fwd_forced_paths_many_slabs(B, H, L, hd, path):
    """every oneprot_attn_force_fwd_path at a mid-sized case of each row width (513 / 1280 slabs) against fp64"""
    bias = padded_case(B, H, L)
    q, k, v = fwd_inputs(B, H, L, hd, 300 + path + hd)
    hip.query("oneprot_attn_force_fwd_path", path)
    try:
        ctx, lse = run_fwd(q, k, v, bias)
    finally:
        hip.query("oneprot_attn_force_fwd_path", -1)
    check_fwd([(f"path {path}", ctx, lse)], q, k, v, bias, tag=f"B {B} H {H} L {L} hd {hd}")


@pytest.mark.parametrize("B,H,L,nb", [(256, 12, 256, 21), (64, 20, 512, 12), (64, 20, 300, 12)])
def test_fwd_hd64_chunk_stream_across_slabs(B, H, L, nb):
    """A.3: k_attn_fwd3w.  B 256, H 12, L 256 is BERT-base at the bench's batch (one chunk per slab, 12 slabs per work-group); L 512 and 300 are two chunks
    per slab: the chunk stream crosses slab boundaries (5 slabs per work-group).  fp64 per slab, and bit for bit the launch in one-slab-per-work-group slices."""
    hd = 64
    bias = padded_case(B, H, L)
    q, k, v = fwd_inputs(B, H, L, hd, 500 + L)
    ctx, lse = run_fwd(q, k, v, bias)
    check_fwd([("persistent", ctx, lse)], q, k, v, bias, tag=f"hd 64 B {B} H {H} L {L}")
    ctx_s, lse_s = sliced_fwd(q, k, v, bias, nb)
    bad = (ctx_s != ctx).view(B, L, H, hd).any(-1).any(1) | (lse_s != lse).any(-1)
    assert not bad.any(), f"{int(bad.sum())} slabs depend on their place in a walk, first (b, h) = {tuple(int(i) for i in bad.nonzero()[0])}"
    free()


@pytest.mark.parametrize("L,hd", [(400, 64), (512, 64), (512, 32)])
def test_fwd_extreme_scores_in_chosen_slabs_of_a_walk(L, hd):
    """A.4: the construction of test_attention_fwd_nomax_overflow_underflow_net (keys u + noise, query row i = alpha_i u: scores near -400 ... +400 log2
    units) at B * H = 800, with the extreme rows ONLY in slabs that are the second, the third and the last of some work-group's walk; every other slab
    ordinary.  hd 64: the persistent kernel marks exactly those slabs and k_attn_fwd2_redo repeats them; hd 32: the in-kernel exact pass.  Every slab
    finite and within the gates; and every ordinary slab bit for bit what a launch without any extreme row writes (a slab repeated without a mark -- or
    a mark put on a neighbour -- would go through the exact pass, which rounds differently)."""
    B, H = 40, 20
    wk = [w for w in walks(B * H, _n_cu()) if len(w) >= 3]
    assert len(wk) >= 3, "B * H = 800 gives every work-group three or four slabs on 256 CUs"
    chosen = sorted({wk[5][1], wk[5][2], wk[len(wk) // 2][-1], wk[-1][1], wk[-3][-1]})
    g = gen(3000 + L + hd)
    q_plain = randn((B, H, L, hd), g, 0.3, dtype=torch.bfloat16)
    k_plain = bf(torch.randn(hd, generator=g, device=DEV) * 0.7 + 0.05 * torch.randn(B, H, L, hd, generator=g, device=DEV))
    v = randn((B, H, L, hd), g, 1.0, dtype=torch.bfloat16)
    q, k = q_plain.clone(), k_plain.clone()
    is_x = extreme_rows(q, k, chosen, g)
    assert float((q_plain.view(B * H, L, hd)[:8].float() @ k_plain.view(B * H, L, hd)[:8].float().transpose(-1, -2)).abs().max()) < 40
    bias = key_bias(pick_patterns(B, H, _n_cu()), L)
    ctx, lse = run_fwd(q, k, v, bias)
    nonfinite = ~(torch.isfinite(ctx.float()).view(B, L, H, hd).all(-1).all(1) & torch.isfinite(lse).all(-1))
    assert not nonfinite.any(), f"non-finite output in flat slabs {nonfinite.flatten().nonzero().flatten().tolist()[:8]} (extreme rows in {chosen})"
    check_fwd([("extreme slabs", ctx, lse)], q, k, v, bias, extreme=is_x, tag=f"hd {hd} L {L}")
    ctx_p, lse_p = run_fwd(q_plain, k_plain, v, bias)
    same = ~((ctx_p != ctx).view(B, L, H, hd).any(-1).any(1) | (lse_p != lse).any(-1))
    assert bool(same[~is_x].all()), f"{int((~same & ~is_x).sum())} ordinary slabs changed by extreme rows elsewhere, first flat slab {int((~same & ~is_x).flatten().nonzero()[0])} (chosen: {chosen})"
    assert not bool(same[is_x].any())
    free()


@pytest.mark.parametrize("B,H", [(10923, 3), (2048, 16)])
def test_fwd_hd64_at_the_limit_of_the_redo_marks(B, H):
    """A.5: hd 64, L 32.  B * H = REDO_SLABS + 1 = 10923 x 3 falls back to k_attn_fwd2 in launch_fwd_nomax; B * H = REDO_SLABS runs the persistent form
    (128 slabs per work-group, marks up to the last word of a set)"""
    L, hd = 32, 64
    assert B * H in (REDO_SLABS, REDO_SLABS + 1)
    ids = torch.randint(0, len(PATTERNS), (B,), generator=torch.Generator().manual_seed(B)).tolist()
    bias = key_bias(ids, L)
    q, k, v = fwd_inputs(B, H, L, hd, 900 + H)
    wk = walks(B * H, _n_cu())
    chosen = sorted({B * H - 1, wk[3][len(wk[3]) // 2], wk[len(wk) // 2][-1], 6})          # the last slab of the launch: the last word of a set of marks
    is_x = extreme_rows(q, k, chosen, gen(901))
    ctx, lse = run_fwd(q, k, v, bias)
    nonfinite = ~(torch.isfinite(ctx.float()).view(B, L, H, hd).all(-1).all(1) & torch.isfinite(lse).all(-1))
    assert not nonfinite.any(), f"non-finite output in flat slabs {nonfinite.flatten().nonzero().flatten().tolist()[:8]} (extreme rows in {chosen})"
    check_fwd([("", ctx, lse)], q, k, v, bias, extreme=is_x, tag=f"hd 64 L 32 B {B} H {H}")
    free()


# ====================================================================================================== B. backward at the bench's slab count
def bwd_ref(q, k, v, bias, dctx, cos, sin, scale, b0, b1):
    """tests/attn_ref.py bwd_ref for batch elements [b0, b1): d(q proj), d(k proj), d(v) as [b1 - b0, H, L, hd]"""
    L = q.shape[2]
    return AR.bwd_ref(q[b0:b1], k[b0:b1], v[b0:b1], None if bias is None else bias[b0:b1], dctx[b0 * L:b1 * L], scale, cos, sin)


def grad_gates(got, ref, name):
    """got / ref [n, H, rows, hd]: per (n, h) slab rel_err < 2e-2 and |err| <= 5e-2 |ref| + 5e-2 max|ref of the slab| (test_attention_fwd_bwd)"""
    got = got.to(F64)
    rel = (got - ref).flatten(2).norm(dim=-1) / (ref.flatten(2).norm(dim=-1) + 1e-20)
    assert bool(torch.isfinite(rel).all()) and float(rel.max()) < 2e-2, f"{name}: rel err {float(torch.nan_to_num(rel, nan=9.9).max()):.3e} in slab {tuple(int(i) for i in (~(rel < 2e-2)).nonzero()[0])}"
    close(got, ref, 5e-2, 5e-2 * ref.abs().flatten(2).amax(-1)[..., None, None], name)


def run_bwd_case(B, H, L, hd, seed, path=-1):
    bias = padded_case(B, H, L)
    q, k, v = fwd_inputs(B, H, L, hd, seed)
    scale = hd ** -0.5
    ctx = torch.empty(B * L, H * hd, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, H, L, device=DEV)
    hip.call("oneprot_attn_fwd", q, k, v, bias, ctx, lse, B, H, L, hd)
    dctx = randn((B * L, H * hd), gen(seed + 1), 1.0, dtype=torch.bfloat16)
    cos, sin = O.rope_tables(L, hd)
    cosd, sind = cos[:, : hd // 2].contiguous().to(DEV), sin[:, : hd // 2].contiguous().to(DEV)
    w = ws(hip.query("oneprot_attn_bwd_workspace", B, H, L))
    outs = []
    hip.query("oneprot_attn_force_bwd_path", path)
    try:
        for rep in range(2):
            dqkv = torch.full((B * L, 3 * H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
            hip.call("oneprot_attn_bwd", q, k, v, bias, ctx, dctx, lse, cosd, sind, scale, dqkv, w, B, H, L, hd)
            outs.append(dqkv)
    finally:
        hip.query("oneprot_attn_force_bwd_path", -1)
    assert torch.equal(outs[0], outs[1]), "two launches of the backward differ (the dQ sums run in a fixed order)"
    got = outs[0].view(B, L, 3, H, hd)
    assert torch.isfinite(got.float()).all()
    # masked keys (probability exactly 0) receive exactly zero dK / dV, in every slab
    masked = bias <= -1.0e30
    assert float(got[:, :, 1:].float().abs().amax((2, 3, 4))[masked].max()) == 0.0, "dK / dV of a masked key is not exactly zero"
    c64, s64 = torch.cat([cosd, cosd], -1).to(F64), torch.cat([sind, sind], -1).to(F64)       # the fp32 tables the kernel reads
    bc = max(1, int(2.5e8 // (H * L * L * 8)))
    for b0 in range(0, B, bc):
        b1 = min(B, b0 + bc)
        refs = bwd_ref(q, k, v, bias, dctx, c64, s64, scale, b0, b1)
        for i, name in enumerate(("dq", "dk", "dv")):
            grad_gates(got[b0:b1, :, i].permute(0, 2, 1, 3), refs[i], f"{name} B {B} H {H} L {L} hd {hd} path {path} from b0 = {b0}")
        del refs
    free()


def test_bwd_bench_launch_hd32():
    """B.1: hd 32, L 512, B 256, H 20, automatic path (the fused kernel with 64 keys per wave): 5120 slabs, each batch element with its own padding"""
    run_bwd_case(256, 20, 512, 32, 1201)


@pytest.mark.parametrize("L,path", [(512, -1), (416, -1), (288, -1), (479, 0), (479, 1), (479, 2)])
def test_bwd_263_slabs_every_path(L, path):
    """B.2: B * H = 263 (not a multiple of 8) at one length per automatic path, and every forced path at L 479"""
    run_bwd_case(263, 1, L, 32, 1300 + L + path, path)


@pytest.mark.parametrize("B,H,L", [(256, 12, 256), (16, 20, 512)])
def test_bwd_hd64_split_kernels_many_slabs(B, H, L):
    """B.3: hd 64 (k_attn_bwd_dq + k_attn_bwd_dkv): BERT-base at the bench's batch, and the 650M head shape at L 512"""
    run_bwd_case(B, H, L, 64, 1400 + L)


# ====================================================================================================== C. NT GEMM epilogues at the bench's launches
def _rows(M, step=8192):
    for r0 in range(0, M, step):
        yield r0, min(M, r0 + step)


def gemm_nt(A, W, epi, bias, o0, o1=None, o2=None, aux=None, cos=None, sin=None, scale=1.0, L=0, H=0, hd=0):
    M, K = A.shape
    N = W.shape[0]
    hip.call("oneprot_gemm_bf16_nt", A, W, M, N, K, K, K, epi, bias, o0, o1, o2, aux, cos, sin, scale, L, H, hd)


def gemm_inputs(M, N, K, seed, wscale=0.1):
    g = gen(seed)
    return randn((M, K), g, 1.0, dtype=torch.bfloat16), randn((N, K), g, wscale, dtype=torch.bfloat16), randn((N,), g, 0.5)


def both_modes(fn):
    """fn() -> tuple of output tensors; run on static tile lists, then on the work queues: equal bits; returns the static outputs"""
    with tiles_mode() as tm:
        tm.set(False)
        ref = fn()
        tm.set(True)
        got = fn()
        torch.cuda.synchronize()
    assert hip.sched_error() == 0
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), f"output {i}: work queues differ from static lists"
    del got
    return ref


def gelu64(z):
    cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    return z * cdf, cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def check_bias_gelu(A, W, bias, u, z, u2, A2=None, dz=None, tag=""):
    """the BIAS_GELU gates of test_gemm_nt_epilogues per 8192-row chunk; dz: GELU_BWD of A2 W^T reading the codes z"""
    W64, b64 = W.to(F64), bias.to(F64)
    for r0, r1 in _rows(A.shape[0]):
        zr = A[r0:r1].to(F64) @ W64.t() + b64
        gz, dg = gelu64(zr)
        close(u[r0:r1], gz, 2 ** -7, 2e-2, f"{tag} gelu(z) rows {r0}")
        close(u2[r0:r1], gz, 2 ** -7, 2e-2, f"{tag} gelu(z), no derivative, rows {r0}")
        zdec = (z[r0:r1].to(F64) - 25.0) / 192.0
        # half a code step (1/384) + the slope of gelu' (<= 0.8) times the bf16-operand error of z itself; exact at the saturated ends
        d = (zdec - dg).abs()
        assert float(d.max()) < 1 / 384 + 2e-3, f"{tag} gelu'(z) codes rows {r0}: {float(d.max()):.3e}"
        assert float(d.mean()) < 1.6e-3, f"{tag} gelu'(z) codes rows {r0}: mean {float(d.mean()):.3e}"
        sat = zr.abs() > 6.0
        assert torch.equal(zdec[sat], (zr[sat] > 0).to(F64)), f"{tag} saturated codes rows {r0}"
        if dz is not None:
            close(dz[r0:r1], (A2[r0:r1].to(F64) @ W64.t()) * zdec, 2 ** -6, 3e-2, f"{tag} gelu bwd rows {r0}")


@pytest.mark.parametrize("M", [131072, 131072 + 256])
def test_gemm_ffn1_gelu_and_its_backward_at_bench_rows(M):
    """(N, K) = (2560, 640): BIAS_GELU with and without the derivative codes, then GELU_BWD reading those codes -- 16 tiles per persistent work-group;
    131328 rows = 513 row panels: whole tiles, work-groups with unequal tile counts"""
    N, K = 2560, 640
    A, W, bias = gemm_inputs(M, N, K, 2100)
    A2 = randn((M, K), gen(2101), 1.0, dtype=torch.bfloat16)

    def run():
        u = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        z = torch.zeros(M, N, dtype=torch.uint8, device=DEV)
        gemm_nt(A, W, hip.EPI_BIAS_GELU, bias, u, z)
        u2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        gemm_nt(A, W, hip.EPI_BIAS_GELU, bias, u2)
        dz = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        gemm_nt(A2, W, hip.EPI_GELU_BWD, None, dz, aux=z)
        return u, z, u2, dz
    u, z, u2, dz = both_modes(run)
    check_bias_gelu(A, W, bias, u, z, u2, A2, dz, tag=f"M {M}")
    free()


@pytest.mark.parametrize("M", [131072, 131072 + 256])
def test_gemm_ffn2_resid_and_bf16_at_bench_rows(M):
    """(N, K) = (640, 2560): BIAS_RESID in place (as the encoder runs it) and BF16"""
    N, K = 640, 2560
    A, W, bias = gemm_inputs(M, N, K, 2200, 0.05)
    resid = randn((M, N), gen(2201))

    def run():
        x = resid.clone()
        gemm_nt(A, W, hip.EPI_BIAS_RESID, bias, x, aux=x)
        o = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        gemm_nt(A, W, hip.EPI_BF16, bias, o)
        return x, o
    x, o = both_modes(run)
    W64, b64 = W.to(F64), bias.to(F64)
    for r0, r1 in _rows(M):
        ref = A[r0:r1].to(F64) @ W64.t() + b64
        close(x[r0:r1], ref + resid[r0:r1].to(F64), 1e-4, 1e-3 * math.sqrt(K / 64), f"bias+resid rows {r0}")
        close(o[r0:r1], ref, 2 ** -7, 2e-2, f"EPI_BF16 rows {r0}")
    free()


def test_gemm_640_by_1920_bf16_at_bench_rows():
    M, N, K = 131072, 640, 1920
    A, W, bias = gemm_inputs(M, N, K, 2300, 0.05)

    def run():
        o = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        gemm_nt(A, W, hip.EPI_BF16, None, o)
        return (o,)
    (o,) = both_modes(run)
    W64 = W.to(F64)
    for r0, r1 in _rows(M):
        close(o[r0:r1], A[r0:r1].to(F64) @ W64.t(), 2 ** -7, 2e-2, f"EPI_BF16 rows {r0}")
    free()


def test_gemm_650m_width_ffn():
    """ESM-2-650M width at M = 32768: (5120, 1280) BIAS_GELU and (1280, 5120) BIAS_RESID"""
    M = 32768
    A, W, bias = gemm_inputs(M, 5120, 1280, 2400, 0.07)

    def run1():
        u = torch.full((M, 5120), float("nan"), dtype=torch.bfloat16, device=DEV)
        z = torch.zeros(M, 5120, dtype=torch.uint8, device=DEV)
        gemm_nt(A, W, hip.EPI_BIAS_GELU, bias, u, z)
        u2 = torch.full((M, 5120), float("nan"), dtype=torch.bfloat16, device=DEV)
        gemm_nt(A, W, hip.EPI_BIAS_GELU, bias, u2)
        return u, z, u2
    u, z, u2 = both_modes(run1)
    check_bias_gelu(A, W, bias, u, z, u2, tag="650M FFN-1")
    del u, z, u2
    A, W, bias = gemm_inputs(M, 1280, 5120, 2401, 0.035)
    resid = randn((M, 1280), gen(2402))

    def run2():
        x = resid.clone()
        gemm_nt(A, W, hip.EPI_BIAS_RESID, bias, x, aux=x)
        return (x,)
    (x,) = both_modes(run2)
    W64, b64 = W.to(F64), bias.to(F64)
    for r0, r1 in _rows(M):
        close(x[r0:r1], A[r0:r1].to(F64) @ W64.t() + b64 + resid[r0:r1].to(F64), 1e-4, 1e-3 * math.sqrt(5120 / 64), f"650M bias+resid rows {r0}")
    free()


def test_gemm_qkv_rope_then_attention_at_bench_shape():
    """(N, K) = (1920, 640) QKV_ROPE writing q / k / v [256, 20, 512, 32] with q_scale = hd^-1/2 log2 e against fp64 (the gates of
    test_gemm_qkv_rope_epilogue, 16 batch elements at a time), and those q / k / v straight into oneprot_attn_fwd with the padding patterns: the chain the
    encoder runs, end to end at size"""
    B, H, L, hd = 256, 20, 512, 32
    d = H * hd
    M, N, K = B * L, 3 * d, d
    # Projections of the scale the attention gates were set at (test_attention_fwd_bwd: k, v of unit scale, q x log2 e of scale one -- the absolute part
    # of the ctx gate, 1e-2, is about 2.5 x 2^-9 x max|v| there): k / v rows of W give unit columns, q rows four times that (q_scale is 0.255).
    A, W, bias = gemm_inputs(M, N, K, 2500, 0.04)
    W[:d] = bf(W[:d].float() * 4.0)
    bias[d:] *= 0.5
    cos, sin = O.rope_tables(L, hd)
    cosd, sind = cos[:, : hd // 2].contiguous().to(DEV), sin[:, : hd // 2].contiguous().to(DEV)
    q_scale = hd ** -0.5 * hip.LOG2E

    def run():
        q, k, v = (torch.full((B, H, L, hd), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(3))
        gemm_nt(A, W, hip.EPI_QKV_ROPE, bias, q, k, v, None, cosd, sind, q_scale, L, H, hd)
        return q, k, v
    q, k, v = both_modes(run)
    c64, s64 = torch.cat([cosd, cosd], -1).to(F64), torch.cat([sind, sind], -1).to(F64)
    W64, b64 = W.to(F64), bias.to(F64)
    for r0, r1 in _rows(M):
        b0, b1 = r0 // L, r1 // L
        y = (A[r0:r1].to(F64) @ W64.t() + b64).view(b1 - b0, L, 3, H, hd).permute(2, 0, 3, 1, 4)
        yq = y[0] * q_scale
        close(q[b0:b1], yq * c64 + rot_half(yq) * s64, 2 ** -7, 2e-2, f"q from b0 = {b0}")
        close(k[b0:b1], y[1] * c64 + rot_half(y[1]) * s64, 2 ** -7, 2e-2, f"k from b0 = {b0}")
        close(v[b0:b1], y[2], 2 ** -7, 2e-2, f"v from b0 = {b0}")
    kb = padded_case(B, H, L)
    ctx, lse = run_fwd(q, k, v, kb)
    check_fwd([("after the QKV GEMM", ctx, lse)], q, k, v, kb, tag="chain")
    free()


# ====================================================================================================== D. packed attention per segment
SEG_LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1026]      # tests/test_packed_gpu.py


def packed_lengths(total, seed):
    """every edge length once, the rest drawn from [32, 1026] (skewed to short: >= 200 segments in 64 k rows), shuffled: segment starts are not aligned to anything"""
    g = torch.Generator().manual_seed(seed)
    lengths = list(SEG_LENGTHS)
    while True:
        n = 32 + int(994 * float(torch.rand((), generator=g)) ** 3)
        if sum(lengths) + n > total:
            break
        lengths.append(n)
    return [lengths[i] for i in torch.randperm(len(lengths), generator=g).tolist()]


def _packed_case(H, hd, total, t_pad, seed):
    lengths = packed_lengths(total, seed)
    p = PackedTokens.from_list([torch.full((n,), 5, dtype=torch.int64) for n in lengths], t_pad=t_pad).to(DEV)
    T = p.T_pad
    cu = cu_of(lengths)
    g = gen(seed)
    scale = hd ** -0.5
    cosd, sind = (t.to(DEV) for t in gathered_tables(lengths, T, hd))
    c, s = torch.cat([cosd, cosd], -1), torch.cat([sind, sind], -1)
    q0, k0 = randn((H, T, hd), g), randn((H, T, hd), g)
    q = bf((q0 * c + rot_half(q0) * s) * (scale * hip.LOG2E * 3.0))                  # (x 3: scores of a few units, as a trained tower has)
    k = bf(k0 * c + rot_half(k0) * s)
    v = randn((H, T, hd), g, 1.0, dtype=torch.bfloat16)
    return p, lengths, cu, T, q, k, v, cosd, sind, scale


def varlen_fwd(p, work, q, k, v, T, H, hd):
    ctx = torch.full((T, H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((H, T), float("nan"), device=DEV)
    hip.call("oneprot_attn_varlen_fwd", q, k, v, p.cu_seqlens, work, work.shape[0], ctx, lse, len(p), T, H, hd)
    return ctx, lse


def varlen_bwd(p, work, q, k, v, ctx, dctx, lse, cosd, sind, scale, T, H, hd):
    w = ws(hip.query("oneprot_attn_varlen_bwd_workspace", H, T))
    dqkv = torch.full((T, 3 * H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.call("oneprot_attn_varlen_bwd", q, k, v, p.cu_seqlens, work, work.shape[0], ctx, dctx, lse, cosd, sind, scale, dqkv, w, len(p), T, H, hd)
    return dqkv


def work_orders(p, lengths):
    """the product's work list (longest segment first), reversed, shuffled, and with items the kernels must ignore: a segment >= N, a negative one, a block
    past its segment's end (varlen_item returns early: an argument check, such a work-group only leaves)"""
    w = p.attn_work()
    n = w.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(DEV)
    short = min(range(len(lengths)), key=lambda b: lengths[b])
    junk = torch.tensor([[len(lengths), 0], [-1, 0], [short, 1], [0, 9]], dtype=torch.int32, device=DEV)
    with_junk = torch.cat([w[: n // 2], junk, w[n // 2:]]).contiguous()
    return w, {"reversed": w.flip(0).contiguous(), "shuffled": w[perm].contiguous(), "with out-of-range items": with_junk}


@pytest.mark.parametrize("H,hd,total,t_pad", [(20, 32, 65536, 65536), (20, 64, 24576, 24576), (20, 32, 24000, 24832)])
def test_packed_attention_per_segment(H, hd, total, t_pad):
    """D: the varlen kernels at H = 20 on a 64 k-row stream of >= 200 shuffled segments (hd 64 and a stream with a tail of > 256 rows on smaller ones).
    Forward: 3e-2 abs ctx and 1e-2 lse per segment against fp64, tail rows exactly zero.  Backward: per (segment, head) the gates of the padded backward
    (rel_err < 2e-2; 5e-2 |ref| + 5e-2 max|ref| of that slab) for segments of >= 32 tokens; for the shorter ones |err| < 0.05 max|ref| with the maximum
    over the whole stream, as test_varlen_attention_backward has it -- these are the six edge lengths 1, 2, 15, 16, 17, 31 of 200+ / 80+ / 60+ segments,
    below a tenth; tail rows exactly zero; twice, equal bits.  Every order of the work list, and a list with out-of-range items, gives equal bits."""
    p, lengths, cu, T, q, k, v, cosd, sind, scale = _packed_case(H, hd, total, t_pad, 4000 + hd + total)
    N, n_real = len(lengths), cu[-1]
    n_short = sum(1 for n in lengths if n < 32)
    assert set(SEG_LENGTHS) <= set(lengths) and n_short == 6 and 10 * n_short < N
    if total == 65536:
        assert N >= 200
    if t_pad != total:
        assert T - n_real > 256
    work, others = work_orders(p, lengths)
    ctx, lse = varlen_fwd(p, work, q, k, v, T, H, hd)
    assert bool((ctx[n_real:] == 0).all()) and bool((lse[:, n_real:] == 0).all()), "tail rows of the forward"
    assert torch.isfinite(ctx[:n_real].float()).all() and torch.isfinite(lse[:, :n_real]).all()
    dctx = randn((T, H * hd), gen(77), 1.0, dtype=torch.bfloat16)
    dctx[n_real:] = 0
    dqkv = varlen_bwd(p, work, q, k, v, ctx, dctx, lse, cosd, sind, scale, T, H, hd)
    assert torch.equal(dqkv, varlen_bwd(p, work, q, k, v, ctx, dctx, lse, cosd, sind, scale, T, H, hd)), "two launches of the packed backward differ"
    assert bool((dqkv[n_real:] == 0).all()), "tail rows of the backward"
    for name, w2 in others.items():
        c2, l2 = varlen_fwd(p, w2, q, k, v, T, H, hd)
        assert torch.equal(c2, ctx) and torch.equal(l2, lse), f"forward, work list {name}"
        assert torch.equal(varlen_bwd(p, w2, q, k, v, ctx, dctx, lse, cosd, sind, scale, T, H, hd), dqkv), f"backward, work list {name}"
    # fp64 per segment
    c64, s64 = torch.cat([cosd, cosd], -1).to(F64), torch.cat([sind, sind], -1).to(F64)
    refs = [torch.zeros(H, T, hd, dtype=F64, device=DEV) for _ in range(3)]
    for a, n in zip(cu[:-1], lengths):
        qkv = [x[None, :, a:a + n] for x in (q, k, v)]                     # the segment as a batch of one
        o, lse64 = AR.fwd_ref(*qkv, None)
        got = ctx[a:a + n].to(F64).view(n, H, hd).transpose(0, 1)
        e = float((got - o[0]).abs().max())
        assert e < 3e-2, f"ctx of the segment at {a} ({n} tokens): {e:.3e}"
        e = float((lse[:, a:a + n].to(F64) - lse64[0]).abs().max())
        assert e < 1e-2, f"lse of the segment at {a} ({n} tokens): {e:.3e}"
        for r, gr in zip(refs, AR.bwd_ref(*qkv, None, dctx[a:a + n], scale, c64[a:a + n], s64[a:a + n])):
            r[:, a:a + n] = gr[0]
    dm = H * hd
    for i, name in enumerate(("dq", "dk", "dv")):
        got = dqkv[:, i * dm:(i + 1) * dm].view(T, H, hd).transpose(0, 1)
        stream_max = float(refs[i].abs().max())
        for a, n in zip(cu[:-1], lengths):
            if n >= 32:
                grad_gates(got[None, :, a:a + n], refs[i][None, :, a:a + n], f"{name} of the segment at {a} ({n} tokens)")
            else:
                e = float((got[:, a:a + n].to(F64) - refs[i][:, a:a + n]).abs().max())
                assert e < 0.05 * stream_max, f"{name} of the segment at {a} ({n} tokens): {e:.3e}"
    free()
