"""The kernels of oneprot_amd/csrc/pronet.hip one by one against the fp64 restatement (tests/pronet_ref.py), on the fixtures of
tests/pronet_fixtures.py: the graph exactly, everything else per element.  Tolerances: the project's fp32 rule, rtol 1e-4 and atol 1e-3 sqrt(K / 64)
with K the contraction length (atol 1e-3 for the features, which contract nothing).

The graph kernels run on three batches (N = 475 in 7 graphs, 1025 in one, 8193 in 8), the convolutions also at N = 4097 and 8193 and at every feature
width's instantiation, the row ops and the weight gradient at 8193 rows: the sizes at which a grid stops growing, a chunk gets longer than one element or an
accumulator wraps.  Outputs of the large cases start as NaN, and each large case shows on the host that its bound sees one lost row."""
import math

import numpy as np
import pytest
import torch

from oneprot_amd import hip
from oneprot_amd import pronet as P
from tests import pronet_ref as R
from tests import pronet_rng_ref as RNG
from tests.gate import close, rel_l2
from tests.pronet_fixtures import BATCHES, CUTOFF, conv_case, large_batch, mixed_batch, restated_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NR, NP = 6, 16


@pytest.fixture(scope="module", params=["mixed", "one_graph", "large"])
def graph(request):
    """(batch on the device, the kernels' Graph, the restatement's nbr / deg): N = 475 in 7 graphs; N = 1025 in one (the scan's chunks of 2, its
    trailing threads empty); N = 8193 in 8 (chunks of 9)"""
    b = BATCHES[request.param]()
    g = P.Graph(b.to(DEV), CUTOFF, 32, P.feature_constants(NR, NP).to(DEV), NR, NP)
    nbr, deg, _, _ = restated_graph(request.param)
    return b, g, nbr, deg


def test_radius_graph_equals_the_restatement(graph):
    b, g, nbr, deg = graph
    got_nbr, got_deg = g.nbr.cpu().numpy(), g.deg.cpu().numpy()
    assert np.array_equal(got_deg, deg) and np.array_equal(got_nbr, nbr)
    ptr, bat = b.ptr.numpy(), b.batch.numpy()
    sizes = np.diff(ptr)
    if b is mixed_batch():
        assert list(sizes) == [2, 1, 33, 34, 100, 5, 300]
        assert deg[ptr[1]] == 0                                                        # the 1-node graph
        assert (deg[ptr[2]:ptr[3]] == 32).all()                                        # 33 nodes in the ball: everybody else
        a34 = ptr[3]
        assert (deg[a34:ptr[4]] == 32).all() and nbr[a34, 31] == a34 + 32 and (nbr[a34:a34 + 2] != a34 + 33).all()        # cap: j = 33 dropped for low i
        assert nbr[a34 + 33, 31] == a34 + 31                                           # ... and the last node keeps 0 .. 31
        walk = deg[ptr[6]:]
        assert walk.min() < 32 and walk.max() <= 32 and walk.min() >= 1
    else:
        assert len(deg) in (1025, 8193) and 0 < deg.min() < 32 and (deg == 32).sum() > len(deg) // 2      # under the cap on the surface, at it inside
    for i in range(len(deg)):
        js = got_nbr[i, :got_deg[i]]
        assert (bat[js] == bat[i]).all() and (js != i).all() and (np.diff(js) > 0).all()
        assert (got_nbr[i, got_deg[i]:] == -1).all()


def test_by_source_is_the_ordered_permutation(graph):
    _, g, nbr, deg = graph
    off, lst = R.by_source(nbr, deg)
    got_off = g.src_off.cpu().numpy()
    assert np.array_equal(got_off, off)
    got = g.src_list.cpu().numpy()[:off[-1]]
    assert np.array_equal(got, lst)
    filled = np.nonzero((np.arange(32)[None, :] < deg[:, None]).reshape(-1))[0]
    assert np.array_equal(np.sort(got), filled)                                    # a permutation of the by-target slots


def test_edge_features_per_element(graph):
    b, g, nbr, deg = graph
    ref = R.edge_features(b.coords_ca, b.coords_n, b.coords_c, nbr, deg, NR, NP, CUTOFF)
    N = b.num_nodes
    assert deg[0] > 0 and deg[N - 1] > 0                                           # the wrap rows carry edges
    for k in range(3):
        close(g.feat[k], ref[k], 1e-4, 1e-3, f"feature{k}")
    if b is mixed_batch():
        line = slice(int(b.ptr[5]) * 32, int(b.ptr[6]) * 32)                       # exactly collinear CA triples
        assert all(torch.isfinite(f[line]).all() for f in g.feat)


def test_edge_features_with_euler_noise(graph):
    b, _, nbr, deg = graph
    seed, stream = 0x1234ABCD5, (4 << 60) | 77
    g = P.Graph(b.to(DEV), CUTOFF, 32, P.feature_constants(NR, NP).to(DEV), NR, NP, euler=(seed, stream))
    noise = RNG.euler_noise(b.num_nodes * 32, seed, stream)
    assert float(noise.abs().max()) <= 0.1 and float(noise.std()) > 0.02
    ref = R.edge_features(b.coords_ca, b.coords_n, b.coords_c, nbr, deg, NR, NP, CUTOFF, euler_noise=noise)
    plain = R.edge_features(b.coords_ca, b.coords_n, b.coords_c, nbr, deg, NR, NP, CUTOFF)
    assert float((ref[1] - plain[1]).abs().max()) > 1e-2                           # the noise is visible at this tolerance
    for k in range(3):
        close(g.feat[k], ref[k], 1e-4, 1e-3, f"feature{k} with noise")
    g2 = P.Graph(b.to(DEV), CUTOFF, 32, P.feature_constants(NR, NP).to(DEV), NR, NP, euler=(seed, stream))
    assert all(torch.equal(u, v) for u, v in zip(g.feat, g2.feat))


@pytest.mark.parametrize("cap", [1, 16])
@pytest.mark.parametrize("name", ["mixed", "large"])
def test_graph_under_a_smaller_cap(name, cap):
    """max_num_neighbors below the table's width: the lowest `cap` sources survive, every slot behind them up to column 31 is -1"""
    b = BATCHES[name]()
    nbr, deg, off, lst = restated_graph(name, cap)
    N, G = b.num_nodes, b.num_graphs
    ca, ptr, bat = b.coords_ca.to(DEV).contiguous(), b.ptr.to(DEV, torch.int32), b.batch.to(DEV, torch.int32)
    got_nbr, got_deg = torch.full((N, 32), 7, dtype=torch.int32, device=DEV), torch.full((N,), 7, dtype=torch.int32, device=DEV)
    hip.call("oneprot_radius_graph", ca, ptr, bat, got_nbr, got_deg, N, G, CUTOFF, cap)
    assert np.array_equal(got_deg.cpu().numpy(), deg) and np.array_equal(got_nbr.cpu().numpy(), nbr)
    assert int(got_deg.max()) == cap and (cap == 1 or deg.min() < cap) and (deg == cap).sum() > N // 2
    assert bool((got_nbr.cpu()[torch.arange(32)[None, :] >= got_deg.cpu()[:, None].long()] == -1).all()) and bool((got_nbr[:, cap:] == -1).all())
    src_off, src_list = torch.full((N + 1,), -7, dtype=torch.int32, device=DEV), torch.full((N * 32,), -7, dtype=torch.int32, device=DEV)
    hip.call("oneprot_graph_by_source", ptr, bat, got_nbr, got_deg, torch.empty(N, dtype=torch.int32, device=DEV), src_off, src_list, N, G)
    E = int(deg.sum())
    assert np.array_equal(src_off.cpu().numpy(), off) and off[-1] == E
    got = src_list.cpu().numpy()
    assert np.array_equal(got[:E], lst) and (got[E:] == -7).all()                   # nothing written behind the last edge
    assert np.array_equal(np.sort(got[:E]), np.nonzero((np.arange(32)[None, :] < deg[:, None]).reshape(-1))[0])


def _conv_refs(feat, W64, a, dm, nbr, deg, drop=None):
    """fp64 (m, dWfT) by their definitions, with the edges into target `drop` left out: what a kernel that loses that row would have computed"""
    slot, i, j = R.edge_index(nbr, deg)
    if drop is not None:
        keep = i != drop
        slot, i, j = slot[keep], i[keep], j[keep]
    f = feat.double()[slot]
    m = torch.zeros(a.shape, dtype=torch.float64).index_add(0, i, (f @ W64) * a.double()[j])
    return m, f.t() @ (dm.double()[i] * a.double()[j])


@pytest.mark.parametrize("h", [64, 128, 256])
@pytest.mark.parametrize("F", [24, 36, 16])
def test_edge_conv_forward_and_backwards(h, F):
    _edge_conv_check(80, h, F)


@pytest.mark.parametrize("h, F", [(64, 1), (128, 17), (192, 25), (256, 37), (128, 48), (192, 48)])
def test_edge_conv_at_every_width(h, F):
    """F below the instantiation's FMAX (1 in 16, 17 in 24, 25 in 36, 37 in 48: the zero padding of the registers and of the LDS tile), the FMAX = 48
    instantiation at its full width, and h = 192"""
    _edge_conv_check(80, h, F)


@pytest.mark.parametrize("F", [24, 36])
@pytest.mark.parametrize("N", [4097, 8193])
def test_edge_conv_past_the_grids(N, F):
    """N = 4097: the forward / by-source grids stop at 4096 work-groups, so work-group 0 walks rows 0 and 4096 and re-stages its LDS tiles.
    N = 8193: rows 4096 .. 8192 are all second passes; the weight gradient runs 512 work-groups of 17 targets, the last 30 of which own no target and
    write zero slabs, and node 0's 6144 edges are 192 chunks of one by-source row."""
    _edge_conv_check(N, 128, F)


def _edge_conv_check(N, h, F):
    mid = 64
    nbr, deg, feat, a, dm = conv_case(N, F, h, seed=F + h)
    gen = torch.Generator().manual_seed(5)
    W1, W2 = torch.randn(mid, F, generator=gen) / math.sqrt(F), torch.randn(h, mid, generator=gen) / math.sqrt(mid)
    off, lst = R.by_source(nbr, deg)
    out_deg = np.diff(off)
    assert out_deg[N - 1] == 0 and out_deg[0] > 32 and set(deg.tolist()) == {0, 1, 31, 32}
    # fp64 reference under autograd, the folded operand formed as the host does (an fp32 GEMM) so that only the kernels' error is measured
    WfT = (W1.double().t() @ W2.double().t()).float()
    slot, i, j = R.edge_index(nbr, deg)
    a64, W64 = a.double().requires_grad_(), WfT.double().requires_grad_()
    w = feat.double()[slot] @ W64
    m_ref = torch.zeros(N, h, dtype=torch.float64).index_add(0, i, w * a64[j])
    m_ref.backward(dm.double())
    d = lambda t: torch.as_tensor(t).to(DEV)                                   # noqa: E731
    featd, ad, dmd, Wd, nbrd, degd = feat.to(DEV), a.to(DEV), dm.to(DEV), WfT.to(DEV), d(nbr), d(deg)
    offd, lstd = d(off), torch.zeros(N * 32, dtype=torch.int32, device=DEV)
    lstd[:len(lst)] = d(lst)
    E = int(deg.sum())

    nws = hip.query("oneprot_edge_conv_bwd_w_workspace", N, h, F)
    assert nws == min((N + 15) // 16, 512) * F * h * 4 and (N != 8193 or nws == 512 * F * h * 4)

    def run():
        # NaN everywhere first: a row, a slab or an element that no thread writes stays visible
        m, da, dW = (torch.full(s, float("nan"), device=DEV) for s in ((N, h), (N, h), (F, h)))
        hip.call("oneprot_edge_conv_fwd", featd, Wd, ad, nbrd, degd, m, N, h, F)
        hip.call("oneprot_edge_conv_bwd_x", featd, Wd, dmd, offd, lstd, da, N, h, F)
        ws = torch.full((nws // 4,), float("nan"), device=DEV).view(torch.uint8)
        hip.call("oneprot_edge_conv_bwd_w", featd, ad, dmd, nbrd, degd, dW, ws, ws.numel(), N, h, F)
        return m, da, dW
    m, da, dW = run()
    tol_m, tol_da, tol_w = 1e-3 * math.sqrt(32 * F / 64), 1e-3 * math.sqrt(int(out_deg.max()) * F / 64), 1e-3 * math.sqrt(E / 64)
    worst = lambda x, ref: float((x.double().cpu() - ref).abs().max())                   # noqa: E731
    print(f"edge conv N {N} h {h} F {F} E {E}: worst |err| m {worst(m, m_ref.detach()):.2e} (atol {tol_m:.2e})  da {worst(da, a64.grad):.2e} (atol {tol_da:.2e})  "
          f"dWfT {worst(dW, W64.grad):.2e} (atol {tol_w:.2e})")
    close(m, m_ref, 1e-4, tol_m, "m")
    close(da, a64.grad, 1e-4, tol_da, "da")
    close(dW, W64.grad, 1e-4, tol_w, "dWfT")
    assert (m[torch.as_tensor(deg == 0)] == 0).all() and (da[N - 1] == 0).all()
    again = run()
    assert all(torch.equal(u, v) for u, v in zip((m, da, dW), again))
    if N <= 4096:
        return
    # the bounds above can see one lost row: the references with the edges into one target left out are outside them.  The last target with edges, and
    # (N = 8193) target 4097, the second row of work-group 1 in the forward and one of the 17 of work-group 241 in the weight gradient.  At N = 4097 the
    # only second-pass row, 4096, has no edge: what it checks is the exact zero that row (and da[4096]) must receive over the NaN.
    full_m, full_w = _conv_refs(feat, WfT.double(), a, dm, nbr, deg)
    assert float((full_m - m_ref.detach()).abs().max()) < 1e-9 and float((full_w - W64.grad).abs().max()) < 1e-9
    last = int(np.nonzero(deg)[0][-1])
    assert last == N - 2 and deg[N - 1] == 0
    for t in (last, 4097) if N > 4098 else (last,):
        assert deg[t] > 0
        lost_m, lost_w = _conv_refs(feat, WfT.double(), a, dm, nbr, deg, drop=t)
        dm_, dw_ = (full_m - lost_m).abs(), (full_w - lost_w).abs()
        seen_m, seen_w = dm_ > tol_m + 1e-4 * full_m.abs(), dw_ > tol_w + 1e-4 * full_w.abs()
        print(f"  target {t} (deg {deg[t]}) lost: m off by up to {float(dm_.max()):.2e}, {int(seen_m.sum())} elements outside; dWfT off by up to {float(dw_.max()):.2e}, "
              f"{int(seen_w.sum())} of {F * h} outside")
        assert seen_m.any() and seen_w.any()


def test_embedding_pooling_and_row_ops():
    _row_ops_check(mixed_batch())


def test_embedding_pooling_and_row_ops_at_8193_rows():
    """the same on the large batch: 1100-node segments, 33 row blocks in the column sum (its eight accumulators wrap four times, the last block holds
    one row), and 8193 x 128 elements in a 384-wide column block"""
    _row_ops_check(large_batch())


@pytest.mark.parametrize("n", [64, 100, 384])
@pytest.mark.parametrize("M", [2049, 8193])
def test_colsum_at_large_M(M, n):
    """M = 2049 is the first with more than eight row blocks (nine: a[0] takes two) and M = 8193 has 33; both end in a block of one row.  n = 100 leaves
    the second 64-column group partial and the final kernel's only work-group 156 idle threads; n = 384 runs two work-groups there."""
    bat = large_batch().batch[:M]
    gen = torch.Generator().manual_seed(100 * n + M)
    x, dy = torch.randn(M, n, generator=gen), torch.randn(int(bat.max()) + 1, n, generator=gen)
    bound = 4 * 2.0 ** -24
    for rows, label in ((x, "random rows"), (dy[bat], "equal rows")):
        nws = hip.query("oneprot_colsum_f32_workspace", M, n)
        assert nws == (M + 255) // 256 * n * 4
        cs, ws = torch.full((n + 1,), float("nan"), device=DEV), torch.full((nws // 4,), float("nan"), device=DEV).view(torch.uint8)
        hip.call("oneprot_colsum_f32", rows.to(DEV).contiguous(), cs, ws, ws.numel(), M, n)
        assert bool(torch.isnan(cs[n]))                                                 # nothing behind the last column
        got, ref, lost = cs[:n].cpu().double(), rows.double().sum(0), rows[:-1].double().sum(0)
        err, gap, err_lost = float((got - ref).norm() / ref.norm()), float((lost - ref).norm() / ref.norm()), float((got - lost).norm() / lost.norm())
        print(f"colsum M {M} n {n} {label}: rel-L2 {err:.2e} (bound {bound:.2e}); without the last row the reference moves by {gap:.2e}")
        assert err < bound, (label, err)
        assert gap > bound and err_lost > bound, (label, gap, err_lost)                 # the bound sees one lost row


def _row_ops_check(b):
    N, h, G = b.num_nodes, 128, b.num_graphs
    seg = int(np.diff(b.ptr.numpy()).max())
    gen = torch.Generator().manual_seed(3)
    W, bias = torch.randn(h, 32, generator=gen), torch.randn(h, generator=gen)
    z, bb = b.x[:, 0].contiguous(), b.bb_embs
    x0, f32 = torch.empty(N, h, device=DEV), torch.empty(N, 32, device=DEV)
    hip.call("oneprot_pronet_embed_fwd", z.to(DEV), bb.to(DEV), W.to(DEV), bias.to(DEV), x0, f32, N, h)
    inp = torch.cat([torch.nn.functional.one_hot(z, 26).double(), bb.double()], dim=1)
    assert torch.equal(f32.cpu().double(), inp.float().double())
    close(x0, inp @ W.double().t() + bias.double(), 1e-4, 1e-3, "embedding")
    # sum pooling and its backward
    x = torch.randn(N, h, generator=gen)
    y = torch.empty(G, h, device=DEV)
    hip.call("oneprot_segment_sum_f32", x.to(DEV), b.ptr.to(DEV, torch.int32), y, G, h)
    ref = torch.zeros(G, h, dtype=torch.float64).index_add(0, b.batch, x.double())
    assert seg in (300, 1100)
    close(y, ref, 1e-4, 1e-3 * math.sqrt(seg / 64), "segment sum")
    dy, dx = torch.randn(G, h, generator=gen), torch.empty(N, h, device=DEV)
    hip.call("oneprot_segment_sum_bwd_f32", dy.to(DEV), b.batch.to(DEV, torch.int32), dx, N, h)
    assert torch.equal(dx.cpu(), dy[b.batch])
    # column sums (bias gradients): random rows, and the readout's backward, whose rows are equal within a graph
    for rows, label in ((x, "random rows"), (dy[b.batch], "equal rows")):
        ws = torch.empty(hip.query("oneprot_colsum_f32_workspace", N, h), dtype=torch.uint8, device=DEV)
        cs = torch.empty(h, device=DEV)
        hip.call("oneprot_colsum_f32", rows.to(DEV).contiguous(), cs, ws, ws.numel(), N, h)
        ref = rows.double().sum(0)
        err = float((cs.cpu().double() - ref).norm() / ref.norm())
        assert err < 4 * 2.0 ** -24, (label, err)                                   # a blocked sum: a few roundings, not one per row
    # bias + activation (+ residual) into a column block, and the activation's backward
    for act, fn in ((0, lambda t: t), (1, R.swish), (2, torch.relu)):
        zz, res = torch.randn(N, h, generator=gen) * 3, torch.randn(N, h, generator=gen)
        zd, wide = zz.to(DEV), torch.zeros(N, 3 * h, device=DEV)
        hip.call("oneprot_pronet_bias_act", zd, bias.to(DEV), res.to(DEV), wide.data_ptr() + 4 * h, N, h, 3 * h, act)
        z64 = (zz.double() + bias.double()).requires_grad_()
        out = fn(z64) + res.double()
        assert torch.equal(zd.cpu(), (zz + bias))                                   # the pre-activation, in place
        close(wide[:, h:2 * h], out, 1e-4, 1e-3, f"act {act}")
        assert (wide[:, :h] == 0).all() and (wide[:, 2 * h:] == 0).all()
        g = torch.randn(N, 3 * h, generator=gen)
        out.backward(g[:, h:2 * h].double())
        dz, gd = torch.empty(N, h, device=DEV), g.to(DEV)
        hip.call("oneprot_pronet_act_bwd", gd.data_ptr() + 4 * h, zd, dz, N, h, 3 * h, act)
        close(dz, z64.grad, 1e-4, 1e-3, f"act' {act}")


@pytest.mark.parametrize("M, n, k", [(1, 128, 128), (8, 8, 128), (129, 64, 32), (475, 128, 384), (8193, 128, 128), (8193, 128, 32), (8193, 100, 70),
                                     (8193, 128, 384), (33000, 64, 64)])
def test_wgrad_blocked_over_rows(M, n, k):
    """dW = dz^T x, the weight gradient of every node linear (M = the batch's nodes): one slab at M <= 128, a partial last slab, 65 slabs at M = 8193 (the
    reduction's accumulators wrap eight times), 192-row slabs beyond 32 768 rows, tiles cut by n and k.  Per element under the file's rule with K = M, and
    in relative L2 within 4 x the error of the same contraction in fp32 torch, measured here -- the rule of tests/test_pronet_gpu.py, which the plain GEMM's
    single chain of M terms missed by a factor of 6 to 36 at M = 8193.  Random rows, and dz equal within a graph (the readout's backward)."""
    bat = large_batch().batch
    bat = torch.cat([bat + 8 * r for r in range((M + 8192) // 8193)])[:M]
    gen = torch.Generator().manual_seed(M + 7 * n + k)
    x, dz_rand, dy = torch.randn(M, k, generator=gen), torch.randn(M, n, generator=gen), torch.randn(int(bat.max()) + 1, n, generator=gen)
    nws = hip.query("oneprot_wgrad_f32_workspace", M, n, k)
    per = max(128, ((M + 255) // 256 + 63) // 64 * 64)
    assert nws == (M + per - 1) // per * n * k * 4
    for dz, label in ((dz_rand, "random rows"), (dy[bat], "equal rows")):
        def run():
            dW, ws = torch.full((n * k + 1,), float("nan"), device=DEV), torch.full((nws // 4,), float("nan"), device=DEV).view(torch.uint8)
            hip.call("oneprot_wgrad_f32", dz.to(DEV).contiguous(), x.to(DEV), dW, ws, ws.numel(), M, n, k)
            assert bool(torch.isnan(dW[n * k]))                                         # nothing behind the last element
            return dW[:n * k].reshape(n, k)
        dW = run()
        ref, lost = dz.double().t() @ x.double(), dz[:-1].double().t() @ x[:-1].double()
        e32, err, gap = rel_l2(dz.t() @ x, ref), rel_l2(dW, ref), rel_l2(lost, ref)
        print(f"wgrad M {M} n {n} k {k} {label}: rel-L2 hip {err:.2e}  fp32 torch {e32:.2e}  ratio {err / max(e32, 1e-30):.2f}; without the last row the reference moves by {gap:.2e}")
        close(dW, ref, 1e-4, 1e-3 * math.sqrt(M / 64), f"dW {label}")
        assert err <= 4 * max(e32, 2.0 ** -25), (label, err, e32)                       # 2^-25: one rounding, where torch's own sum happens to be exact
        assert M == 1 or (gap > 4 * max(e32, 2.0 ** -25) and rel_l2(dW, lost) > 4 * max(e32, 2.0 ** -25)), (label, gap)      # the bound sees one lost row
        assert torch.equal(dW, run())
    with pytest.raises(hip.HipKernelError):                                             # a short workspace is refused before any launch
        hip.call("oneprot_wgrad_f32", x.to(DEV), x.to(DEV), torch.empty(k, k, device=DEV), torch.empty(16, dtype=torch.uint8, device=DEV), 4, M, k, k)


def test_noise_add_and_the_plain_calls():
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(770, 128, generator=gen)
    xd, y = x.to(DEV), torch.empty(770, 128, device=DEV)
    seed, stream = 99, (4 << 60) | 5
    hip.call("oneprot_clipped_normal_add_f32", xd, y, x.numel(), 0.025, 0.1, seed, stream)
    noise = RNG.node_noise(x.shape, seed, stream)
    assert float(noise.abs().max()) <= 0.1 and abs(float(noise.mean())) < 1e-3 and 0.02 < float(noise.std()) < 0.026
    close(y, x.double() + noise, 0.0, 1e-5, "x + noise")                      # the sum's own fp32 rounding is 2.4e-7 at |x| <= 4; the normals agree far below 1e-5
    y2 = torch.empty_like(y)
    hip.call("oneprot_clipped_normal_add_f32", xd, y2, x.numel(), 0.025, 0.1, seed, stream)
    assert torch.equal(y, y2)
    hip.call("oneprot_clipped_normal_add_f32", xd, y2, x.numel(), 0.0, 0.1, seed, stream)      # sigma 0: the plain copy, bit for bit
    assert torch.equal(y2, xd)
    hip.call("oneprot_dropout_f32", xd, y2, x.numel(), 0.0, seed, stream)                       # p = 0 likewise
    assert torch.equal(y2, xd)
    # refusals: a bad shape returns -1 before any launch
    with pytest.raises(hip.HipKernelError):
        hip.call("oneprot_clipped_normal_add_f32", xd, y2, 6, 0.025, 0.1, seed, stream)
    with pytest.raises(hip.HipKernelError):
        hip.call("oneprot_edge_conv_fwd", xd, xd, xd, torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), y2, 4, 96, 24)
