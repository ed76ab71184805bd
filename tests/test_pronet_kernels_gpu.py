"""The kernels of oneprot_amd/csrc/pronet.hip one by one against the fp64 restatement (tests/pronet_ref.py), on the fixtures of
tests/pronet_fixtures.py: the graph exactly, everything else per element.  Tolerances: the project's fp32 rule, rtol 1e-4 and atol 1e-3 sqrt(K / 64)
with K the contraction length (atol 1e-3 for the features, which contract nothing)."""
import math

import numpy as np
import pytest
import torch

from oneprot_amd import hip
from oneprot_amd import pronet as P
from tests import pronet_ref as R
from tests import pronet_rng_ref as RNG
from tests.pronet_fixtures import CUTOFF, conv_case, mixed_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NR, NP = 6, 16


def assert_close(a, ref, rtol, atol, msg=""):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(a).all(), msg
    err = (a - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())
    assert not bad.any(), f"{msg}: {int(bad.sum())} of {bad.numel()} outside, worst |err| {float(err.max()):.3e}"


@pytest.fixture(scope="module")
def graph():
    """(batch on the device, the kernels' Graph, the restatement's nbr / deg)"""
    b = mixed_batch()
    g = P.Graph(b.to(DEV), CUTOFF, 32, P.feature_constants(NR, NP).to(DEV), NR, NP)
    nbr, deg = R.radius_graph(b.coords_ca.numpy(), b.ptr.numpy(), CUTOFF, 32)
    return b, g, nbr, deg


def test_radius_graph_equals_the_restatement(graph):
    b, g, nbr, deg = graph
    got_nbr, got_deg = g.nbr.cpu().numpy(), g.deg.cpu().numpy()
    assert np.array_equal(got_deg, deg) and np.array_equal(got_nbr, nbr)
    ptr, bat = b.ptr.numpy(), b.batch.numpy()
    sizes = np.diff(ptr)
    assert list(sizes) == [2, 1, 33, 34, 100, 5, 300]
    assert deg[ptr[1]] == 0                                                        # the 1-node graph
    assert (deg[ptr[2]:ptr[3]] == 32).all()                                        # 33 nodes in the ball: everybody else
    a34 = ptr[3]
    assert (deg[a34:ptr[4]] == 32).all() and nbr[a34, 31] == a34 + 32 and (nbr[a34:a34 + 2] != a34 + 33).all()        # cap: j = 33 dropped for low i
    assert nbr[a34 + 33, 31] == a34 + 31                                           # ... and the last node keeps 0 .. 31
    walk = deg[ptr[6]:]
    assert walk.min() < 32 and walk.max() <= 32 and walk.min() >= 1
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
        assert_close(g.feat[k], ref[k], 1e-4, 1e-3, f"feature{k}")
    line = slice(int(b.ptr[5]) * 32, int(b.ptr[6]) * 32)                           # exactly collinear CA triples
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
        assert_close(g.feat[k], ref[k], 1e-4, 1e-3, f"feature{k} with noise")
    g2 = P.Graph(b.to(DEV), CUTOFF, 32, P.feature_constants(NR, NP).to(DEV), NR, NP, euler=(seed, stream))
    assert all(torch.equal(u, v) for u, v in zip(g.feat, g2.feat))


@pytest.mark.parametrize("h", [64, 128, 256])
@pytest.mark.parametrize("F", [24, 36, 16])
def test_edge_conv_forward_and_backwards(h, F):
    N, mid = 80, 64
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

    def run():
        m, da, dW = torch.empty(N, h, device=DEV), torch.empty(N, h, device=DEV), torch.empty(F, h, device=DEV)
        hip.call("oneprot_edge_conv_fwd", featd, Wd, ad, nbrd, degd, m, N, h, F)
        hip.call("oneprot_edge_conv_bwd_x", featd, Wd, dmd, offd, lstd, da, N, h, F)
        ws = torch.empty(hip.query("oneprot_edge_conv_bwd_w_workspace", N, h, F), dtype=torch.uint8, device=DEV)
        hip.call("oneprot_edge_conv_bwd_w", featd, ad, dmd, nbrd, degd, dW, ws, ws.numel(), N, h, F)
        return m, da, dW
    m, da, dW = run()
    assert_close(m, m_ref, 1e-4, 1e-3 * math.sqrt(32 * F / 64), "m")
    assert_close(da, a64.grad, 1e-4, 1e-3 * math.sqrt(int(out_deg.max()) * F / 64), "da")
    assert_close(dW, W64.grad, 1e-4, 1e-3 * math.sqrt(E / 64), "dWfT")
    assert (m[torch.as_tensor(deg == 0)] == 0).all() and (da[N - 1] == 0).all()
    again = run()
    assert all(torch.equal(u, v) for u, v in zip((m, da, dW), again))


def test_embedding_pooling_and_row_ops():
    b = mixed_batch()
    N, h, G = b.num_nodes, 128, b.num_graphs
    gen = torch.Generator().manual_seed(3)
    W, bias = torch.randn(h, 32, generator=gen), torch.randn(h, generator=gen)
    z, bb = b.x[:, 0].contiguous(), b.bb_embs
    x0, f32 = torch.empty(N, h, device=DEV), torch.empty(N, 32, device=DEV)
    hip.call("oneprot_pronet_embed_fwd", z.to(DEV), bb.to(DEV), W.to(DEV), bias.to(DEV), x0, f32, N, h)
    inp = torch.cat([torch.nn.functional.one_hot(z, 26).double(), bb.double()], dim=1)
    assert torch.equal(f32.cpu().double(), inp.float().double())
    assert_close(x0, inp @ W.double().t() + bias.double(), 1e-4, 1e-3, "embedding")
    # sum pooling and its backward
    x = torch.randn(N, h, generator=gen)
    y = torch.empty(G, h, device=DEV)
    hip.call("oneprot_segment_sum_f32", x.to(DEV), b.ptr.to(DEV, torch.int32), y, G, h)
    ref = torch.zeros(G, h, dtype=torch.float64).index_add(0, b.batch, x.double())
    assert_close(y, ref, 1e-4, 1e-3 * math.sqrt(300 / 64), "segment sum")
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
        assert_close(wide[:, h:2 * h], out, 1e-4, 1e-3, f"act {act}")
        assert (wide[:, :h] == 0).all() and (wide[:, 2 * h:] == 0).all()
        g = torch.randn(N, 3 * h, generator=gen)
        out.backward(g[:, h:2 * h].double())
        dz, gd = torch.empty(N, h, device=DEV), g.to(DEV)
        hip.call("oneprot_pronet_act_bwd", gd.data_ptr() + 4 * h, zd, dz, N, h, 3 * h, act)
        assert_close(dz, z64.grad, 1e-4, 1e-3, f"act' {act}")


def test_noise_add_and_the_plain_calls():
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(770, 128, generator=gen)
    xd, y = x.to(DEV), torch.empty(770, 128, device=DEV)
    seed, stream = 99, (4 << 60) | 5
    hip.call("oneprot_clipped_normal_add_f32", xd, y, x.numel(), 0.025, 0.1, seed, stream)
    noise = RNG.node_noise(x.shape, seed, stream)
    assert float(noise.abs().max()) <= 0.1 and abs(float(noise.mean())) < 1e-3 and 0.02 < float(noise.std()) < 0.026
    assert_close(y, x.double() + noise, 0.0, 1e-5, "x + noise")                      # the sum's own fp32 rounding is 2.4e-7 at |x| <= 4; the normals agree far below 1e-5
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
