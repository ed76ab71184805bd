"""Graph fixtures of the ProNet tests, built once per process.  Every fixture used on the GPU keeps | |ca_j - ca_i| - cutoff | >= 1e-4 A for all
same-graph pairs and its coordinates within +-64 A: there the fp32 d^2 comparison is wrong by about 2e-6 A at most, so the kernel's graph can be asked to
equal the restatement's exactly (tests/test_pronet_cpu.py asserts the condition, so that a vacuous fixture fails)."""
import functools

import numpy as np
import torch

from oneprot_amd.graph_data import GraphBatch, GraphData, calc_bb_embs

CUTOFF = 10.0
MARGIN = 1e-4
# graph sizes of the mixed batch, in batch order: the first and the last graph have edges, so that the wrap rows i = 0 and i = N - 1 carry features
MIXED = (("walk", 2), ("walk", 1), ("ball", 33), ("ball", 34), ("walk", 100), ("line", 5), ("walk", 300))
# graph sizes of the large batch, N = 8193: past the scan's 1024 threads (1025 in the one-graph batch), the convolutions' 4096 work-groups and the
# weight gradient's 512 x 16 targets; graph 1 alone is the one-graph batch
LARGE = (1100, 1025, 1100, 1000, 1100, 900, 1100, 868)


def _unit(rs, n):
    v = rs.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _ca(kind, n, rs):
    if kind == "walk":                                   # 3.8 A steps, centred
        ca = np.cumsum(3.8 * _unit(rs, n), axis=0)
        return ca - ca.mean(axis=0)
    if kind == "ball":                                   # uniform in a ball of radius 4.9 A: every pair within the cutoff
        return 4.9 * _unit(rs, n) * rs.uniform(size=(n, 1)) ** (1.0 / 3.0)
    if kind == "line":                                   # exactly collinear CA atoms (fp32-exact coordinates)
        ca = np.zeros((n, 3))
        ca[:, 0] = 3.75 * np.arange(n) - 8.0
        return ca
    if kind == "globule":                                # 3.8 A steps, re-drawn while they leave a ball of radius 3 n^(1/3) A around the first atom
        ca, rad = np.zeros((n, 3)), 3.0 * n ** (1.0 / 3.0)
        for k in range(1, n):
            while True:
                p = ca[k - 1] + 3.8 * _unit(rs, 1)[0]
                if np.linalg.norm(p) <= rad:
                    break
            ca[k] = p
        return ca
    raise ValueError(kind)


def pair_margin(ca):
    """min over the pairs of | |ca_j - ca_i| - cutoff |, fp64, of the fp32 coordinates"""
    p = np.asarray(ca, dtype=np.float32).astype(np.float64)
    d = np.linalg.norm(p[:, None] - p[None], axis=-1)
    iu = np.triu_indices(len(p), 1)
    return np.abs(d[iu] - CUTOFF).min() if len(p) > 1 else np.inf


def protein(kind, n, seed):
    """the first seed >= `seed` whose coordinates satisfy the fixture condition"""
    for s in range(seed, seed + 64):
        rs = np.random.RandomState(s)
        ca = _ca(kind, n, rs).astype(np.float32)
        if pair_margin(ca) >= MARGIN and np.abs(ca).max() <= 60.0:
            break
    else:
        raise AssertionError("no seed satisfies the fixture condition")
    cn = (ca + 1.46 * _unit(rs, n)).astype(np.float32)
    cc = (ca + 1.52 * _unit(rs, n)).astype(np.float32)
    ca, cn, cc = (torch.from_numpy(a) for a in (ca, cn, cc))
    bb = calc_bb_embs(torch.stack((cn, ca, cc), dim=1))
    bb[torch.isnan(bb)] = 0
    return GraphData(x=torch.from_numpy(rs.randint(0, 21, size=(n, 1))), coords_ca=ca, coords_n=cn, coords_c=cc, bb_embs=bb, side_chain_embs=torch.zeros(n, 8))


@functools.lru_cache(maxsize=None)
def mixed_batch():
    return GraphBatch.from_data_list([protein(kind, n, 10 * k) for k, (kind, n) in enumerate(MIXED)])


@functools.lru_cache(maxsize=None)
def large_batch():
    """eight compact chains, 8193 nodes: most targets sit at the cap of 32, the surface ones under it, and the busiest source feeds over 128 targets"""
    return GraphBatch.from_data_list([protein("globule", n, 100 * k) for k, n in enumerate(LARGE)])


@functools.lru_cache(maxsize=None)
def one_graph_batch():
    """the 1025-node globule of the large batch alone"""
    return GraphBatch.from_data_list([protein("globule", LARGE[1], 100)])


BATCHES = {"mixed": mixed_batch, "one_graph": one_graph_batch, "large": large_batch}


@functools.lru_cache(maxsize=None)
def restated_graph(name, cap=32):
    """(nbr, deg, src_off, src_list) of the restatement (tests/pronet_ref.py) for a batch of BATCHES, computed once per process and not to be written to"""
    from tests import pronet_ref as R
    b = BATCHES[name]()
    nbr, deg = R.radius_graph(b.coords_ca.numpy(), b.ptr.numpy(), CUTOFF, cap)
    off, lst = R.by_source(nbr, deg)
    for a in (nbr, deg, off, lst):
        a.setflags(write=False)
    return nbr, deg, off, lst


@functools.lru_cache(maxsize=None)
def small_batch():
    """three small graphs (12 nodes) for the fp64 gradcheck"""
    return GraphBatch.from_data_list([protein("walk", 5, 1), protein("ball", 4, 2), protein("walk", 3, 3)])


def conv_case(N=80, F=24, h=64, seed=0):
    """a hand-made edge table for the convolution kernels: target degrees cycle through {0, 1, 31, 32}; node 0 is a source of every non-empty target
    (out-degree > 32), node N - 1 is a source of none (out-degree 0).  Returns numpy nbr, deg and fp32 torch feat [32 N, F], a [N, h], dm [N, h].
    Up to 256 nodes the other sources are drawn from all of 1 .. N - 2; beyond that from the 128 nearest indices, which keeps the build linear in N."""
    rs = np.random.RandomState(seed)
    nbr, deg = np.full((N, 32), -1, np.int32), np.zeros(N, np.int32)
    for i in range(N):
        d = (0, 1, 31, 32)[i % 4]
        if i == 0:
            d = 32
        if N <= 256:
            pool = [j for j in range(1, N - 1) if j != i]
        else:
            lo = min(max(1, i - 64), N - 1 - 129)
            pool = [j for j in range(lo, lo + 129) if j != i][:128]
        js = sorted(([0] if i != 0 and d > 0 else []) + list(rs.choice(pool, d - (1 if i != 0 and d > 0 else 0), replace=False)))
        nbr[i, :d], deg[i] = js, d
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(N * 32, F, generator=g)
    feat[torch.arange(32)[None, :].expand(N, 32).reshape(-1) >= torch.from_numpy(deg).long().repeat_interleave(32)] = 0
    return nbr, deg, feat, torch.randn(N, h, generator=g), torch.randn(N, h, generator=g)
