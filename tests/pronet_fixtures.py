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
def small_batch():
    """three small graphs (12 nodes) for the fp64 gradcheck"""
    return GraphBatch.from_data_list([protein("walk", 5, 1), protein("ball", 4, 2), protein("walk", 3, 3)])


def conv_case(N=80, F=24, h=64, seed=0):
    """a hand-made edge table for the convolution kernels: target degrees cycle through {0, 1, 31, 32}; node 0 is a source of every non-empty target
    (out-degree > 32), node N - 1 is a source of none (out-degree 0).  Returns numpy nbr, deg and fp32 torch feat [32 N, F], a [N, h], dm [N, h]."""
    rs = np.random.RandomState(seed)
    nbr, deg = np.full((N, 32), -1, np.int32), np.zeros(N, np.int32)
    for i in range(N):
        d = (0, 1, 31, 32)[i % 4]
        if i == 0:
            d = 32
        pool = [j for j in range(1, N - 1) if j != i]
        js = sorted(([0] if i != 0 and d > 0 else []) + list(rs.choice(pool, d - (1 if i != 0 and d > 0 else 0), replace=False)))
        nbr[i, :d], deg[i] = js, d
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(N * 32, F, generator=g)
    feat[torch.arange(32)[None, :].expand(N, 32).reshape(-1) >= torch.from_numpy(deg).long().repeat_interleave(32)] = 0
    return nbr, deg, feat, torch.randn(N, h, generator=g), torch.randn(N, h, generator=g)
