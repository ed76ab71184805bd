"""Host rebuild of the ProNet tower's train-mode draws, from the generators' definitions (tests/philox_ref.py) and the rules stated in
include/oneprot_hip.h: Box-Muller normals on 23-bit uniforms of Philox4x32-10 words, clipped; and the tower's stream numbering."""
import numpy as np
import torch

from tests.philox_ref import M32, philox4x32_10, philox_keep, dropout_threshold

SIGMA, CLIP = 0.025, 0.1


def normals4(n_counters, seed, stream):
    """fp64 [n_counters, 4]: the four standard normals of counter q = 0 .. n - 1: words (0, 1) -> normals 0, 1 (r cos, r sin), words (2, 3) -> 2, 3"""
    q = np.arange(n_counters, dtype=np.uint64)
    w = philox4x32_10(q & np.uint64(M32), q >> np.uint64(32), stream & M32, (stream >> 32) & M32, seed & M32, (seed >> 32) & M32)
    u = [((x >> np.uint32(9)).astype(np.float64) + 0.5) / 8388608.0 for x in w]
    out = np.empty((n_counters, 4))
    for k in (0, 2):
        r, ang = np.sqrt(-2.0 * np.log(u[k])), 2.0 * np.pi * u[k + 1]
        out[:, k], out[:, k + 1] = r * np.cos(ang), r * np.sin(ang)
    return out


def clipped(n):
    return np.clip(SIGMA * n, -CLIP, CLIP)


def euler_noise(n_slots, seed, stream):
    """[n_slots, 3]: what oneprot_pronet_edge_features adds to the three Euler angles of every slot"""
    return torch.from_numpy(clipped(normals4(n_slots, seed, stream)[:, :3]))


def node_noise(shape, seed, stream):
    """[N, h]: what oneprot_clipped_normal_add_f32 adds, element e = normal e & 3 of counter e >> 2"""
    n = int(np.prod(shape))
    return torch.from_numpy(clipped(normals4(n // 4, seed, stream).reshape(-1))).reshape(shape)


def keep_mask(shape, p, seed, stream):
    """(bool mask, scale) of oneprot_dropout_f32 on a tensor of this shape"""
    n = int(np.prod(shape))
    return torch.from_numpy(philox_keep(n, p, seed, stream)).reshape(shape), float(dropout_threshold(p)[1])
