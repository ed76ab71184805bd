"""Plain-torch restatement of the ProNet tower (backbone level), written from the published model (Wang et al., "Learning Hierarchical Protein
Representations via Complete 3D Graph Networks", ICLR 2023; the DIG implementation as remembered) and not from the kernels: the oracle of
oneprot_amd/pronet.py.  Everything is differentiable by autograd and runs in the dtype asked for (fp64 for the tests, fp32 on the GPU for
tools/pronet_ab.py).  It materialises what the HIP path never writes: the [E, h] edge weights and messages.

The graph follows torch_cluster's GPU radius(): sources of the same graph within the cutoff, the LOWEST max_num_neighbors indices when more are in
range; the comparison is d^2 <= r^2 in fp32 (numpy, one rounding per operation), which is what makes graph equality with the kernel exact."""
import functools
import math

import numpy as np
import torch

SLOTS = 32
Y00, Y1 = 0.28209479, 0.48860251


def sph_jn(l, x):
    """spherical Bessel j_l, l in 0..2, on a tensor (closed forms)"""
    if l == 0:
        return torch.sin(x) / x
    if l == 1:
        return torch.sin(x) / x ** 2 - torch.cos(x) / x
    return (3.0 / x ** 2 - 1.0) * torch.sin(x) / x - 3.0 * torch.cos(x) / x ** 2


@functools.lru_cache(maxsize=None)
def bessel_zeros(num_radial):
    """fp64 [2, num_radial]: the first positive zeros of j_0 and j_1 (scipy's root finder on scipy's j_l)"""
    from scipy.optimize import brentq
    from scipy.special import spherical_jn
    out = np.zeros((2, num_radial))
    for l in (0, 1):
        found, x, step = [], 0.5, 0.1
        prev = spherical_jn(l, x)
        while len(found) < num_radial:
            cur = spherical_jn(l, x + step)
            if prev * cur < 0:
                found.append(brentq(lambda t: spherical_jn(l, t), x, x + step, xtol=1e-15, rtol=1e-15))
            x, prev = x + step, cur
        out[l] = found
    return out


def bessel_norms(zeros):
    z = torch.as_tensor(zeros, dtype=torch.float64)
    return torch.stack([math.sqrt(2.0) / sph_jn(l + 1, z[l]).abs() for l in (0, 1)]).numpy()


def rbf(d, num_radial, dtype=torch.float64):
    """[..., 2, num_radial]: sqrt(2) / |j_{l+1}(z_ln)| j_l(z_ln d), no envelope"""
    zeros = bessel_zeros(num_radial)
    z, nrm = torch.as_tensor(zeros, dtype=dtype, device=d.device), torch.as_tensor(bessel_norms(zeros), dtype=dtype, device=d.device)
    x = d[..., None, None] * z
    return torch.stack([nrm[0] * sph_jn(0, x[..., 0, :]), nrm[1] * sph_jn(1, x[..., 1, :])], dim=-2)


# ---- graph ---------------------------------------------------------------------------------------------------------------------------------------------
def radius_graph(ca, ptr, cutoff, cap):
    """(nbr int32 [N, 32], deg int32 [N]) from fp32 coordinates [N, 3] and graph offsets [G + 1]"""
    ca = np.asarray(ca, dtype=np.float32)
    N = ca.shape[0]
    nbr, deg = np.full((N, SLOTS), -1, np.int32), np.zeros(N, np.int32)
    r2 = np.float32(cutoff) * np.float32(cutoff)
    for g in range(len(ptr) - 1):
        a, b = int(ptr[g]), int(ptr[g + 1])
        p = ca[a:b]
        df = p[None, :, :] - p[:, None, :]                 # [i, j] = ca_j - ca_i, fp32
        sq = df * df
        d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        ok = d2 <= r2
        np.fill_diagonal(ok, False)
        for i in range(b - a):
            js = np.nonzero(ok[i])[0][:cap] + a
            nbr[a + i, :len(js)] = js
            deg[a + i] = len(js)
    return nbr, deg


def by_source(nbr, deg):
    """(src_off int32 [N + 1], src_list int32 [E]): for every source its edges' slots i * 32 + e, targets ascending"""
    N = nbr.shape[0]
    lists = [[] for _ in range(N)]
    for i in range(N):
        for e in range(int(deg[i])):
            lists[int(nbr[i, e])].append(i * SLOTS + e)
    off = np.zeros(N + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([s for l in lists for s in l], np.int32)


def edge_index(nbr, deg, device="cpu"):
    """(slot, i, j) int64 [E] of the filled slots, by target"""
    nbr_t, deg_t = torch.as_tensor(np.asarray(nbr)).long(), torch.as_tensor(np.asarray(deg)).long()
    N = nbr_t.shape[0]
    filled = torch.arange(SLOTS)[None, :] < deg_t[:, None]
    slot = torch.nonzero(filled.reshape(-1))[:, 0]
    return slot.to(device), (slot // SLOTS).to(device), nbr_t.reshape(-1)[slot].to(device)


# ---- features --------------------------------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return torch.cross(a, b, dim=-1)


def _dot(a, b):
    return (a * b).sum(-1)


def edge_features(ca, cn, cc, nbr, deg, num_radial=6, num_pos_emb=16, cutoff=10.0, euler_noise=None, dtype=torch.float64):
    """(feature0 [32 N, 4 nr], feature1 [32 N, 6 nr], feature2 [32 N, np]) in `dtype`, unfilled slots 0.  euler_noise: [32 N, 3] already scaled and
    clipped, added to the three Euler angles (the train-mode augmentation; the draws are the caller's)."""
    dev = ca.device
    ca, cn, cc = ca.to(dtype), cn.to(dtype), cc.to(dtype)
    N = ca.shape[0]
    slot, i, j = edge_index(nbr, deg, dev)
    r0, r1 = (i - 1) % N, (i + 1) % N
    v, u0, u1 = ca[j] - ca[i], ca[r0] - ca[i], ca[r1] - ca[i]
    dist = v.norm(dim=-1)
    theta = torch.atan2(_cross(v, u0).norm(dim=-1), _dot(v, u0))
    p1, p2 = _cross(u0, u1), _cross(u0, v)
    phi = torch.atan2(_dot(_cross(p1, p2), u0) / u0.norm(dim=-1), _dot(p1, p2))
    x1, x2 = cn[i] - ca[i], cn[j] - ca[j]
    z1, z2 = _cross(x1, _cross(x1, cc[i] - ca[i])), _cross(x2, _cross(x2, cc[j] - ca[j]))
    l1, l2 = z1.norm(dim=-1) + 1e-7, z2.norm(dim=-1) + 1e-7
    nn_ = _cross(z1, z2)
    a1 = torch.atan2(_dot(_cross(x1, nn_), z1) / l1, _dot(x1, nn_))
    a2 = torch.atan2(nn_.norm(dim=-1), _dot(z1, z2))
    a3 = torch.atan2(_dot(_cross(nn_, x2), z2) / l2, _dot(nn_, x2))
    ang = torch.stack([a1, a2, a3], dim=-1)
    if euler_noise is not None:
        ang = ang + euler_noise.to(dtype).to(dev)[slot]
    rb = rbf(dist / cutoff, num_radial, dtype)                                            # [E, 2, nr]
    Y = torch.stack([torch.full_like(theta, Y00), Y1 * torch.cos(theta), Y1 * torch.sin(theta) * torch.cos(phi), Y1 * torch.sin(theta) * torch.sin(phi)], dim=-1)
    # out[a, b, n] = Y[2 a + b] rbf[b, n]: the published view of the four harmonics as [2, 2] against rbf [2, nr]
    f0 = (Y.reshape(-1, 2, 2, 1) * rb[:, None, :, :]).reshape(len(slot), -1)
    f1 = torch.cat([torch.stack([Y00 * rb[:, 0], Y1 * torch.cos(ang[:, k:k + 1]) * rb[:, 1]], dim=1).reshape(len(slot), -1) for k in range(3)], dim=-1)
    freq = torch.exp(torch.arange(0, num_pos_emb, 2, dtype=dtype, device=dev) * -(math.log(10000.0) / num_pos_emb))
    arg = (j - i).to(dtype)[:, None] * freq
    f2 = torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1)
    out = []
    for f in (f0, f1, f2):
        full = torch.zeros(N * SLOTS, f.shape[1], dtype=dtype, device=dev)
        full[slot] = f
        out.append(full)
    return out


# ---- tower -----------------------------------------------------------------------------------------------------------------------------------------------
def swish(x):
    return x * torch.sigmoid(x)


def edge_conv(feat, W1, W2, a, slot, i, j):
    """m_i = sum_{e into i} (W2 W1 f_e) * a_j, with the edge weights and messages written out"""
    w = (feat[slot] @ W1.t()) @ W2.t()
    return torch.zeros_like(a).index_add(0, i, w * a[j])


def _lin(sd, name, x, bias=True):
    y = x @ sd[name + ".weight"].t()
    return y + sd[name + ".bias"] if bias else y


def block(sd, pre, x, feats, slot, i, j, int_emb_layers=3, x_noise=None, keep=None):
    """one interaction block; x_noise [N, h] is added first, keep = (mask [N, 3 h], scale) is the dropout of the concatenated h_c"""
    if x_noise is not None:
        x = x + x_noise.to(x.dtype)
    a, s = swish(_lin(sd, pre + "lin_1", x)), swish(_lin(sd, pre + "lin_2", x))
    hs = []
    for c in range(3):
        m = edge_conv(feats[c], sd[f"{pre}lin_feature{c}.lin1.weight"], sd[f"{pre}lin_feature{c}.lin2.weight"], a, slot, i, j)
        g = _lin(sd, f"{pre}conv{c}.lin_l", m) + _lin(sd, f"{pre}conv{c}.lin_r", a, bias=False)
        hs.append(swish(_lin(sd, f"{pre}lin{c}", g)))
    t = torch.cat(hs, dim=1)
    if keep is not None:
        t = t * keep[0].to(t.dtype) * keep[1]
    for k in range(int_emb_layers):
        t = swish(_lin(sd, f"{pre}lins_cat.{k}", t))
    t = t + s
    for k in range(int_emb_layers - 1):
        t = swish(_lin(sd, f"{pre}lins.{k}", t))
    return _lin(sd, pre + "final", t)


def forward(sd, batch, num_blocks=4, num_radial=6, num_pos_emb=16, cutoff=10.0, max_num_neighbors=32, int_emb_layers=3, out_layers=2, dtype=torch.float64,
            graph=None, aug=None):
    """[num_graphs, out_channels].  sd: the tower's state dict (published names) in `dtype`; graph = (nbr, deg) if already built.
    aug (train mode): {"euler": [32 N, 3], "x_noise": [per block [N, h]], "keep_H": [per block (mask, scale)], "keep_out": [per readout layer (mask, scale)]}"""
    aug = aug or {}
    dev = batch.coords_ca.device
    ptr = batch.ptr.cpu().numpy()
    nbr, deg = graph if graph is not None else radius_graph(batch.coords_ca.cpu().numpy(), ptr, cutoff, max_num_neighbors)
    feats = edge_features(batch.coords_ca, batch.coords_n, batch.coords_c, nbr, deg, num_radial, num_pos_emb, cutoff, aug.get("euler"), dtype)
    slot, i, j = edge_index(nbr, deg, dev)
    inp = torch.cat([torch.nn.functional.one_hot(batch.x[:, 0].long(), 26).to(dtype), batch.bb_embs.to(dtype)], dim=1)
    x = _lin(sd, "embedding", inp)
    for b in range(num_blocks):
        x = block(sd, f"interaction_blocks.{b}.", x, feats, slot, i, j, int_emb_layers, aug["x_noise"][b] if "x_noise" in aug else None,
                  aug["keep_H"][b] if "keep_H" in aug else None)
    G = int(batch.num_graphs)
    y = torch.zeros(G, x.shape[1], dtype=dtype, device=dev).index_add(0, batch.batch.long(), x)
    for k in range(out_layers - 1):
        y = torch.relu(_lin(sd, f"lins_out.{k}", y))
        if "keep_out" in aug:
            y = y * aug["keep_out"][k][0].to(dtype) * aug["keep_out"][k][1]
    return _lin(sd, "lin_out", y)
