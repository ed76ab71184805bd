"""The fp64 restatement of the attention kernels, forward and backward, with an optional probability-dropout keep mask.  q is what the kernels are handed:
rotated, scaled and in log2 units (x log2 e).  keep = None is the all-ones mask: no mask and no scale enter the arithmetic."""
import math

import torch

from oneprot_amd import hip

F64 = torch.float64
LN2 = math.log(2.0)


def rot_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)


def bhld(x, B, H, L, hd):
    """ctx / dctx [B * L, H * hd] as [B, H, L, hd]"""
    return x.view(B, L, H, hd).permute(0, 2, 1, 3)


def _scores(q, k, bias):
    s = (q.to(F64) @ k.to(F64).transpose(-1, -2)) * LN2
    if bias is not None:
        s = s + bias.to(F64)[:, None, None, :]
    return s


def fwd_ref(q, k, v, bias, keep=None, scale=1.0):
    """fp64 (keep * softmax(q k^T ln 2 + bias) * scale) v as [B, H, L, hd], and the undropped lse [B, H, L]; q is in log2 units"""
    s = _scores(q, k, bias)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    if keep is not None:
        p = p * keep * scale
    return p @ v.to(F64), lse


def bwd_ref(q, k, v, bias, dctx, q_scale, cos=None, sin=None, keep=None, scale=1.0):
    """fp64 autograd through (rotary +) scale + softmax (+ mask): the gradients w.r.t. the un-rotated, un-scaled projections, i.e. w.r.t. the stored q
    divided by log2 e and q_scale.  The kernel is handed the rotated, scaled q and the rotated k (bf16); the projections they came from are recovered
    exactly (a rotation is orthogonal), made the leaves, and rotated again inside the graph.  cos / sin fp64 [L, hd] or None; dctx [B * L, H * hd].
    [B, H, L, hd] each."""
    B, H, L, hd = q.shape
    qr, kr = q.to(F64) / hip.LOG2E, k.to(F64)
    if cos is not None:
        qr, kr = qr * cos - rot_half(qr) * sin, kr * cos - rot_half(kr) * sin
    ql, kl, vl = (qr / q_scale).requires_grad_(True), kr.requires_grad_(True), v.to(F64).requires_grad_(True)
    qs, ks = ql * q_scale, kl
    if cos is not None:
        qs, ks = qs * cos + rot_half(qs) * sin, ks * cos + rot_half(ks) * sin
    s = qs @ ks.transpose(-1, -2)
    if bias is not None:
        s = s + bias.to(F64)[:, None, None, :]
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep * scale
    o = p @ vl
    o.backward(bhld(dctx, B, H, L, hd).to(F64))
    return ql.grad, kl.grad, vl.grad


def bwd_ref_reading_ctx(q, k, v, bias, ctx_in, dctx, keep, scale, q_scale, cos=None, sin=None):
    """The same gradients in closed form, with delta = rowsum(dO * ctx_in) from a given ctx [B, H, L, hd] (fp64): dS = P (keep scale dP - delta),
    dq = q_scale R^T (dS k), dk = R^T (dS^T q / log2 e), dv = (keep P scale)^T dO, R^T the inverse rotation.  With the fp64 ctx it IS bwd_ref (asserted
    where it is used); with the bf16 ctx the backward is handed it is the fp64 value of what that call is asked to compute from its inputs."""
    B, H, L, hd = q.shape
    P = torch.softmax(_scores(q, k, bias), -1)
    dO = bhld(dctx, B, H, L, hd).to(F64)
    dS = P * (keep * scale * (dO @ v.to(F64).transpose(-1, -2)) - (dO * ctx_in).sum(-1, keepdim=True))
    dq, dk, dv = dS @ k.to(F64), dS.transpose(-1, -2) @ (q.to(F64) / hip.LOG2E), (P * keep * scale).transpose(-1, -2) @ dO
    if cos is not None:
        dq, dk = dq * cos - rot_half(dq) * sin, dk * cos - rot_half(dk) * sin
    return q_scale * dq, dk, dv
