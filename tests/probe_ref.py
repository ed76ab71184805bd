"""Plain-torch restatement of the MLP probe (oneprot_amd/probe.py, ref src/saprot_fit_mlp.py) under autograd, in any dtype: the MLP with the reference's
state-dict names, the three losses, AdamW and the fit loop.  It draws nothing: the dropout masks (rebuilt on the host with tests/philox_ref.py) and the
permutations are handed in.  In fp64 it is the oracle of tests/test_probe_gpu.py; in fp32 it is the yardstick (what plain torch loses on the same input).
tests/test_probe_cpu.py ties it to the reference's own class through tests/golden/probe_mlp.pt."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import philox_ref

EPS = 1e-5
ACTS = {"relu": F.relu, "gelu": F.gelu, "leaky_relu": lambda x: F.leaky_relu(x, 0.01), "identity": lambda x: x}


def spec(hidden_dims, norm="none", activation="relu", use_residual=False, dropout_rate=0.0):
    """norm: "none" | "batch" | "layer" """
    return dict(hidden_dims=list(hidden_dims), norm=norm, activation=activation, use_residual=use_residual, dropout_rate=float(dropout_rate))


def keep_mask(M, n, p, seed, stream):
    """bool [M, n]: the library's dropout mask over the flat [M, n] index, and the fp32 scale of kept values"""
    total = M * n
    keep = philox_ref.philox_keep((total + 7) // 8 * 8, p, seed, stream)[:total].reshape(M, n)
    return torch.from_numpy(keep.copy()), float(philox_ref.dropout_threshold(p)[1])


def dropout(y, mask_scale):
    if mask_scale is None:
        return y
    mask, scale = mask_scale
    return torch.where(mask.to(y.device), y * torch.tensor(scale, dtype=y.dtype), torch.zeros((), dtype=y.dtype))


def layer_names(sp):
    """[(linear index, norm index or None)] into hidden_layers, as the reference's ModuleList numbers them"""
    out, i = [], 0
    for _ in sp["hidden_dims"]:
        lin = i
        i += 1
        norm = None
        if sp["norm"] != "none":
            norm = i
            i += 1
        i += 1                                      # the activation
        if sp["dropout_rate"] > 0:
            i += 1
        out.append((lin, norm))
    return out


def hidden_layer(a, W, b, norm, activation, gamma=None, beta=None, running_mean=None, running_var=None, training=True, mask_scale=None, resid=None):
    """One hidden layer on its own, as the kernels are tested: (z, y, stats) with z = a W^T + b, y = dropout(act(norm(z))) (+ resid); norm "none" | "batch" |
    "layer"; stats holds the batch statistics and the updated running ones of a train-mode BatchNorm"""
    z = a @ W.T + b
    stats, M = {}, a.shape[0]
    h = z
    if norm == "batch":
        if training:
            mean = z.mean(0)
            var = ((z - mean) ** 2).mean(0)
            stats = dict(mean=mean.detach(), rstd=(1.0 / torch.sqrt(var + EPS)).detach(), running_mean=(0.9 * running_mean + 0.1 * mean).detach(),
                         running_var=(0.9 * running_var + 0.1 * var * (M / (M - 1))).detach())
        else:
            mean, var = running_mean, running_var
        h = (z - mean) / torch.sqrt(var + EPS) * gamma + beta
    elif norm == "layer":
        mean = z.mean(1, keepdim=True)
        var = ((z - mean) ** 2).mean(1, keepdim=True)
        h = (z - mean) / torch.sqrt(var + EPS) * gamma + beta
    y = dropout(ACTS[activation](h), mask_scale)
    if resid is not None:
        y = y + resid
    return z, y, stats


def forward(sd, x, sp, training, masks=None):
    """(logits, {buffer name: new value}) of state dict `sd` (parameters and buffers, any dtype) on x [M, input_dim]; masks: one (mask, scale) or None per hidden
    layer, used in training only"""
    new_buffers = {}
    h = x
    for li, (lin, norm) in enumerate(layer_names(sp)):
        kw = {}
        if norm is not None:
            kw = dict(gamma=sd[f"hidden_layers.{norm}.weight"], beta=sd[f"hidden_layers.{norm}.bias"])
        if sp["norm"] == "batch":
            kw.update(running_mean=sd[f"hidden_layers.{norm}.running_mean"], running_var=sd[f"hidden_layers.{norm}.running_var"])
        _, h, stats = hidden_layer(h, sd[f"hidden_layers.{lin}.weight"], sd[f"hidden_layers.{lin}.bias"], sp["norm"], sp["activation"], training=training,
                                   mask_scale=masks[li] if masks is not None else None, **kw)
        if stats:
            new_buffers[f"hidden_layers.{norm}.running_mean"] = stats["running_mean"]
            new_buffers[f"hidden_layers.{norm}.running_var"] = stats["running_var"]
            new_buffers[f"hidden_layers.{norm}.num_batches_tracked"] = sd[f"hidden_layers.{norm}.num_batches_tracked"] + 1
    if sp["use_residual"]:
        r = x
        if "residual_projection.weight" in sd:
            r = x @ sd["residual_projection.weight"].T + sd["residual_projection.bias"]
        h = h + r
    return h @ sd["output_layer.weight"].T + sd["output_layer.bias"], new_buffers


def loss(logits, target, kind):
    """kind 0 BCE with logits, 1 MSE, 2 cross entropy -- the calls of the reference's training_step, the single-output tasks squeezed as there"""
    if kind == 2:
        return F.cross_entropy(logits, target)
    t = target.to(logits.dtype).reshape(logits.shape)
    return F.binary_cross_entropy_with_logits(logits, t) if kind == 0 else F.mse_loss(logits, t)


def is_param(name):
    return not name.endswith(("running_mean", "running_var", "num_batches_tracked"))


def loss_and_grads(sd, x, target, sp, kind, training, masks=None, dtype=torch.float64):
    """(logits, loss, {parameter: gradient}, new buffers) in `dtype`"""
    p = {k: (v.detach().to(dtype).clone().requires_grad_() if is_param(k) else (v.detach().clone() if k.endswith("num_batches_tracked") else v.detach().to(dtype)))
         for k, v in sd.items()}
    logits, nb = forward(p, x.to(dtype), sp, training, masks)
    ls = loss(logits, target, kind)
    ls.backward()
    return logits.detach(), ls.detach(), {k: v.grad for k, v in p.items() if is_param(k)}, nb


def adamw_step(p, g, m, v, step, lr, wd=0.01, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.AdamW's update on tensors of one dtype, out of place: (p, m, v)"""
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


def fit(sd, sp, kind, train, valid, perms, mask_fn, *, learning_rate, batch_size, dtype=torch.float64):
    """The fit loop on handed permutations (one per epoch; their count is the number of epochs): AdamW steps over the batches of each (the tail kept), the
    eval-mode mean validation loss after each, the best epoch's weights (first among equals) returned.  mask_fn(call, layer, M, n) -> (mask, scale) or None.
    Returns (validation losses, best epoch, final state dict).  The learning rate is constant: three epochs never reach the plateau rule."""
    xt, yt = train[0].to(dtype), train[1]
    xv, yv = valid[0].to(dtype), valid[1]
    cur = {k: (v.detach().to(dtype).clone() if v.dtype.is_floating_point else v.detach().clone()) for k, v in sd.items()}
    names = [k for k in cur if is_param(k)]
    m = {k: torch.zeros_like(cur[k]) for k in names}
    v = {k: torch.zeros_like(cur[k]) for k in names}
    step, call, vals, best, best_sd = 0, 0, [], None, None
    for perm in perms:
        perm = torch.as_tensor(np.asarray(perm)).long()
        for s in range(0, len(perm), batch_size):
            idx = perm[s:s + batch_size]
            M = len(idx)
            masks = None
            if sp["dropout_rate"] > 0:
                masks = [mask_fn(call, li, M, n) for li, n in enumerate(sp["hidden_dims"])]
                call += 1
            _, _, g, nb = loss_and_grads(cur, xt[idx], yt[idx], sp, kind, True, masks, dtype)
            step += 1
            for k in names:
                cur[k], m[k], v[k] = adamw_step(cur[k], g[k], m[k], v[k], step, learning_rate)
            cur.update(nb)
        with torch.no_grad():
            val = float(loss(forward(cur, xv, sp, False)[0], yv, kind))
        vals.append(val)
        if best is None or val < vals[best]:
            best, best_sd = len(vals) - 1, {k: t.clone() for k, t in cur.items()}
    return vals, best, best_sd
