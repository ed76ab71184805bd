"""The downstream MLP probe on the device (ref src/saprot_fit_mlp.py): fit, predict and score embeddings with no Lightning, Hydra or sklearn.

`MLP` has the reference's constructor, forward and state-dict names (ref :63-115) and runs on the "few rows" kernels of csrc/probe.hip: a Linear with its
BatchNorm, activation, dropout and residual sum is ONE launch, the backward of norm + activation + dropout is one launch, and all parameters are views of one
flat fp32 tensor (`MLP.arena()`), so AdamW is one launch.  `fit` restates the single-process training loop the reference builds out of Lightning (ref :174-219,
:253-277): embeddings and targets resident, one device permutation per epoch, batches as index ranges of it (never materialised), one readback per epoch.

PINNED: the MLP's arithmetic against the reference's own class (tests/golden/probe_mlp.pt) and the plateau schedule against torch's ReduceLROnPlateau.
NOT pinned: the early-stopping and checkpoint rules, restated from Lightning's documentation (Lightning is not installed here), and every random draw --
shuffle order, dropout masks and the initialisation come from this library's own seeds."""
import itertools
import math

import numpy as np
import torch
import torch.nn as nn

from . import downstream, hip
from .optim import FusedAdamW
from .rng import DOMAINS, StreamOwner

RNG_DOMAIN_PROBE = DOMAINS["probe"]
ACTIVATIONS = {"relu": nn.ReLU, "gelu": nn.GELU, "leaky_relu": nn.LeakyReLU}
EVAL_SLAB = 4096               # rows of one eval-mode forward (validation loss, predict)

# ref saprot_fit_mlp.py:135-150
OUTPUT_DIMS = {"MetalIonBinding": 1, "DeepLoc2": 1, "HumanPPI": 1, "ThermoStability": 1, "EC": 585, "GO-BP": 1943, "GO-MF": 489, "GO-CC": 320, "DeepLoc10": 10,
               "TopEnzyme": 826}
BCE_TASKS = downstream.BINARY_TASKS + downstream.MULTILABEL_TASKS               # ref :164
SQUEEZED_TASKS = downstream.BINARY_TASKS + downstream.REGRESSION_TASKS          # ref :177: y_hat.squeeze(1)


def task_dims(task_name, model_type):
    """(input_dim, output_dim, loss kind) of ref saprot_fit_mlp.py:123-169; loss kind is hip.PROBE_LOSS_BCE / _MSE / _CE"""
    if task_name not in OUTPUT_DIMS:
        raise ValueError(f"Unknown task_name: {task_name}")
    if model_type in ("esm2", "saprot", "oneprot_15", "oneprot_16"):
        input_dim = 1280
    elif model_type == "oneprot_9":
        input_dim = 256
    else:
        input_dim = 1024
    if task_name == "HumanPPI":
        input_dim *= 2
    kind = hip.PROBE_LOSS_BCE if task_name in BCE_TASKS else hip.PROBE_LOSS_MSE if task_name in downstream.REGRESSION_TASKS else hip.PROBE_LOSS_CE
    return input_dim, OUTPUT_DIMS[task_name], kind


class _Saved:
    """what the backward of one forward needs"""
    __slots__ = ("x", "idx", "M", "layers", "last")


class _MLPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, record, *params):
        logits, saved = model._run(x, None, model.training, record)
        ctx.model, ctx.saved, ctx.params = model, saved if record else None, params
        return logits

    @staticmethod
    def backward(ctx, dout):
        if ctx.saved is None:
            raise RuntimeError("MLP: backward of a forward that recorded nothing, or a second backward through the same forward")
        model, saved = ctx.model, ctx.saved
        ctx.saved = None
        model._backward(saved, dout.contiguous().to(torch.float32))
        # copies, not views of the gradient arena: the engine may hold a returned gradient uncopied (a second call of the model in the same graph,
        # torch.autograd.grad's results) while the next backward rewrites the arena
        return (None, None, None) + tuple(model._gview[id(p)].clone() if p.requires_grad else None for p in ctx.params)


class MLP(StreamOwner, nn.Module):
    """ref saprot_fit_mlp.py:63-115, same constructor, forward and state-dict names.  An activation outside {relu, gelu, leaky_relu} raises ValueError (the
    reference silently builds no activation).  With both norm flags BatchNorm wins, as in the reference."""

    def __init__(self, input_dim, output_dim, hidden_dims=[256], dropout_rate=0.0, use_batch_norm=False, use_layer_norm=False, activation="relu", use_residual=False):
        super().__init__()
        if activation not in ACTIVATIONS:
            raise ValueError(f"MLP(activation={activation!r}): one of {', '.join(ACTIVATIONS)}")
        hidden_dims = [int(h) for h in hidden_dims]
        if input_dim < 1 or output_dim < 1 or any(h < 1 for h in hidden_dims):
            raise ValueError("MLP: input_dim, output_dim and every hidden width must be at least 1")
        if not 0 <= float(dropout_rate) < 1:
            raise ValueError(f"MLP(dropout_rate={dropout_rate}): a probability in [0, 1)")
        if use_residual and not hidden_dims:
            raise ValueError("MLP(use_residual=True) needs a hidden layer")
        self.use_residual, self.input_dim, self.output_dim = bool(use_residual), int(input_dim), int(output_dim)
        self.hidden_dims, self.dropout_rate, self.activation = hidden_dims, float(dropout_rate), activation
        layers, in_features = [], self.input_dim
        for h in hidden_dims:
            lin, norm = nn.Linear(in_features, h), None
            layers.append(lin)
            if use_batch_norm:
                norm = nn.BatchNorm1d(h)
            elif use_layer_norm:
                norm = nn.LayerNorm(h)
            if norm is not None:
                layers.append(norm)
            layers.append(ACTIVATIONS[activation]())
            if dropout_rate > 0:
                layers.append(nn.Dropout(dropout_rate))
            in_features = h
        self.hidden_layers = nn.ModuleList(layers)
        self.output_layer = nn.Linear(in_features, self.output_dim)
        self.residual_projection = nn.Linear(self.input_dim, hidden_dims[-1]) if self.use_residual and self.input_dim != hidden_dims[-1] else None
        self._init_streams(fixed_seed=True)
        self._flatten()

    # ---- the arena: every parameter a view of one flat tensor, every gradient the kernels write a view of a second one.  The bookkeeping (_plan, _flat, _gflat,
    # _gview) is derived state outside the module's registered tensors: it is rebuilt from them after a move (_apply) and after unpickling, which is also how
    # copy.deepcopy arrives (__getstate__ / __setstate__), and is never copied.
    _DERIVED = ("_plan", "_flat", "_gflat", "_gview")

    @torch.no_grad()
    def _flatten(self):
        plan, mods = [], list(self.hidden_layers)                              # (Linear, its norm or None) per hidden layer, read off the ModuleList
        for i, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                nxt = mods[i + 1] if i + 1 < len(mods) else None
                plan.append((m, nxt if isinstance(nxt, (nn.BatchNorm1d, nn.LayerNorm)) else None))
        self.__dict__["_plan"] = plan
        params = list(self.parameters())
        dev = params[0].device
        flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
        gflat = torch.zeros_like(flat)
        gview, off = {}, 0
        for p in params:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat[off:off + n].view(p.shape)
            gview[id(p)] = gflat[off:off + n].view(p.shape)
            off += n
        flat.grad = gflat
        self.__dict__.update(_flat=flat, _gflat=gflat, _gview=gview)

    def _is_flat(self):
        """every parameter is still the view of the arena that _flatten made it"""
        flat, off = self._flat, 0
        for p in self.parameters():
            if p.device != flat.device or p.dtype != flat.dtype or p.data_ptr() != flat.data_ptr() + 4 * off or id(p) not in self._gview:
                return False
            off += p.numel()
        return off == flat.numel()

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        if not self._is_flat():                                                # a real move gave every parameter storage of its own; .to() of where it is did not
            self._flatten()
        return self

    def __getstate__(self):
        return {k: v for k, v in super().__getstate__().items() if k not in self._DERIVED}

    def __setstate__(self, state):
        super().__setstate__(state)
        self._flatten()

    def arena(self):
        """The flat fp32 tensor all parameters are views of, in parameters() order.  Its .grad is the flat gradient of the LAST backward (the kernels write, they do
        not accumulate; p.grad of the autograd path accumulates as usual).  A move to another device or dtype makes a new arena: take arena() -- and build an
        optimiser on it -- after the model is where it will run (fit() and predict() move the model to the current GPU if it is elsewhere)."""
        return self._flat

    def _bn_modules(self):
        return [norm for _, norm in self._plan if isinstance(norm, nn.BatchNorm1d)]

    def snapshot(self):
        """device copies of everything a checkpoint of the reference carries: the arena and the BatchNorm buffers"""
        return self._flat.clone(), [b.clone() for m in self._bn_modules() for b in (m.running_mean, m.running_var, m.num_batches_tracked)]

    @torch.no_grad()
    def restore(self, snap):
        self._flat.copy_(snap[0])
        for b, s in zip([b for m in self._bn_modules() for b in (m.running_mean, m.running_var, m.num_batches_tracked)], snap[1]):
            b.copy_(s)

    # ---- RNG position of the dropout masks
    def stream_of(self, call, layer):
        """the Philox stream of hidden layer `layer`'s dropout in train-mode forward number `call`"""
        return self._rng_stream(RNG_DOMAIN_PROBE, call * max(len(self._plan), 1) + layer)

    # ---- forward
    def forward(self, x):
        if x.dim() != 2 or x.shape[1] != self.input_dim or x.shape[0] < 1:
            raise ValueError(f"MLP: input of shape {tuple(x.shape)}; [rows >= 1, {self.input_dim}] is expected")
        if x.requires_grad:
            raise NotImplementedError("MLP: the input is data; no gradient with respect to it is built")
        x = x.to(torch.float32).contiguous()
        params = tuple(self.parameters())
        record = torch.is_grad_enabled() and any(p.requires_grad for p in params)       # grad mode is off inside Function.forward: decided here
        return _MLPFn.apply(self, x, record, *params)

    def _run(self, x, idx, training, save):
        """logits [M, output_dim] of rows idx (int32 device tensor, or None for all rows) of x, and what the backward needs when `save`"""
        M = x.shape[0] if idx is None else idx.numel()
        plan, H = self._plan, len(self._plan)
        bns = self._bn_modules()
        if training and bns:
            if M < 2:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size [{M}, {plan[0][0].out_features}]")
            if M > hip.PROBE_MAX_BATCH:
                raise ValueError(f"MLP: a BatchNorm batch of {M} rows; the train-mode kernel holds at most {hip.PROBE_MAX_BATCH}")
        call = self._next_call() if training and self.dropout_rate > 0 and H else None
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        act = hip.PROBE_ACT[self.activation]
        resid, resid_gathered = None, False
        if self.use_residual:
            rp = self.residual_projection
            if rp is not None:
                resid = new(M, rp.out_features)
                hip.probe_linear_fwd(x, rp.weight, rp.bias, M, rp.out_features, self.input_dim, idx=idx, z=resid)
            else:
                resid, resid_gathered = x, idx is not None
        a, a_idx, k, layers = x, idx, self.input_dim, []
        for i, (lin, norm) in enumerate(plan):
            n = lin.out_features
            last = i == H - 1
            rng = (self.dropout_rate, self._drop_seed, self.stream_of(call, i)) if call is not None else None
            r = resid if last else None
            y, z, mean, rstd = new(M, n), None, None, None
            if isinstance(norm, nn.LayerNorm):
                z = new(M, n)
                if save:
                    mean, rstd = new(M), new(M)
                hip.probe_linear_fwd(a, lin.weight, lin.bias, M, n, k, idx=a_idx, z=z)
                hip.probe_rownorm_act_fwd(z, norm.weight, norm.bias, y, M, n, act=act, resid=r, resid_idx=idx if (r is not None and resid_gathered) else None,
                                          mean=mean, rstd=rstd, rng=rng)
            else:
                z = new(M, n) if save else None
                kw = {}
                if norm is not None:
                    if training:
                        mean, rstd = new(n), new(n)
                    kw = dict(norm=hip.PROBE_NORM_BN_TRAIN if training else hip.PROBE_NORM_BN_EVAL, gamma=norm.weight, beta=norm.bias, mean=mean, rstd=rstd,
                              running_mean=norm.running_mean, running_var=norm.running_var)
                hip.probe_linear_fwd(a, lin.weight, lin.bias, M, n, k, idx=a_idx, z=z, y=y, resid=r, resid_idx=idx if (r is not None and resid_gathered) else None, act=act, rng=rng, **kw)
            layers.append((a, a_idx, k, n, z, mean, rstd, rng, training))
            a, a_idx, k = y, None, n
        if training and bns:
            torch._foreach_add_([m.num_batches_tracked for m in bns], 1)
        logits = new(M, self.output_dim)
        hip.probe_linear_fwd(a, self.output_layer.weight, self.output_layer.bias, M, self.output_dim, k, idx=a_idx, z=logits)
        if not save:
            return logits, None
        saved = _Saved()
        saved.x, saved.idx, saved.M, saved.layers, saved.last = x, idx, M, layers, (a, a_idx, k)
        return logits, saved

    def _backward(self, saved, dlogits):
        """every parameter gradient of one forward, written into the gradient arena"""
        M, G, out = saved.M, self._gview, self.output_layer
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dlogits.device)
        act = hip.PROBE_ACT[self.activation]
        a, a_idx, k = saved.last
        hip.call("oneprot_probe_linear_bwd_w", dlogits, a, a_idx, G[id(out.weight)], G[id(out.bias)], M, self.output_dim, k)
        if not self._plan:
            return
        dA = new(M, k)
        hip.call("oneprot_probe_linear_bwd_x", dlogits, out.weight, dA, M, self.output_dim, k)
        rp = self.residual_projection
        if self.use_residual and rp is not None:
            hip.call("oneprot_probe_linear_bwd_w", dA, saved.x, saved.idx, G[id(rp.weight)], G[id(rp.bias)], M, rp.out_features, self.input_dim)
        for i in reversed(range(len(self._plan))):
            lin, norm = self._plan[i]
            a, a_idx, k, n, z, mean, rstd, rng, training = saved.layers[i]
            dz = new(M, n)
            if isinstance(norm, nn.LayerNorm):
                hip.probe_rownorm_act_bwd(dA, z, norm.weight, norm.bias, mean, rstd, dz, M, n, act=act, dgamma=G[id(norm.weight)], dbeta=G[id(norm.bias)], rng=rng)
            elif norm is not None:
                stats = dict(norm=hip.PROBE_NORM_BN_TRAIN, mean=mean, rstd=rstd) if training else dict(norm=hip.PROBE_NORM_BN_EVAL, mean=norm.running_mean, rstd=norm.running_var)
                hip.probe_norm_act_bwd(dA, z, dz, M, n, act=act, gamma=norm.weight, beta=norm.bias, dgamma=G[id(norm.weight)], dbeta=G[id(norm.bias)], rng=rng, **stats)
            else:
                hip.probe_norm_act_bwd(dA, z, dz, M, n, act=act, rng=rng)
            hip.call("oneprot_probe_linear_bwd_w", dz, a, a_idx, G[id(lin.weight)], G[id(lin.bias)], M, n, k)
            if i > 0:                                                          # layer 0's input is data
                dA = new(M, k)
                hip.call("oneprot_probe_linear_bwd_x", dz, lin.weight, dA, M, n, k)

    # ---- the fused training step of fit(): no autograd, no readback
    def train_step(self, x, target, idx, kind, optimizer, loss_sum, ws, weight=1.0):
        """forward, loss, backward and one optimiser step on rows idx of the resident (x, target); loss_sum (float64 [1]) += weight x the batch's mean loss"""
        logits, saved = self._run(x, idx, True, True)
        dlogits = torch.empty_like(logits)
        tk = dict(labels=target) if kind == hip.PROBE_LOSS_CE else dict(target=target)
        hip.probe_loss(logits, saved.M, self.output_dim, kind, loss_sum, ws, idx=idx, dlogits=dlogits, weight=weight, **tk)
        self._backward(saved, dlogits)
        optimizer.step()

    @torch.no_grad()
    def eval_loss(self, x, target, kind, loss_sum, ws):
        """loss_sum += the eval-mode loss summed over the rows of (x, target) (mean loss of a slab x its rows): no readback"""
        for s in range(0, x.shape[0], EVAL_SLAB):
            xs, ts = x[s:s + EVAL_SLAB], target[s:s + EVAL_SLAB]
            logits, _ = self._run(xs, None, False, False)
            tk = dict(labels=ts) if kind == hip.PROBE_LOSS_CE else dict(target=ts)
            hip.probe_loss(logits, xs.shape[0], self.output_dim, kind, loss_sum, ws, weight=float(xs.shape[0]), **tk)


# ---------------------------------------------------------------------------------------------------------------------------------
# The schedules of the reference's Trainer, on host floats (one per epoch)
class PlateauSchedule:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode="min", factor=0.1, patience=10) with torch's defaults (threshold 1e-4 relative, cooldown 0, min_lr 0,
    eps 1e-8), ref saprot_fit_mlp.py:208-210; step(loss) returns the learning rate of the next epoch"""

    def __init__(self, lr, factor=0.1, patience=10, threshold=1e-4, eps=1e-8):
        self.lr, self.factor, self.patience, self.threshold, self.eps = float(lr), factor, patience, threshold, eps
        self.best, self.num_bad_epochs = math.inf, 0

    def step(self, loss):
        loss = float(loss)
        if loss < self.best * (1.0 - self.threshold):
            self.best, self.num_bad_epochs = loss, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.lr * self.factor, 0.0)
            if self.lr - new_lr > self.eps:
                self.lr = new_lr
            self.num_bad_epochs = 0
        return self.lr


class EarlyStopping:
    """Lightning's EarlyStopping(monitor="val_loss", mode="min", min_delta=0, check_finite=True) as its documentation states it (ref :253-259; unpinned):
    step(loss) is True when training stops -- on a non-finite loss, or once `patience` epochs in a row brought no strict improvement"""

    def __init__(self, patience):
        self.patience, self.best, self.wait = int(patience), math.inf, 0

    def step(self, loss):
        loss = float(loss)
        if not math.isfinite(loss):
            return True
        if loss < self.best:
            self.best, self.wait = loss, 0
            return False
        self.wait += 1
        return self.wait >= self.patience


class BestEpoch:
    """ModelCheckpoint(monitor="val_loss_epoch", mode="min", save_top_k=1) (ref :261-267; unpinned): the first epoch is always kept, a later one replaces it only
    when strictly lower, so the first among equals wins; step(loss) is True when this epoch is the new best"""

    def __init__(self):
        self.epoch, self.loss, self._n = None, None, 0

    def step(self, loss):
        loss, e = float(loss), self._n
        self._n += 1
        if self.epoch is None or loss < self.loss or (math.isnan(self.loss) and not math.isnan(loss)):
            self.epoch, self.loss = e, loss
            return True
        return False


def run_schedule(val_losses, learning_rate, early_stopping_patience):
    """the host side of fit() on a given sequence of validation losses: (learning rate used in every epoch run, best epoch, number of epochs run)"""
    sched, stop, best, lrs = PlateauSchedule(learning_rate), EarlyStopping(early_stopping_patience), BestEpoch(), []
    for v in val_losses:
        lrs.append(sched.lr)
        best.step(v)
        halt = stop.step(v)
        sched.step(v)
        if halt:
            break
    return lrs, best.epoch, len(lrs)


# ---------------------------------------------------------------------------------------------------------------------------------
def _check_partition(name, emb, target, input_dim, output_dim, kind, task_name):
    """shape and dtype rules of one (embeddings, targets) pair; returns them as host-or-device tensors, not yet moved"""
    e = emb if isinstance(emb, torch.Tensor) else torch.as_tensor(np.asarray(emb))
    t = target if isinstance(target, torch.Tensor) else torch.as_tensor(np.asarray(target))
    if e.dim() != 2 or e.shape[0] == 0:
        raise ValueError(f"{name}: embeddings of shape {tuple(e.shape)}; a non-empty [rows, {input_dim}] is expected")
    if e.shape[1] != input_dim:
        raise ValueError(f"{name}: embeddings are {e.shape[1]} wide, the model takes {input_dim}")
    if not e.dtype.is_floating_point:
        raise ValueError(f"{name}: embeddings of dtype {e.dtype}; floating point is expected")
    if t.shape[0] != e.shape[0]:
        raise ValueError(f"{name}: {e.shape[0]} embeddings and {t.shape[0]} targets")
    if kind == hip.PROBE_LOSS_CE:
        if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"{name}: {task_name} takes integer class labels [rows]; got {t.dtype} {tuple(t.shape)}")
    elif task_name in SQUEEZED_TASKS:
        if t.dim() != 1 and tuple(t.shape[1:]) != (1,):
            raise ValueError(f"{name}: {task_name} takes one target per row; got shape {tuple(t.shape)}")
    elif t.dim() != 2 or t.shape[1] != output_dim:
        raise ValueError(f"{name}: {task_name} takes targets [rows, {output_dim}]; got shape {tuple(t.shape)}")
    return e, t


def _resident(e, t, kind, dev):
    e = e.detach().to(dev, torch.float32).contiguous()
    t = t.detach().to(dev, torch.int64 if kind == hip.PROBE_LOSS_CE else torch.float32).contiguous()
    return e, t


def _task_of_model(model, task_name):
    if task_name not in OUTPUT_DIMS:
        raise ValueError(f"Unknown task_name: {task_name}")
    if model.output_dim != OUTPUT_DIMS[task_name]:
        raise ValueError(f"{task_name} has {OUTPUT_DIMS[task_name]} outputs, the model {model.output_dim}")
    return task_dims(task_name, "esm2")[2]


def fit(model, task_name, train, valid, *, learning_rate, batch_size, max_epochs, early_stopping_patience, seed=None):
    """One fit of `model` (ref saprot_fit_mlp.py:174-219, :253-277 on one device): AdamW(lr) steps over shuffled batches of `train` (the tail batch kept), after
    every epoch the eval-mode loss over all of `valid` (the mean over its samples), ReduceLROnPlateau and early stopping on it, and at the end the weights of the
    epoch with the lowest validation loss (the first among equals) restored.  train / valid: (embeddings [N, input_dim], targets); host data is copied to the
    device once.  Returns the per-epoch history: dicts of epoch, lr (used in that epoch), train_loss (the mean over the epoch's samples of the train-mode loss, every batch weighted by its rows as Lightning's
    epoch aggregate is), val_loss, best (bool)."""
    kind = _task_of_model(model, task_name)
    batch_size, max_epochs = int(batch_size), int(max_epochs)
    if batch_size < 1 or max_epochs < 1:
        raise ValueError("fit: batch_size and max_epochs must be at least 1")
    (xt, yt), (xv, yv) = (_check_partition(f"fit: {nm}", *part, model.input_dim, model.output_dim, kind, task_name) for nm, part in (("train", train), ("valid", valid)))
    N = xt.shape[0]
    if model._bn_modules():
        if batch_size > hip.PROBE_MAX_BATCH:
            raise ValueError(f"fit: BatchNorm with batch_size {batch_size}; the train-mode kernel holds at most {hip.PROBE_MAX_BATCH} rows")
        if N % batch_size == 1:
            raise ValueError(f"fit: BatchNorm with {N} training rows and batch_size {batch_size} leaves a tail batch of one row "
                             "(the reference dies mid-epoch: Expected more than 1 value per channel when training)")
    hip.lib()                                                                  # HipLibraryMissing before any device work
    dev = torch.device("cuda", torch.cuda.current_device())
    model.to(dev)
    (xt, yt), (xv, yv) = _resident(xt, yt, kind, dev), _resident(xv, yv, kind, dev)
    gen = None
    if seed is not None:
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        model.set_rng_state({"_drop_seed": int(seed) & 0xFFFFFFFFFFFFFFFF, "_drop_calls": 0, "_rng_uid": 0})      # the masks depend on the seed alone
    opt = FusedAdamW([model.arena()], lr=learning_rate)
    sched, stopper, best = PlateauSchedule(learning_rate), EarlyStopping(early_stopping_patience), BestEpoch()
    sums = torch.zeros(2, dtype=torch.float64, device=dev)                     # train and validation loss sums of the epoch
    ws = hip.probe_loss_workspace(dev)
    history, best_snap = [], None
    for epoch in range(max_epochs):
        model.train()
        opt.param_groups[0]["lr"] = sched.lr
        perm = torch.randperm(N, generator=gen, device=dev).to(torch.int32)
        sums.zero_()
        for s in range(0, N, batch_size):
            model.train_step(xt, yt, perm[s:s + batch_size], kind, opt, sums[0:1], ws, weight=float(min(batch_size, N - s)))
        model.eval()
        model.eval_loss(xv, yv, kind, sums[1:2], ws)
        train_sum, val_sum = sums.cpu().tolist()                               # the epoch's one readback
        val = val_sum / xv.shape[0]
        is_best = best.step(val)
        if is_best:
            best_snap = model.snapshot()
        history.append({"epoch": epoch, "lr": sched.lr, "train_loss": train_sum / N, "val_loss": val, "best": is_best})
        halt = stopper.step(val)
        sched.step(val)
        if halt:
            break
    model.restore(best_snap)
    model.eval()
    return history


@torch.no_grad()
def predict(model, task_name, x):
    """ref predict_step (saprot_fit_mlp.py:221-236) in eval mode, on the device, in slabs: sigmoid [N] (binary), sigmoid [N, C] (multilabel), the output [N]
    (regression) or the argmax class int64 [N] (multiclass)"""
    _task_of_model(model, task_name)
    e = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if e.dim() != 2 or e.shape[0] == 0 or e.shape[1] != model.input_dim:
        raise ValueError(f"predict: embeddings of shape {tuple(e.shape)}; a non-empty [rows, {model.input_dim}] is expected")
    hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    model.to(dev)
    e = e.detach().to(dev, torch.float32).contiguous()
    was_training = model.training
    model.eval()
    outs = []
    for s in range(0, e.shape[0], EVAL_SLAB):
        logits, _ = model._run(e[s:s + EVAL_SLAB], None, False, False)
        if task_name in downstream.BINARY_TASKS:
            outs.append(torch.sigmoid(logits.squeeze(1)))
        elif task_name in downstream.MULTILABEL_TASKS:
            outs.append(torch.sigmoid(logits))
        elif task_name in downstream.REGRESSION_TASKS:
            outs.append(logits.squeeze(1))
        else:
            outs.append(torch.argmax(logits, dim=1))
    model.train(was_training)
    return torch.cat(outs)


def build_model(cfg):
    input_dim, output_dim, _ = task_dims(cfg["task_name"], cfg["model_type"])
    m = cfg["model"]
    return MLP(input_dim, output_dim, hidden_dims=list(m["hidden_dims"]), dropout_rate=m["dropout_rate"], use_batch_norm=m["use_batch_norm"],
               use_layer_norm=m["use_layer_norm"], activation=m["activation"], use_residual=m["use_residual"])


def evaluate(cfg, data):
    """ref evaluate (saprot_fit_mlp.py:240-332): fit, restore the best weights, predict on `valid` and `test`, and return the reference's result dict.  cfg: a
    mapping with the keys of configs/saprot_mlp.yaml (task_name, model_type, model.*; an optional top-level `seed` seeds the initialisation, the shuffles and the
    dropout).  data: {"train_emb", "train_target", "valid_emb", ...} as load_data returns it.  The fitted model and the history are left in evaluate.last."""
    task, m, seed = cfg["task_name"], cfg["model"], cfg["seed"] if "seed" in cfg else None
    if seed is not None:
        torch.manual_seed(int(seed))                                           # nn.Linear's default initialisation, from our own seed
    model = build_model(cfg)
    history = fit(model, task, (data["train_emb"], data["train_target"]), (data["valid_emb"], data["valid_target"]), learning_rate=m["learning_rate"],
                  batch_size=m["batch_size"], max_epochs=m["max_epochs"], early_stopping_patience=m["early_stopping_patience"], seed=seed)
    results = {}
    for partition in ("valid", "test"):
        pred = predict(model, task, data[f"{partition}_emb"])
        results.update(downstream.evaluate_predictions(task, pred, data[f"{partition}_target"], partition))
    evaluate.last = (model, history)
    return results


SWEEP_KEYS = ("learning_rate", "batch_size", "max_epochs", "hidden_dims", "dropout_rate", "use_batch_norm", "use_layer_norm", "activation", "use_residual",
              "task_name", "model_type")


def sweep(cfg, data):
    """the product(...) loop of ref main (saprot_fit_mlp.py:347-401): one row per combination of cfg["sweep"], {the combination's values, the results}.  data: one
    mapping as evaluate takes it, or a callable (cfg) -> mapping that loads a combination's task (load_data)."""
    rows = []
    for combo in itertools.product(*(cfg["sweep"][k] for k in SWEEP_KEYS)):
        c = {k: cfg[k] for k in cfg.keys() if k not in ("sweep", "model")}
        c["model"] = {k: cfg["model"][k] for k in cfg["model"].keys()}
        for k, v in zip(SWEEP_KEYS, combo):
            if k in ("task_name", "model_type"):
                c[k] = v
            else:
                c["model"][k] = v
        results = evaluate(c, data(c) if callable(data) else data)
        rows.append({**dict(zip(SWEEP_KEYS, combo)), **results})
    return rows


load_data = downstream.load_data
