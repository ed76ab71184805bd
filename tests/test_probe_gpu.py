"""The MLP probe on the device (csrc/probe.hip, oneprot_amd/probe.py) against the fp64 restatement tests/probe_ref.py.

Two kinds of bound, neither measured on the code under test:
  * the plain Linear: |Z - Z64| <= gamma (|A| |W|^T + |b|) elementwise, gamma = (k + 1) u / (1 - (k + 1) u), u = 2^-24, which holds for ANY summation order;
  * everything else: per tensor, the relative L2 error against the fp64 run may be 4 x that of the restatement's fp32 run on the same input (a different
    summation order is worth a small factor and no more, as tests/test_pronet_gpu.py).  Both figures are printed before the assertion (-s).
The yardstick is floored at u / 2 = 2^-25, the rounding of merely storing a result in fp32: on a scalar (a loss) or a tensor of a few elements the fp32 run's
error is ONE draw from a distribution of that scale and can land far below it by luck (measured: 1e-9 on a loss), which no fp32 arithmetic can be held to.
The floor decides nothing wherever the fp32 run's error is an ordinary 3e-8 or more.
A tensor whose exact value is zero has no relative error: the gradient of a bias in front of a train-mode BatchNorm (the norm subtracts the column mean) is
rounding noise in every fp32 run, and so is every gradient through a LayerNorm over ONE feature (its output is beta).  The first is measured against the norm
of the same layer's weight gradient, the second against the norm of the incoming gradient, the yardstick floored at u: 4 x max(e32, u).  Adam
divides that noise by its own magnitude, so such a bias moves by up to lr per step in fp32 and stays put in fp64; after a fit only |p - p64| <= 1.1 steps lr is
asserted for it (nothing else sees it: it cancels in the norm).
The fit test uses 44 training rows: batch 8 needs a row count that is no multiple of 8 for a tail batch (40 has none)."""
import pytest
import torch
import torch.nn.functional as F

from oneprot_amd import downstream, hip, probe
from oneprot_amd.optim import FusedAdamW
from tests import probe_ref as R
from tests.gate import rel_l2
from tests.probe_cases import GOLDEN, make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
FACTOR = 4.0
FLOOR = U / 2             # see the module docstring
M_EDGES = (1, 2, 31, 32, 33, 64, 65, 256, 257, 1000)
N_EDGES = (1, 10, 15, 16, 17, 256, 585)
K_EDGES = (1, 24, 63, 64, 65, 1280)
ACT_NAMES = ("relu", "gelu", "leaky_relu", "identity")
SEED, STREAM = 0x1234ABCD5, (5 << 60) | 77


def check(rows, label):
    """rows: (name, fp32 restatement's error, HIP error) -- print all, then assert the 4 x rule on every one, the yardstick floored at FLOOR"""
    for name, e32, eh in rows:
        print(f"{label} {name:40s} fp32-torch {e32:.3e}  hip {eh:.3e}  ratio {eh / max(e32, 1e-30):.2f}")
    bad = [(n, e32, eh) for n, e32, eh in rows if not eh <= FACTOR * max(e32, FLOOR)]
    assert not bad, f"{label}: outside {FACTOR} x the fp32 restatement's own error: {bad[:6]} ({len(bad)} of {len(rows)})"
    return max((eh for _, _, eh in rows), default=0.0), max((e32 for _, e32, _ in rows), default=0.0)


def zero_valued(got, r32, r64, scale):
    """(e32, ehip) of a tensor whose exact value is 0, against `scale`, the yardstick floored at u"""
    s = float(scale.double().norm())
    return max(float(r32.double().norm()) / s, U), float((got.double().cpu() - r64.double()).norm()) / s


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def new(*shape):
    return torch.empty(shape, dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
def _linear_cases():
    cases = set()
    for i, M in enumerate(M_EDGES):
        cases.add((M, K_EDGES[i % len(K_EDGES)], N_EDGES[i % len(N_EDGES)]))
    for i, k in enumerate(K_EDGES):
        cases.add((M_EDGES[(i + 3) % len(M_EDGES)], k, N_EDGES[(i + 2) % len(N_EDGES)]))
    for i, n in enumerate(N_EDGES):
        cases.add((M_EDGES[(i + 5) % len(M_EDGES)], K_EDGES[(i + 1) % len(K_EDGES)], n))
    cases |= {(1, 1, 1), (1000, 1280, 585), (257, 65, 17), (64, 1280, 256), (65, 63, 15), (256, 64, 16), (33, 1280, 585)}
    return sorted(cases)


def test_linear_fwd_against_the_order_free_bound():
    gen = torch.Generator().manual_seed(1)
    worst = 0.0
    for M, k, n in _linear_cases():
        N = M + 5
        X, W, b = torch.randn(N, k, generator=gen), torch.randn(n, k, generator=gen) / max(k, 1) ** 0.5, torch.randn(n, generator=gen)
        idx = torch.randint(0, N, (M,), generator=gen)
        if M > 2:
            idx[1] = idx[0]                                                        # a repeat for certain; unsorted by construction
        for rows in (None, idx):
            A = X[:M] if rows is None else X[rows]
            z64 = A.double() @ W.double().T + b.double()
            bound = (A.double().abs() @ W.double().abs().T + b.double().abs()) * ((k + 1) * U / (1 - (k + 1) * U))
            z = new(M, n)
            hip.probe_linear_fwd(dev(X), dev(W), dev(b), M, n, k, idx=None if rows is None else dev(rows.to(torch.int32)), z=z)
            err = (z.cpu().double() - z64).abs()
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert bool((err <= bound).all()), (M, k, n, rows is not None, ratio)
    print(f"linear_fwd: worst |Z - Z64| / bound over {len(_linear_cases())} shapes x 2 = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
def _layer_cases(norm):
    ms = [m for m in M_EDGES if norm != "batch_train" or 2 <= m <= 256]
    cases = [(M, 17, 24) for M in ms] + [(33, n, 24) for n in N_EDGES] + [(ms[-1], 585, 63), (ms[0], 1, 24), (2, 16, 1)]
    return list(dict.fromkeys(cases))


def _layer_reference(dtype, t, norm, act, training, mask_scale):
    p = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in t.items() if k in ("a", "W", "b", "gamma", "beta")}
    kw = dict(gamma=p["gamma"], beta=p["beta"]) if norm != "none" else {}
    if norm == "batch":
        kw.update(running_mean=t["rm"].to(dtype), running_var=t["rv"].to(dtype))
    z, y, stats = R.hidden_layer(p["a"], p["W"], p["b"], norm, act, training=training, mask_scale=mask_scale, resid=t["resid"].to(dtype) if t["resid"] is not None else None, **kw)
    z.retain_grad()
    (y * t["cot"].to(dtype)).sum().backward()
    out = dict(z=z.detach(), y=y.detach(), dz=z.grad, dA=p["a"].grad, dW=p["W"].grad, db=p["b"].grad)
    if norm != "none":
        out.update(dgamma=p["gamma"].grad, dbeta=p["beta"].grad)
    out.update(stats)
    return out


def _layer_hip(t, M, n, k, norm, act, training, rng):
    a, W, b, cot, resid = (dev(t[k2]) for k2 in ("a", "W", "b", "cot", "resid"))
    ridx = None
    if t.get("resid_rows") is not None:                                             # the residual as rows resid_rows[m] of a taller matrix: the identity residual of a batch
        rows = t["resid_rows"]                                                      # that is an index range of the resident embeddings
        tall = torch.full((int(rows.max()) + 3, n), float("nan"))
        tall[rows] = t["resid"]
        resid, ridx = dev(tall), dev(rows.to(torch.int32))
    gamma, beta, rm, rv = (dev(t[k2]) for k2 in ("gamma", "beta", "rm", "rv"))
    actid = hip.PROBE_ACT[act]
    out = dict(z=new(M, n), y=new(M, n), dz=new(M, n), dA=new(M, k), dW=new(n, k), db=new(n))
    if norm == "layer":
        mean, rstd = new(M), new(M)
        out.update(dgamma=new(n), dbeta=new(n))
        hip.probe_linear_fwd(a, W, b, M, n, k, z=out["z"])
        hip.probe_rownorm_act_fwd(out["z"], gamma, beta, out["y"], M, n, act=actid, resid=resid, resid_idx=ridx, mean=mean, rstd=rstd, rng=rng)
        hip.probe_rownorm_act_bwd(cot, out["z"], gamma, beta, mean, rstd, out["dz"], M, n, act=actid, dgamma=out["dgamma"], dbeta=out["dbeta"], rng=rng)
    elif norm == "batch":
        out.update(dgamma=new(n), dbeta=new(n))
        if training:
            out.update(mean=new(n), rstd=new(n), running_mean=rm.clone(), running_var=rv.clone())
            hip.probe_linear_fwd(a, W, b, M, n, k, z=out["z"], y=out["y"], resid=resid, resid_idx=ridx, norm=hip.PROBE_NORM_BN_TRAIN, act=actid, gamma=gamma, beta=beta, mean=out["mean"],
                                 rstd=out["rstd"], running_mean=out["running_mean"], running_var=out["running_var"], rng=rng)
            hip.probe_norm_act_bwd(cot, out["z"], out["dz"], M, n, norm=hip.PROBE_NORM_BN_TRAIN, act=actid, gamma=gamma, beta=beta, mean=out["mean"], rstd=out["rstd"],
                                   dgamma=out["dgamma"], dbeta=out["dbeta"], rng=rng)
        else:
            hip.probe_linear_fwd(a, W, b, M, n, k, z=out["z"], y=out["y"], resid=resid, resid_idx=ridx, norm=hip.PROBE_NORM_BN_EVAL, act=actid, gamma=gamma, beta=beta, running_mean=rm,
                                 running_var=rv, rng=rng)
            hip.probe_norm_act_bwd(cot, out["z"], out["dz"], M, n, norm=hip.PROBE_NORM_BN_EVAL, act=actid, gamma=gamma, beta=beta, mean=rm, rstd=rv, dgamma=out["dgamma"],
                                   dbeta=out["dbeta"], rng=rng)
    else:
        hip.probe_linear_fwd(a, W, b, M, n, k, z=out["z"], y=out["y"], resid=resid, resid_idx=ridx, act=actid, rng=rng)
        hip.probe_norm_act_bwd(cot, out["z"], out["dz"], M, n, act=actid, rng=rng)
    hip.call("oneprot_probe_linear_bwd_w", out["dz"], a, None, out["dW"], out["db"], M, n, k)
    hip.call("oneprot_probe_linear_bwd_x", out["dz"], W, out["dA"], M, n, k)
    return out


@pytest.mark.parametrize("norm", ["none", "batch_train", "batch_eval", "layer"])
def test_every_epilogue_and_backward_kernel_per_tensor(norm):
    """forward epilogue (z, y, the statistics, the running buffers) and norm_act_bwd / rownorm_act_bwd / linear_bwd_w / linear_bwd_x (dz, dgamma, dbeta, dW, db, dA)
    at every edge of M and n, the activations in turn, dropout 0.25 and the residual sum on alternate cases, every other residual through a row list (unsorted
    rows of a taller matrix whose other rows hold NaN)"""
    gen, gen_rows = torch.Generator().manual_seed(7), torch.Generator().manual_seed(70)
    kind, training = {"none": ("none", True), "batch_train": ("batch", True), "batch_eval": ("batch", False), "layer": ("layer", True)}[norm]
    worst_h, worst_32 = 0.0, 0.0
    for ci, (M, n, k) in enumerate(_layer_cases(norm)):
        act = ACT_NAMES[ci % 4]
        p = 0.25 if ci % 2 == 0 else 0.0
        t = dict(a=torch.randn(M, k, generator=gen), W=torch.randn(n, k, generator=gen) / k ** 0.5, b=0.1 * torch.randn(n, generator=gen),
                 gamma=1.0 + 0.2 * torch.rand(n, generator=gen), beta=0.1 * torch.randn(n, generator=gen), rm=0.1 * torch.randn(n, generator=gen),
                 rv=1.0 + 0.2 * torch.rand(n, generator=gen), cot=torch.randn(M, n, generator=gen), resid=torch.randn(M, n, generator=gen) if ci % 3 == 0 else None)
        t["resid_rows"] = torch.randperm(M + 4, generator=gen_rows)[:M] if (t["resid"] is not None and ci % 2 == 1) else None
        rng = (p, SEED, STREAM + ci) if p > 0 else None
        mask_scale = R.keep_mask(M, n, p, SEED, STREAM + ci) if p > 0 else None
        r64, r32 = (_layer_reference(dt, t, kind, act, training, mask_scale) for dt in (torch.float64, torch.float32))
        got = _layer_hip(t, M, n, k, kind, act, training, rng)
        assert set(got) == set(r64), (set(got), set(r64))
        rows = []
        for name in r64:
            if name == "db" and norm == "batch_train":                              # (at M = 2 dW is itself a residue, see below: the terms that cancel)
                e32, eh = zero_valued(got[name], r32[name], r64[name], r64["dW"] if M > 2 else t["gamma"].double() * r64["rstd"] * t["cot"].double())
            elif norm == "batch_train" and M == 2 and name in ("dz", "dA", "dW"):
                # two rows normalise to +-1 whatever they hold, so dz is the residue eps / (var + eps) of a cancellation between terms kappa times its size
                # (kappa, printed: 730 at n = 17, 1e5 at n = 1 where dropout took one of the two rows): every fp32 evaluation, torch's included, carries ~kappa u of relative error there (300 draws of the fp32 restatement:
                # median 6e-4, largest 0.3), and one draw against another says nothing.  Both are measured against the terms that cancel.
                kappa = float((t["gamma"].double() * r64["rstd"] * t["cot"].double()).norm() / r64["dz"].norm())
                e32, eh = max(rel_l2(r32[name], r64[name]) / kappa, U), rel_l2(got[name], r64[name]) / kappa
                print(f"{norm} M=2 n={n} k={k} {name}: kappa {kappa:.1f}, unscaled fp32-torch {rel_l2(r32[name], r64[name]):.3e}  hip {rel_l2(got[name], r64[name]):.3e}")
            elif norm == "layer" and n == 1 and name in ("dz", "dA", "dW", "db"):
                assert float(r64[name].norm()) == 0.0
                e32, eh = zero_valued(got[name], r32[name], r64[name], t["cot"])
            else:
                e32, eh = rel_l2(r32[name], r64[name]), rel_l2(got[name], r64[name])
            rows.append((name, e32, eh))
        h, e = check(rows, f"{norm} M={M} n={n} k={k} {act} p={p} resid={'rows' if t['resid_rows'] is not None else t['resid'] is not None}")
        worst_h, worst_32 = max(worst_h, h), max(worst_32, e)
    print(f"{norm}: largest HIP error {worst_h:.3e}, largest fp32-torch error {worst_32:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------------
def _drop_ref(x, p, stream):
    """the existing oneprot_dropout_f32 on a copy padded to a multiple of 8 elements"""
    n = x.numel()
    buf = torch.zeros((n + 7) // 8 * 8, dtype=torch.float32, device=DEV)
    buf[:n] = x.reshape(-1)
    hip.call("oneprot_dropout_f32", buf, buf, buf.numel(), p, SEED, stream)
    return buf[:n].view_as(x)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M, n", [(33, 17), (7, 585), (256, 16), (65, 15)])
def test_fused_dropout_is_the_existing_kernels_mask(M, n, p):
    gen = torch.Generator().manual_seed(M * n)
    k = 24
    a, W, b = dev(torch.randn(M, k, generator=gen)), dev(torch.randn(n, k, generator=gen) / k ** 0.5), dev(torch.randn(n, generator=gen))
    gamma, beta, dy = dev(1.0 + torch.rand(n, generator=gen)), dev(torch.randn(n, generator=gen)), dev(torch.randn(M, n, generator=gen))
    rng = (p, SEED, STREAM)
    for norm in (hip.PROBE_NORM_NONE, hip.PROBE_NORM_BN_TRAIN):
        if norm and M < 2:
            continue
        kw = dict(norm=norm, gamma=gamma, beta=beta, mean=new(n), rstd=new(n)) if norm else {}
        y0, y00, yp, z = new(M, n), new(M, n), new(M, n), new(M, n)
        hip.probe_linear_fwd(a, W, b, M, n, k, z=z, y=y0, act=hip.PROBE_ACT["gelu"], **kw)
        hip.probe_linear_fwd(a, W, b, M, n, k, y=y00, act=hip.PROBE_ACT["gelu"], rng=(0.0, SEED, STREAM), **kw)
        hip.probe_linear_fwd(a, W, b, M, n, k, y=yp, act=hip.PROBE_ACT["gelu"], rng=rng, **kw)
        assert torch.equal(y0, y00)                                                 # p = 0 is the undropped call, bit for bit
        assert torch.equal(yp, _drop_ref(y0, p, STREAM))
        assert 0 < int((yp == 0).sum()) < yp.numel() or n * M < 8
        bk = {k2: v for k2, v in kw.items()}
        dz, dz_ref = new(M, n), new(M, n)                                           # the backward regenerates the same mask: dz(dy, p) == dz(dropout(dy), 0)
        hip.probe_norm_act_bwd(dy, z, dz, M, n, act=hip.PROBE_ACT["gelu"], rng=rng, **bk)
        hip.probe_norm_act_bwd(_drop_ref(dy, p, STREAM), z, dz_ref, M, n, act=hip.PROBE_ACT["gelu"], **bk)
        assert torch.equal(dz, dz_ref)
    mean, rstd, y0, yp = new(M), new(M), new(M, n), new(M, n)                       # the LayerNorm pass
    hip.probe_rownorm_act_fwd(z, gamma, beta, y0, M, n, act=hip.PROBE_ACT["relu"], mean=mean, rstd=rstd)
    hip.probe_rownorm_act_fwd(z, gamma, beta, yp, M, n, act=hip.PROBE_ACT["relu"], rng=rng)
    assert torch.equal(yp, _drop_ref(y0, p, STREAM))
    dz, dz_ref = new(M, n), new(M, n)
    hip.probe_rownorm_act_bwd(dy, z, gamma, beta, mean, rstd, dz, M, n, act=hip.PROBE_ACT["relu"], rng=rng)
    hip.probe_rownorm_act_bwd(_drop_ref(dy, p, STREAM), z, gamma, beta, mean, rstd, dz_ref, M, n, act=hip.PROBE_ACT["relu"])
    assert torch.equal(dz, dz_ref)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_losses_vs_fp64(kind):
    gen = torch.Generator().manual_seed(11 + kind)
    ws = hip.probe_loss_workspace(DEV)
    for C in (1, 5, 489, 1943):
        for M in (1, 33, 256):
            for variant in ("drawn", "extreme", "one_class"):
                x = torch.randn(M, C, generator=gen) * 3
                if variant == "extreme":
                    if kind == 1:
                        continue
                    x.view(-1)[::3] = 80.0
                    x.view(-1)[1::3] = -80.0
                if kind == 2:
                    target = torch.randint(0, C, (M,), generator=gen) if variant != "one_class" else torch.full((M,), C - 1)
                elif kind == 0:
                    target = torch.randint(0, 2, (M, C), generator=gen).float() if variant != "one_class" else torch.zeros(M, C)
                else:
                    target = torch.randn(M, C, generator=gen) if variant != "one_class" else torch.zeros(M, C)
                ref = {}
                for dt in (torch.float64, torch.float32):
                    xx = x.to(dt).requires_grad_()
                    ls = R.loss(xx, target, kind)
                    ls.backward()
                    ref[dt] = (ls.detach(), xx.grad)
                loss_sum, d = torch.zeros(1, dtype=torch.float64, device=DEV), new(M, C)
                tk = dict(labels=dev(target)) if kind == 2 else dict(target=dev(target))
                for _ in range(3):
                    hip.probe_loss(dev(x), M, C, kind, loss_sum, ws, dlogits=d, **tk)
                l64, g64 = ref[torch.float64]
                rows = [("loss (a third of three calls)", rel_l2(ref[torch.float32][0], l64), rel_l2(loss_sum / 3, l64)), ("dlogits", rel_l2(ref[torch.float32][1], g64), rel_l2(d, g64))]
                check(rows, f"loss kind {kind} M={M} C={C} {variant}")
                # the target rows through an index list, and a weight: the same figures
                N = M + 3
                perm = torch.randperm(N, generator=gen)[:M]
                big = torch.zeros((N,) + tuple(target.shape[1:]), dtype=target.dtype)
                big[perm] = target
                tk = dict(labels=dev(big)) if kind == 2 else dict(target=dev(big))
                s2, d2 = torch.zeros(1, dtype=torch.float64, device=DEV), new(M, C)
                hip.probe_loss(dev(x), M, C, kind, s2, ws, idx=dev(perm.to(torch.int32)), dlogits=d2, weight=float(M), **tk)
                assert torch.equal(d2, d) and float(s2) == pytest.approx(float(loss_sum) / 3 * M, rel=1e-12)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", [1, 3, 4, 1025])
def test_adamw_step_vs_fp64(n, wd):
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-3, 1, (1,), generator=gen)) for _ in range(5)]
    ref = {}
    for dt in (torch.float64, torch.float32):
        p, m, v = p0.to(dt), torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt)
        for step, g in enumerate(grads, 1):
            p, m, v = R.adamw_step(p, g.to(dt), m, v, step, 1e-3, wd)
        ref[dt] = (p, m, v)
    w = dev(p0).clone()
    opt = FusedAdamW([w], lr=1e-3, weight_decay=wd)
    for g in grads:
        w.grad = dev(g)
        opt.step()
    st = opt.state[w]
    got = (w, st["exp_avg"], st["exp_avg_sq"])
    check([(nm, rel_l2(ref[torch.float32][i], ref[torch.float64][i]), rel_l2(got[i], ref[torch.float64][i])) for i, nm in enumerate(("p", "exp_avg", "exp_avg_sq"))],
          f"adamw n={n} wd={wd}")


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


def test_mlp_on_the_device_vs_the_reference_class(golden):
    """outputs (train and eval mode), the three losses, every gradient, the BatchNorm buffers: the HIP MLP against the fp64 restatement, the yardstick being the
    error of the values the REFERENCE'S class computed in fp32 (the golden) against the same fp64 run"""
    x, ws = golden["x"], hip.probe_loss_workspace(DEV)
    for cfg in golden["configs"]:
        label = f"{cfg['norm']}/{cfg['activation']}/{cfg['residual']}"
        sp = R.spec(cfg["hidden_dims"], cfg["norm"], cfg["activation"], cfg["use_residual"])
        sd = cfg["state_dict"]
        sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
        zero = {f"hidden_layers.{lin}.bias": f"hidden_layers.{lin}.weight" for lin, _ in R.layer_names(sp)} if cfg["norm"] == "batch" else {}
        with torch.no_grad():
            eval64, _ = R.forward(sd64, x.double(), sp, False)
            train64, nb64 = R.forward(sd64, x.double(), sp, True)
        model = make(cfg, golden)
        model.load_state_dict(sd, strict=True)
        model.to(DEV)
        model.eval()
        with torch.no_grad():
            out_eval = model(x.to(DEV))
        model.train()
        with torch.no_grad():
            out_train = model(x.to(DEV))
        rows = [("out_eval", rel_l2(cfg["out_eval"], eval64), rel_l2(out_eval, eval64)), ("out_train", rel_l2(cfg["out_train"], train64), rel_l2(out_train, train64))]
        after = model.state_dict()
        for k, v in cfg["buffers_after"].items():
            if k.endswith("num_batches_tracked"):
                assert int(after[k]) == int(v) == 1
            else:
                rows.append((k, rel_l2(v, nb64[k]), rel_l2(after[k], nb64[k])))
        for kind in (0, 1, 2):
            target = golden["targets"][kind]
            _, l64, g64, _ = R.loss_and_grads(sd, x, target, sp, kind, True)
            model.load_state_dict(sd, strict=True)
            if kind == 1:                                                           # once through autograd and torch's loss: the Function's backward
                model.zero_grad(set_to_none=True)
                ls = F.mse_loss(model(x.to(DEV)), target.to(DEV))
                ls.backward()
                grads = {k: p.grad for k, p in model.named_parameters()}
            else:                                                                   # the fused path of fit(): loss kernel, gradients in the arena
                logits, saved = model._run(x.to(DEV), None, True, True)
                loss_sum, d = torch.zeros(1, dtype=torch.float64, device=DEV), torch.empty_like(logits)
                tk = dict(labels=dev(target)) if kind == 2 else dict(target=dev(target))
                hip.probe_loss(logits, x.shape[0], golden["output_dim"], kind, loss_sum, ws, dlogits=d, **tk)
                model._backward(saved, d)
                ls, grads = loss_sum[0], {k: model._gview[id(p)].clone() for k, p in model.named_parameters()}
            rows.append((f"loss{kind}", rel_l2(cfg["loss"][kind], l64), rel_l2(ls, l64)))
            for k in g64:
                if k in zero:
                    e32, eh = zero_valued(grads[k], cfg["grads"][kind][k], g64[k], g64[zero[k]])
                else:
                    e32, eh = rel_l2(cfg["grads"][kind][k], g64[k]), rel_l2(grads[k], g64[k])
                rows.append((f"loss{kind} d {k}", e32, eh))
        check(rows, label)


def test_two_forwards_in_one_backward_and_autograd_grad_keep_their_gradients(golden):
    """The autograd path hands out gradients of its own, never views of the arena the next backward rewrites: two calls of the model inside one graph sum
    their gradients, and what torch.autograd.grad returned is not changed by a later backward.  Against the fp64 restatement by the 4 x rule."""
    cfg = next(c for c in golden["configs"] if (c["norm"], c["activation"], c["residual"]) == ("layer", "gelu", "projected"))
    sp = R.spec(cfg["hidden_dims"], cfg["norm"], cfg["activation"], cfg["use_residual"])
    gen = torch.Generator().manual_seed(31)
    x1, x2 = golden["x"], torch.randn(9, golden["input_dim"], generator=gen)
    c1, c2 = torch.randn(7, golden["output_dim"], generator=gen), torch.randn(9, golden["output_dim"], generator=gen)
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = {k: v.detach().to(dt).clone().requires_grad_() for k, v in cfg["state_dict"].items()}
        ((R.forward(p, x1.to(dt), sp, True)[0] * c1.to(dt)).sum() + (R.forward(p, x2.to(dt), sp, True)[0] ** 2 * c2.to(dt)).sum()).backward()
        ref[dt] = {k: v.grad for k, v in p.items()}
        first = {k: v.detach().clone().requires_grad_() for k, v in p.items()}
        (R.forward(first, x1.to(dt), sp, True)[0] * c1.to(dt)).sum().backward()
        ref[dt, "first"] = {k: v.grad for k, v in first.items()}
    model = make(cfg, golden)
    model.load_state_dict(cfg["state_dict"], strict=True)
    model.to(DEV).train()
    ((model(dev(x1)) * dev(c1)).sum() + (model(dev(x2)) ** 2 * dev(c2)).sum()).backward()
    got = {k: p.grad.clone() for k, p in model.named_parameters()}
    check([(k, rel_l2(ref[torch.float32][k], ref[torch.float64][k]), rel_l2(got[k], ref[torch.float64][k])) for k in got], "two forwards, one backward")
    names, params = zip(*model.named_parameters())
    held = torch.autograd.grad((model(dev(x1)) * dev(c1)).sum(), params)
    copies = [h.clone() for h in held]
    (model(dev(x2)) ** 2 * dev(c2)).sum().backward()                                # rewrites the gradient arena
    assert all(torch.equal(h, c) for h, c in zip(held, copies))
    check([(k, rel_l2(ref[torch.float32, "first"][k], ref[torch.float64, "first"][k]), rel_l2(h, ref[torch.float64, "first"][k])) for k, h in zip(names, held)],
          "autograd.grad, held across a backward")


@pytest.mark.parametrize("task", ["DeepLoc2", "DeepLoc10"])
def test_predict_binary_and_multiclass(task):
    """ref predict_step: sigmoid of the squeezed output [N] (binary), the argmax class int64 [N] (multiclass), in eval mode, over more than one slab; against
    the fp64 restatement on the same weights.  A class is compared where the fp64 margin between the two best logits exceeds 1e-4."""
    out_dim = probe.OUTPUT_DIMS[task]
    torch.manual_seed(12)
    model = probe.MLP(24, out_dim, [16, 8], 0.25, True, False, "leaky_relu", True)
    with torch.no_grad():
        for m in model._bn_modules():
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.8, 1.2)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rows = probe.EVAL_SLAB + 37
    x = torch.randn(rows, 24, generator=torch.Generator().manual_seed(13))
    model.train()
    pred = probe.predict(model, task, x.numpy())
    assert model.training and pred.is_cuda and pred.shape == (rows,)                # the mode the caller left is put back
    sp = R.spec([16, 8], "batch", "leaky_relu", True, 0.25)
    with torch.no_grad():
        l64 = R.forward({k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}, x.double(), sp, False)[0]
        l32 = R.forward(sd, x, sp, False)[0]
    if task == "DeepLoc2":
        assert pred.dtype == torch.float32
        check([("sigmoid", rel_l2(torch.sigmoid(l32.squeeze(1)), torch.sigmoid(l64.squeeze(1))), rel_l2(pred, torch.sigmoid(l64.squeeze(1))))], "predict DeepLoc2")
        res = downstream.evaluate_predictions(task, pred, (torch.sigmoid(l64.squeeze(1)) > 0.5).long(), "test")
        assert set(res) == {"test_accuracy", "test_f1_micro", "test_auc"} and res["test_accuracy"] > 0.999
    else:
        assert pred.dtype == torch.int64
        top = l64.topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 1e-4
        assert int(clear.sum()) > rows - 10 and torch.equal(pred.cpu()[clear], l64.argmax(1)[clear])
        assert len(set(pred.cpu().tolist())) > 3


# ---------------------------------------------------------------------------------------------------------------------------------
FIT_ROWS, FIT_VALID, FIT_BATCH, FIT_EPOCHS, FIT_LR, FIT_SEED = 44, 12, 8, 3, 1e-3, 20240
FIT_TASKS = {"batch": "DeepLoc10", "layer": "ThermoStability", "none": "DeepLoc2"}


def _fit_data(task, gen):
    x, xv = torch.randn(FIT_ROWS, 24, generator=gen), torch.randn(FIT_VALID, 24, generator=gen)
    if task == "DeepLoc10":
        return (x, torch.randint(0, 10, (FIT_ROWS,), generator=gen)), (xv, torch.randint(0, 10, (FIT_VALID,), generator=gen))
    if task == "DeepLoc2":
        return (x, torch.randint(0, 2, (FIT_ROWS,), generator=gen)), (xv, torch.randint(0, 2, (FIT_VALID,), generator=gen))
    return (x, torch.randn(FIT_ROWS, generator=gen)), (xv, torch.randn(FIT_VALID, generator=gen))


@pytest.mark.parametrize("norm", ["batch", "layer", "none"])
def test_whole_fit_vs_the_fp64_fit(norm):
    task = FIT_TASKS[norm]
    out_dim, kind = probe.OUTPUT_DIMS[task], probe.task_dims(task, "esm2")[2]
    gen = torch.Generator().manual_seed(3)
    train, valid = _fit_data(task, gen)
    torch.manual_seed(5)
    model = probe.MLP(24, out_dim, [16, 8], 0.25, norm == "batch", norm == "layer", "gelu", True)
    assert model.residual_projection is not None
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    history = probe.fit(model, task, train, valid, learning_rate=FIT_LR, batch_size=FIT_BATCH, max_epochs=FIT_EPOCHS, early_stopping_patience=20, seed=FIT_SEED)
    final = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    g = torch.Generator(device=DEV).manual_seed(FIT_SEED)                           # the permutations fit() drew
    perms = [torch.randperm(FIT_ROWS, generator=g, device=DEV).cpu() for _ in range(FIT_EPOCHS)]
    sp = R.spec([16, 8], norm, "gelu", True, 0.25)
    mask_fn = lambda call, layer, M, n: R.keep_mask(M, n, 0.25, FIT_SEED, model.stream_of(call, layer))
    tr = (train[0], train[1] if kind == 2 else train[1].float()[:, None])
    va = (valid[0], valid[1] if kind == 2 else valid[1].float()[:, None])
    ref = {dt: R.fit(sd0, sp, kind, tr, va, perms, mask_fn, learning_rate=FIT_LR, batch_size=FIT_BATCH, dtype=dt) for dt in (torch.float64, torch.float32)}
    v64, best64, sd64 = ref[torch.float64]
    v32, _, sd32 = ref[torch.float32]
    assert [h["lr"] for h in history] == [FIT_LR] * FIT_EPOCHS and len(history) == FIT_EPOCHS            # exact
    assert max(e for e, h in enumerate(history) if h["best"]) == best64                                 # the restored epoch
    rows = [("val_loss history", rel_l2(torch.tensor(v32), torch.tensor(v64)), rel_l2(torch.tensor([h["val_loss"] for h in history]), torch.tensor(v64)))]
    steps = FIT_EPOCHS * ((FIT_ROWS + FIT_BATCH - 1) // FIT_BATCH)
    zero = {f"hidden_layers.{lin}.bias" for lin, _ in R.layer_names(sp)} if norm == "batch" else set()
    for k, v in sd64.items():
        if k.endswith("num_batches_tracked"):
            assert int(final[k]) == int(v)
        elif k in zero:
            assert float((final[k].double() - v).abs().max()) <= 1.1 * steps * FIT_LR, k
        else:
            rows.append((k, rel_l2(sd32[k], v), rel_l2(final[k], v)))
    check(rows, f"fit {norm}")


# ---------------------------------------------------------------------------------------------------------------------------------
def _eval_cfg(task, seed=9):
    return {"task_name": task, "model_type": "oneprot_9", "seed": seed,
            "model": dict(hidden_dims=[16], dropout_rate=0.1, use_batch_norm=True, use_layer_norm=False, activation="relu", use_residual=False, learning_rate=1e-2,
                          batch_size=32, max_epochs=2, early_stopping_patience=20)}


def _eval_data(task):
    gen = torch.Generator().manual_seed(17)
    data = {}
    Wt = torch.randn(256, 320, generator=gen)
    for part, rows in (("train", 96), ("valid", 32), ("test", 32)):
        x = torch.randn(rows, 256, generator=gen)
        data[f"{part}_emb"] = x.numpy()
        data[f"{part}_target"] = ((x @ Wt) > 16.0).float().numpy() if task == "GO-CC" else (x[:, :8].sum(1) + 0.1 * torch.randn(rows, generator=gen)).numpy()
    return data


@pytest.mark.parametrize("task", ["GO-CC", "ThermoStability"])
def test_evaluate_keys_metrics_and_determinism(task):
    data = _eval_data(task)
    res = probe.evaluate(_eval_cfg(task), data)
    model, history = probe.evaluate.last
    keys = {"GO-CC": ["f1_max"], "ThermoStability": ["mse", "r2", "spearman_rho"]}[task]
    assert set(res) == {f"{part}_{k}" for part in ("valid", "test") for k in keys}
    pred = probe.predict(model, task, data["test_emb"])
    want = downstream.evaluate_predictions(task, pred, data["test_target"], "test")
    first = "test_f1_max" if task == "GO-CC" else "test_spearman_rho"
    assert res[first] == want[first] and all(res[k] == want[k] for k in want)
    assert len(history) == 2 and all(torch.isfinite(torch.tensor(h["val_loss"])) for h in history)
    arena = model.arena().clone()
    res2 = probe.evaluate(_eval_cfg(task), data)                                   # the same seed: the same bits
    assert res2 == res and torch.equal(probe.evaluate.last[0].arena(), arena)
    assert [h["val_loss"] for h in probe.evaluate.last[1]] == [h["val_loss"] for h in history]


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["batch", "layer", "none"])
@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("H", [1, 2])
def test_launch_bound_of_one_optimiser_step(H, projected, norm, monkeypatch):
    """at most 5 H + 8 kernel launches per step (5 H + 10 with the residual projection), nothing copied to the host.  Every hip.call is one launch except the loss
    (partials + the ordered finish: two); the BatchNorm step counters are one torch foreach launch more."""
    hidden = [16, 8][:H] if projected else [16, 24][-H:]
    model = probe.MLP(24, 10, hidden, 0.25, norm == "batch", norm == "layer", "relu", True).to(DEV)
    assert (model.residual_projection is not None) == projected
    gen = torch.Generator().manual_seed(2)
    x, y = dev(torch.randn(64, 24, generator=gen)), dev(torch.randint(0, 10, (64,), generator=gen))
    idx = dev(torch.randperm(64, generator=gen)[:32].to(torch.int32))
    opt = FusedAdamW([model.arena()], lr=1e-3)
    loss_sum, ws = torch.zeros(1, dtype=torch.float64, device=DEV), hip.probe_loss_workspace(DEV)
    model.train()
    model.train_step(x, y, idx, hip.PROBE_LOSS_CE, opt, loss_sum, ws)             # the optimiser state exists from here on
    before = model.arena().clone()
    calls, real = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])

    def refuse(*a, **k):
        raise AssertionError("a readback inside the step")
    monkeypatch.setattr(torch.Tensor, "cpu", refuse)
    monkeypatch.setattr(torch.Tensor, "item", refuse)
    monkeypatch.setattr(torch.Tensor, "tolist", refuse)
    model.train_step(x, y, idx, hip.PROBE_LOSS_CE, opt, loss_sum, ws)
    monkeypatch.undo()
    launches = len(calls) + calls.count("oneprot_probe_loss_fwd_bwd") + (1 if norm == "batch" else 0)
    bound = 5 * H + (10 if projected else 8)
    print(f"H={H} projected={projected} {norm}: {launches} launches (bound {bound}): {calls}")
    assert launches <= bound and calls.count("oneprot_adamw_step") == 1
    assert not torch.equal(model.arena(), before) and bool(torch.isfinite(model.arena()).all()) and float(loss_sum) > 0
