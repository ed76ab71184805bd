"""The suite's comparisons against a reference, once: the elementwise gate `close`, the relative L2 error and the cosine.

`close` computes in fp64 on the device of `ref` (a reference kept on the GPU is compared on the GPU) and counts as bad every element that is NOT
within the tolerance, so a NaN on either side, or inf - inf, fails.  It has no special case for infinities: a site that holds an infinity on both
sides sends its finite positions through `close` and asserts torch.equal on the rest."""
import torch

F64 = torch.float64


def close(got, ref, rtol, atol, msg=""):
    """|got - ref| <= atol + rtol |ref| for every element; atol is a number or a tensor that broadcasts.  Returns the largest error."""
    ref = ref.detach().to(F64)
    got = got.detach().to(device=ref.device, dtype=F64)
    assert got.shape == ref.shape, f"{msg}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if torch.is_tensor(atol):
        atol = atol.to(ref.device)
    err = (got - ref).abs_()
    tol = ref.abs().mul_(rtol)
    ok = err <= (tol + atol if torch.is_tensor(atol) else tol.add_(atol))
    n = ok.numel() - int(ok.sum())
    if n:
        bad = ~ok
        first = int(bad.flatten().nonzero()[0])
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(first), bad.shape))
        finite = err[torch.isfinite(err)]
        raise AssertionError(f"{msg}: {n}/{bad.numel()} off ({int(torch.isnan(got).sum())} NaN in got), first at {idx} of {tuple(bad.shape)}: "
                             f"got {float(got.flatten()[first]):.6g} want {float(ref.flatten()[first]):.6g}, "
                             f"max finite err {float(finite.max()) if finite.numel() else float('nan'):.3e}, ref max {float(ref.abs().max()):.3e}")
    return float(err.max()) if err.numel() else 0.0


def rel_l2(a, ref):
    """|a - ref| / |ref| in fp64 on the host; NaN for a NaN input, which is `<` no threshold"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def cos_sim(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))
