"""Every consumer of the element rule of csrc/philox.h draws the mask tests/philox_ref.py gives, at the smallest shapes that cross a Philox block inside a row,
for one (seed, stream) whose high 32-bit words are both non-zero and p = 0.3.  All mask comparisons are exact.  The Box-Muller normals of
oneprot_clipped_normal_add_f32 are fp32 on the device and fp64 in tests/pronet_rng_ref.py, so that one comparison carries the absolute tolerance 1e-5 of
tests/test_pronet_kernels_gpu.py::test_noise_add_and_the_plain_calls (the same comparison at 770 x 128).  At sigma 1 that is still loose: |normal| <= 5.8, the fp32
angle 2 pi u carries at most 2^-24 x 6.3 = 3.8e-7 rad, so a normal is off by about 2e-6 plus a few roundings of its own."""
import numpy as np
import pytest
import torch

from oneprot_amd import hip
from tests import philox_ref as PR
from tests import pronet_rng_ref as RNG
from tests.gbt_cases import slices16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, SEED, STREAM = 0.3, 0x1E3779B97F4A7C15, (5 << 60) | (0x1234 << 44) | 77
N = 40                    # five blocks
THR, SCALE = PR.dropout_threshold(P)
KEEP = torch.from_numpy(PR.philox_keep(N, P, SEED, STREAM))


def _expect(y, scale):
    """keep = output non-zero, and kept values equal scale exactly"""
    y = y.cpu()
    assert torch.equal(y != 0, KEEP.reshape(y.shape)) and 0 < int(KEEP.sum()) < N
    assert torch.equal(y[y != 0], torch.full((int(KEEP.sum()),), float(scale)).to(y.dtype))


def test_reference_constants():
    assert SEED >> 32 and STREAM >> 32 and THR == 19661 and SCALE == np.float32(65536.0) / np.float32(45875.0)


@pytest.mark.parametrize("entry", ["oneprot_dropout_f32", "oneprot_dropout_add_f32", "oneprot_dropout_bwd_add_f32"])
def test_fp32_outputs(entry):
    ones, y = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    if entry == "oneprot_dropout_f32":
        hip.call(entry, ones, y, N, P, SEED, STREAM)
    elif entry == "oneprot_dropout_add_f32":
        hip.call(entry, ones, torch.zeros(N, device=DEV), y, N, P, SEED, STREAM)
    else:
        hip.call(entry, ones.to(torch.bfloat16), y, N, P, SEED, STREAM)
    _expect(y, SCALE)


@pytest.mark.parametrize("entry", ["oneprot_dropout_bf16", "oneprot_dropout_bwd_add_bf16"])
def test_bf16_outputs(entry):
    ones, y = torch.ones(N, dtype=torch.bfloat16, device=DEV), torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    hip.call(entry, ones, y, N, P, SEED, STREAM)
    _expect(y, torch.tensor(float(SCALE)).to(torch.bfloat16))          # the one rounding of the store


def test_dropout_add_layernorm_sum():
    T, d = 5, 8
    g = torch.Generator().manual_seed(3)
    resid = torch.randn(T, d, generator=g).to(DEV)
    s, y = torch.empty(T, d, device=DEV), torch.empty(T, d, device=DEV)
    hip.call("oneprot_dropout_add_layernorm_fwd", torch.ones(T, d, device=DEV), resid, s, torch.ones(d, device=DEV), torch.zeros(d, device=DEV), None, y, None, None,
             T, d, 1e-12, P, SEED, STREAM)
    keep = KEEP.reshape(T, d).to(DEV)
    assert torch.equal(s, torch.where(keep, resid + float(SCALE), resid))       # 0 + resid and scale + resid: one fp32 addition each, as torch's
    assert torch.equal((s - resid) != 0, keep)


def test_probe_rownorm_mask():
    M, n = 3, 13              # 39 elements: the flat index leaves a block mid-row, n is no multiple of 8
    g = torch.Generator().manual_seed(4)
    z, y = torch.randn(M, n, generator=g).to(DEV), torch.empty(M, n, device=DEV)
    hip.probe_rownorm_act_fwd(z, torch.ones(n, device=DEV), torch.full((n,), 10.0, device=DEV), y, M, n, act=hip.PROBE_ACT["identity"], rng=(P, SEED, STREAM))
    assert torch.equal((y != 0).cpu().reshape(-1), KEEP[:M * n])                # |LayerNorm(z)| <= sqrt(n - 1) < 10: no normalised value + beta is zero


def test_gbt_sample_slices():
    rows, F, feat_stream = 40, 13, STREAM + 1
    rk, fk, fu = torch.empty(rows, dtype=torch.uint8, device=DEV), torch.empty(F, dtype=torch.uint8, device=DEV), torch.empty(F, dtype=torch.int32, device=DEV)
    hip.call("oneprot_gbt_sample", rk, fk, fu, rows, F, 0.5, 6, SEED, STREAM, feat_stream)
    assert np.array_equal(fu.cpu().numpy(), slices16(F, SEED, feat_stream))
    assert np.array_equal(rk.cpu().numpy().astype(bool), slices16(rows, SEED, STREAM) < 0.5 * 65536)


def test_clipped_normal_blocks():
    y = torch.empty(8, device=DEV)
    hip.call("oneprot_clipped_normal_add_f32", torch.zeros(8, device=DEV), y, 8, 1.0, 100.0, SEED, STREAM)
    want = torch.from_numpy(RNG.normals4(2, SEED, STREAM).reshape(-1))
    err = float((y.cpu().double() - want).abs().max())
    print(f"clipped normals: max abs error {err:.3e}")
    assert err <= 1e-5 and float(want.abs().max()) < 100.0
