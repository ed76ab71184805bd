"""tests/gate.py on 2 x 3 tensors: what `close` lets through and what it does not, and that rel_l2 of a NaN passes no threshold."""
import math

import pytest
import torch

from tests.gate import close, cos_sim, rel_l2

REF = torch.tensor([[1.0, -2.0, 4.0], [0.5, 8.0, -16.0]], dtype=torch.float64)
RTOL, ATOL = 2.0 ** -7, 2.0 ** -4           # powers of two on powers of two: atol + rtol |ref| is exact in fp64


def at_boundary():
    return REF + (ATOL + RTOL * REF.abs())


def test_passes_at_exactly_the_boundary_and_returns_the_largest_error():
    assert close(at_boundary(), REF, RTOL, ATOL, "boundary") == ATOL + RTOL * 16.0
    assert close(REF, REF, 0.0, 0.0, "equal") == 0.0


def test_fails_one_ulp_beyond_the_boundary():
    got = at_boundary()
    got[1, 1] = math.nextafter(float(got[1, 1]), math.inf)
    with pytest.raises(AssertionError, match=r"one ulp: 1/6 off \(0 NaN in got\), first at \(1, 1\) of \(2, 3\)"):
        close(got, REF, RTOL, ATOL, "one ulp")


def test_fails_on_nan_in_got():
    got = REF.clone()
    got[0, 2] = float("nan")
    with pytest.raises(AssertionError, match=r"1/6 off \(1 NaN in got\), first at \(0, 2\)"):
        close(got, REF, 1.0, 1e30, "nan in got")
    with pytest.raises(AssertionError, match=r"6/6 off \(6 NaN in got\)"):
        close(torch.full((2, 3), float("nan")), torch.ones(2, 3), 1.0, 1e30, "all nan")


def test_fails_on_nan_in_ref():
    ref = REF.clone()
    ref[1, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"1/6 off \(0 NaN in got\), first at \(1, 0\)"):
        close(REF, ref, 1.0, 1e30, "nan in ref")


def test_fails_on_inf_against_inf():
    got, ref = REF.clone(), REF.clone()
    got[0, 0] = ref[0, 0] = float("inf")
    with pytest.raises(AssertionError, match=r"1/6 off"):
        close(got, ref, 1.0, 1e30, "inf - inf")


def test_fails_on_a_shape_that_would_broadcast():
    with pytest.raises(AssertionError, match=r"shape \(3,\) vs \(2, 3\)"):
        close(REF[0], REF.expand(2, 3) * 0 + REF[0], 0.0, 0.0, "broadcast")


def test_tensor_atol_holds_per_element():
    atol = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 0.5]], dtype=torch.float64)
    got = REF.clone()
    got[0, 0] += 1.0
    got[1, 2] -= 0.5
    assert close(got, REF, 0.0, atol, "per element") == 1.0
    got[0, 1] += 0.25                          # inside the largest atol, outside its own
    with pytest.raises(AssertionError, match=r"1/6 off .*first at \(0, 1\)"):
        close(got, REF, 0.0, atol, "per element")
    assert close(got, REF, 0.0, atol[:, :1] + 0.5, "a column that broadcasts") == 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64])
def test_accepts_every_float_type_of_got(dtype):
    got = REF.to(dtype)                        # every value of REF is a bf16 number
    assert close(got, REF, 0.0, 0.0, str(dtype)) == 0.0
    with pytest.raises(AssertionError):
        close(got * 2, REF, 0.0, 0.0, str(dtype))


def test_rel_l2_of_a_nan_is_below_no_threshold():
    a = REF.clone()
    a[0, 0] = float("nan")
    assert not rel_l2(a, REF) < 1e30 and not rel_l2(REF, a) < 1e30
    assert rel_l2(REF, REF) == 0.0 and rel_l2(REF * 1.5, REF) == 0.5
    assert abs(cos_sim(REF, REF * 3) - 1.0) < 1e-15 and abs(cos_sim(REF, -REF) + 1.0) < 1e-15
