"""CPU: the premise of the mix-instruction form of the f16x2 split (csrc/encoder_x3.h: h2_split_pair).  The second piece is
lo = f16(a - f32(hi)) with hi = f16(a); the kernels form it as ONE fused multiply-add fma(f32(hi), -1, a) rounded once to fp16
where the reference form rounds a - f32(hi) to fp32 first.  The two agree on every input iff that fp32 remainder is exact: checked
here on every finite non-negative fp16 value, every rounding midpoint, their fp32 neighbours and 3.9 M random values with exponents
from -40 to 16 (h2_split_cases.inputs) -- no exceptions."""
import numpy as np
import pytest

import h2_split_cases as H


@pytest.fixture(scope="module")
def a():
    return H.inputs()


def test_the_input_set_is_the_described_one(a):
    assert a.size > 4_000_000
    f16 = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
    assert np.isin(f16, a).all() and np.isin(np.nextafter(f16, np.float32(np.inf)), a).all()
    assert np.isin(np.float32([65520.0, 2.0 ** -25, 3 * 2.0 ** -25]), a).all()              # midpoints: top, lowest two
    e = np.frexp(a[-H.RANDOM:])[1] - 1
    assert e.min() == -40 and e.max() == 16


def test_model_rounds_the_first_piece_to_nearest_even(a):
    hi, _ = H.model(a)
    h = hi.view(np.float16).astype(np.float64)
    a64 = a.astype(np.float64)
    fin = np.isfinite(h)
    assert (~fin == (a >= H.F16_INF_FROM)).all()                                            # overflow exactly from 65520 on
    # nearest: no other fp16 value is closer; a tie went to the even significand
    with np.errstate(over="ignore"):                                                        # (65504's upper neighbour: inf)
        up = np.nextafter(hi.view(np.float16), np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(hi.view(np.float16), np.float16(-np.inf)).astype(np.float64)
    up[~np.isfinite(up)] = 65536.0
    err = np.abs(a64 - h)
    assert (err[fin] <= np.abs(a64 - up)[fin]).all() and (err[fin] <= np.abs(a64 - dn)[fin]).all()
    tie = fin & ((err == np.abs(a64 - up)) | (err == np.abs(a64 - dn))) & (err > 0)
    assert tie.sum() >= 31743 and ((hi[tie] & 1) == 0).all()


def test_the_fp32_remainder_is_exact_so_one_rounding_equals_two(a):
    hi, lo = H.model(a)
    fin = np.isfinite(hi.view(np.float16))
    r64 = a.astype(np.float64)[fin] - hi.view(np.float16).astype(np.float64)[fin]          # exact: both within 53 bits of each other
    r32 = a[fin] - hi.view(np.float16).astype(np.float32)[fin]
    assert (r32.astype(np.float64) == r64).all()                                            # the premise
    once = r64.astype(np.float16)                                                           # the fused form: one rounding
    assert (once.view(np.uint16) == lo[fin]).all()                                          # = the reference form, word for word
    # an overflowed first piece: the remainder is -inf in either form
    assert (lo[~fin] == 0xfc00).all()


def test_the_pieces_leave_a_remainder_below_the_error_bound(a):
    """encoder_x3.h ERROR BOUND: |x - x0 - x1| <= 2^-23 |x| for x >= 2^-2, <= 2^-25 absolute below."""
    hi, lo = H.model(a)
    fin = np.isfinite(hi.view(np.float16))
    x = a.astype(np.float64)[fin]
    rem = np.abs(x - hi.view(np.float16).astype(np.float64)[fin] - lo.view(np.float16).astype(np.float64)[fin])
    assert (rem <= np.where(x >= 0.25, x * 2.0 ** -23, 2.0 ** -25)).all()
