"""Inputs and numpy model of the f16x2 split (csrc/encoder_x3.h: h2_split_pair), shared by test_h2_split_host.py and
test_gpu_h2_split_bits.py.  Not a test module."""
import numpy as np

RANDOM = 3_900_000
F16_INF_FROM = np.float32(65520.0)            # the first fp32 value that rounds (to nearest even) to the fp16 infinity


def _with_neighbours(v):
    v = v.astype(np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def inputs():
    """~4.1 M non-negative finite fp32 values: every finite non-negative fp16 value (subnormals included) and its fp32 neighbours,
    every rounding midpoint between two consecutive fp16 values (the one between 65504 and 2^16 included) and its neighbours, and
    random values with exponents from -40 to 16."""
    f16 = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)          # 0 ... 65504, ascending
    mid = (np.concatenate([f16, [65536.0]])[1:] + f16) / 2                                  # exact in fp32 (12 significant bits)
    assert (mid.astype(np.float32).astype(np.float64) == mid).all() and mid[-1] == float(F16_INF_FROM)
    grid = np.concatenate([_with_neighbours(f16), _with_neighbours(mid)])
    grid = grid[grid >= 0]                                                                    # (the neighbour below zero)
    rng = np.random.default_rng(20240612)
    mant = rng.integers(0, 1 << 23, RANDOM, dtype=np.uint32)
    expo = rng.integers(-40, 17, RANDOM).astype(np.int64)
    rnd = ((expo + 127).astype(np.uint32) << np.uint32(23) | mant).view(np.float32)
    out = np.concatenate([grid, rnd]).astype(np.float32)
    assert np.isfinite(out).all() and (out >= 0).all()
    return out


def edge_inputs():
    """What the GPU test adds: the zeros, the ends of the fp16 subnormal range, the largest finite fp16 value, the first fp32
    values that round to the fp16 infinity, and +inf."""
    sub = np.array([2.0 ** -24, 2.0 ** -25, 1023 * 2.0 ** -24, 2.0 ** -14], np.float32)
    top = np.array([65504.0, 65519.996, F16_INF_FROM, np.nextafter(F16_INF_FROM, np.float32(np.inf)), 65536.0, 1e9, np.inf], np.float32)
    return np.concatenate([np.array([0.0, -0.0], np.float32), _with_neighbours(sub), top])


def model(a):
    """(hi, lo) as uint16 bit patterns: hi = f16(a) rounded to nearest even, lo = f16(a - f32(hi)) with the subtraction in fp32.
    A NaN piece is written as the default quiet NaN 0x7e00 (numpy's inf - inf carries the host's sign)."""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = a.astype(np.float16)
        lo = (a - hi.astype(np.float32)).astype(np.float16)
    hi_w, lo_w = hi.view(np.uint16).copy(), lo.view(np.uint16).copy()
    hi_w[np.isnan(hi)] = 0x7e00
    lo_w[np.isnan(lo)] = 0x7e00
    return hi_w, lo_w
