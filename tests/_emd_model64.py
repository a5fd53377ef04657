"""numpy model of the pair terms of MatchCostGrad (tf_approxmatch.cpp:106-140), for tests/test_gpu_emd_limits.py.

A term is t[k, l] = w * (o / d) with o = q_l - p_k, d = max(sqrtf(ox ox + oy oy + oz oz), 1e-20) and w = match[k, l], every
operation a float32 one rounded on its own -- three products, a left-to-right sum, sqrt, the clamp, a divide, a multiply: what
emd_grad1_kernel / emd_grad2_kernel (csrc/emd.hip, contraction off) and the CPU op both do, so the terms are the kernels' bit
for bit and only the ORDER of a sum is left to compare:
  * grad1[k] = -sum_l t[k, l], l ascending in float32 (the CPU's and the kernel's order): reproduced exactly by grad1_f32();
  * grad2[l] = sum_k t[k, l]: the kernel's lanes stride k by 64 and fold in six butterfly steps, the CPU adds k ascending.
    grad2_f64() sums the float32 terms in float64 and returns sum |t| next to it, for the first-order bound of a float32 sum
    of those terms in any of these orders (grad2_bound())."""
import numpy as np

F = np.float32


def grad_terms(xyz1, xyz2, match_nm):
    """xyz1 (b, n, 3), xyz2 (b, m, 3), match in the CPU layout (b, n, m) -> float32 terms (b, n, m, 3)."""
    p = np.ascontiguousarray(xyz1, dtype=F)[:, :, None, :]
    q = np.ascontiguousarray(xyz2, dtype=F)[:, None, :, :]
    w = np.ascontiguousarray(match_nm, dtype=F)[..., None]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        o = q - p                                                       # (b, n, m, 3) float32
        sq = o * o
        d = np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])             # left to right
        d = np.where(d < F(1e-20), F(1e-20), d).astype(F)[..., None]   # the kernels' form of std::max(d, 1e-20f): a NaN d stays
        t = w * (o / d)
    assert t.dtype == F
    return t


def grad1_f32(terms):
    """-sum over l, l ascending, in float32: (b, n, 3)."""
    g = np.zeros(terms.shape[:2] + (3,), F)
    for l in range(terms.shape[2]):
        g = g - terms[:, :, l, :]
    assert g.dtype == F
    return g


def grad2_f64(terms):
    """(sum over k in float64, sum over k of |t| in float64), each (b, m, 3)."""
    t = terms.astype(np.float64)
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def grad2_bound(sum_abs, adds):
    """|float32 sum of the terms - their float64 sum| <= adds * 2^-24 * sum |t| to first order: every partial sum is at most
    sum |t|, and each of the `adds` additions on the longest path from a term to the result rounds by at most 2^-24 of it."""
    return adds * 2.0 ** -24 * sum_abs
