"""CPU: tests/_emd_model64.py (the float32 pair terms of MatchCostGrad in numpy) against the C oracle, so that the GPU tests of
tests/test_gpu_emd_limits.py may lean on it.

  * its terms, negated and summed l ascending in float32, ARE the oracle's grad1 bit for bit: the terms are the oracle's own;
  * the oracle's grad2 -- the same terms added k ascending in float32, n - 1 additions on the longest path -- lies within
    n * 2^-24 * sum |t| of the helper's float64 sum (first-order bound of a recursive sum; measured <= 0.15 of it at the shapes below)."""
import numpy as np
import pytest

import _emd_model64 as model
from conftest import cloud


def _clouds(kind, b, n, m):
    x1, x2 = cloud(100 + n, b, n), (np.float32(0.7) * cloud(200 + m, b, m)).astype(np.float32)
    if kind == "coincident":
        x2[0, : min(n, m) // 2] = x1[0, : min(n, m) // 2]             # distance 0: the 1e-20 clamp, 0 / 1e-20
        x1[1, :8] *= np.float32(1e-20)                                 # a knot around the origin: denormal squares
        x2[1, :8] = x1[1, :8][::-1] * np.float32(1.5)
    return x1, x2


@pytest.mark.parametrize("kind,b,n,m", [("uniform", 2, 1, 5), ("uniform", 2, 5, 1), ("uniform", 2, 63, 17), ("uniform", 2, 130, 77),
                                         ("uniform", 1, 257, 1039), ("uniform", 1, 2051, 300), ("coincident", 2, 120, 90)])
def test_model_terms_are_the_oracles(oracle, kind, b, n, m):
    x1, x2 = _clouds(kind, b, n, m)
    match = oracle.approx_match(x1, x2)
    g1, g2 = oracle.match_cost_grad(x1, x2, match)
    t = model.grad_terms(x1, x2, match)
    assert np.isfinite(t).all()
    assert np.array_equal(model.grad1_f32(t).view(np.int32), g1.view(np.int32))
    s64, sabs = model.grad2_f64(t)
    err = np.abs(g2.astype(np.float64) - s64)
    bound = model.grad2_bound(sabs, n)
    print("n=%d m=%d: oracle grad2 at most %.3f of n * 2^-24 * sum|t|" % (n, m, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()

