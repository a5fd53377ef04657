"""CPU: the numpy model of the kNN outlier loss (tests/_knn_loss_model.py, the rule of geoadv_knn_outlier_loss in
include/geoadv.h) against torch float64 autograd, against the SOR model, and on the cases with a known answer.  The neighbours
come from a brute-force fp32 search."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_loss_model as M  # noqa: E402
import _stat_defense_model as S  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("n,k,alpha", [(33, 4, 0.0), (257, 15, 1.05), (1500, 5, 1.05)])
def test_gradient_is_float64_autograd_with_the_mask_held_constant(n, k, alpha):
    """TOLERANCE: both sides accumulate in float64 (they differ by the order of a few dozen additions, about 1e-16 relative); the
    model then rounds ONCE to fp32, so every component lies within one fp32 ulp of the float64 value (+ 1e-30 absolute)."""
    import torch
    x = np.stack([M.cloud_of_kind("random", n, 10 * n + c) for c in range(2)])
    idx = M.brute_idx(x, k)
    out = M.knn_outlier_loss(x, idx, k, alpha)
    assert out["mask"].any(axis=1).all()
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    nb = xt[torch.arange(2)[:, None, None], torch.from_numpy(idx.astype(np.int64))]
    score = ((xt[:, :, None, :] - nb) ** 2).sum(-1).mean(-1)
    K = (score * torch.from_numpy(out["mask"].astype(np.float64))).sum(1) / n
    K.sum().backward()
    g64 = xt.grad.numpy()
    ulp = np.spacing(np.abs(g64).astype(np.float32)).astype(np.float64)
    err = np.abs(out["grad"].astype(np.float64) - g64)
    print("largest error in ulps:", (err / ulp).max())
    assert (err <= ulp + 1e-30).all()
    assert np.allclose(out["loss"], K.detach().numpy(), rtol=1e-6, atol=0)      # (the model's scores are sums of fp32 distances)
    assert (out["grad"][~out["mask"] & (M.in_degree(idx, out["mask"]) == 0)].view(np.uint32) == 0).all()


@pytest.mark.parametrize("n,k,alpha", [(33, 4, 0.0), (257, 15, 1.05), (1500, 5, 1.05), (1500, 1, 1.1)])
def test_mask_is_the_complement_of_sor_inliers(n, k, alpha):
    x = np.stack([M.cloud_of_kind(kind, n, n) for kind in ("random", "lattice", "pairs")])
    x[0, 3, 1] = np.nan
    x[0, 7, 0] = np.inf
    idx = M.brute_idx(x, k)
    out = M.knn_outlier_loss(x, idx, k, alpha)
    inl, (mu, var, m) = S.sor_inliers(out["score"], alpha)
    fin = np.isfinite(out["score"])
    assert not fin.all() and np.array_equal(out["mask"][fin], ~inl[fin]) and not out["mask"][~fin].any()
    assert np.array_equal(_bits(out["stats"][:, :3]), _bits(np.stack([mu, var, m.astype(np.float64)], axis=1)))
    assert np.array_equal(out["stats"][:, 3], out["mask"].sum(1))


def test_empty_mask_gives_zero_loss_and_zero_bits():
    x = M.cloud_of_kind("random", 300, 1)[None]
    out = M.knn_outlier_loss(x, M.brute_idx(x, 5), 5, 1e6)
    assert not out["mask"].any()
    assert _bits(out["loss"]).tolist() == [0] * 8 and not _bits(out["grad"]).any()


def test_hub_case():
    x = M.hub_cloud()[None]
    idx = M.brute_idx(x, 5)
    out = M.knn_outlier_loss(x, idx, 5, 0.5)
    assert np.array_equal(np.flatnonzero(out["mask"][0]), np.arange(5, 17))
    assert M.in_degree(idx, out["mask"])[0].tolist() == [12] * 5 + [0] * 12
    # every vertex is at distance 1 from the origin points: score 1, and the origin points are pushed away from all twelve
    assert np.allclose(out["score"][0, 5:], 1.0, rtol=1e-6) and np.isclose(out["loss"][0], 12.0 / 17.0, rtol=1e-6)
    assert np.abs(out["grad"][0, :5]).max() < 1e-6          # the vertices sum to zero
    assert np.allclose(out["grad"][0, 5:], 2.0 / (17 * 5) * 5 * x[0, 5:], rtol=1e-5)
