"""CPU: the numpy model of the kNN loss's SURFACE rule (tests/_surface_loss_model.py, the rule of GEOADV_KNN_LOSS_SURFACE in
include/geoadv.h) against a float64 torch autograd of  sum_p w_p (mean_c |x_p - x_N[p][c]| - thr) / n  with mask and neighbours
held fixed; its mask against numpy's own float32 mean of the fp32 distances (what the reference's defense computes); and the
dodecahedron hub's in-degrees.  Host-side carriers of the rule too: Configuration, run_attack's flags, the struct mirror."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_loss_model as M  # noqa: E402
import _surface_loss_model as SM  # noqa: E402

N = 256


def _median_thr(x, idx, k):
    return np.float32(np.median(SM.scores(SM.dists(x, idx), k)[0]))


@pytest.mark.parametrize("k", [1, 2, 7])
def test_model_against_float64_autograd(k):
    import torch
    x = np.stack([SM.cloud_of_kind("random", N, 40 + k)])
    idx = M.brute_idx(x, k)
    thr = _median_thr(x, idx, k)
    out = SM.surface_loss(x, idx, k, thr)
    w = out["mask"]
    assert 100 <= int(w.sum()) <= 156

    xt = torch.tensor(x[0].astype(np.float64), requires_grad=True)
    nb = torch.as_tensor(idx[0].astype(np.int64))
    # the fp32 score enters the model's loss; the autograd form takes the float64 distances: they differ by fp32 rounding of d
    d = (xt[:, None, :] - xt[nb]).norm(dim=2)
    loss = ((d.mean(dim=1) - float(thr)) * torch.as_tensor(w[0], dtype=torch.float64)).sum() / N
    loss.backward()
    g64 = xt.grad.numpy()
    # loss: every masked score is an fp32 mean of fp32 square roots: (k + 2) roundings of 2^-24 relative, on scores <= 1
    assert abs(out["loss"][0] - loss.item()) <= (k + 2) * 2.0 ** -24 * float(w.sum()) / N
    # gradient: the model's G is a float64 sum of float64 unit vectors whose d is the fp32 distance (relative error <= 2.5 * 2^-24:
    # three roundings in val halved by the root, plus the root's own); every edge adds at most 1 / (n k) per component
    deg = M.in_degree(idx, w)[0] + np.where(w[0], k, 0)
    bound = 2.5 * 2.0 ** -24 * deg[:, None] / (N * k) + 2.0 ** -24 * np.abs(g64)        # + the one rounding to fp32
    assert (np.abs(out["grad"][0].astype(np.float64) - g64) <= bound).all()


@pytest.mark.parametrize("k", [1, 2, 7])
def test_model_edges_and_order_against_float64_autograd(k):
    """With the one fp32 ingredient taken out (exact=True: d the float64 norm) the model's sum over gather and scatter edges is
    the autograd gradient to float64 rounding: every edge adds a component <= 1, so 2^-50 per edge covers the order of the sums.
    And the model's fp32 gradient is its float64 gradient rounded once; its loss the plain float64 sum of the hinge."""
    import torch
    x = np.stack([SM.cloud_of_kind("random", N, 50 + k)])
    idx = M.brute_idx(x, k)
    thr = _median_thr(x, idx, k)
    out = SM.surface_loss(x, idx, k, thr)
    w = out["mask"]
    xt = torch.tensor(x[0].astype(np.float64), requires_grad=True)
    nb = torch.as_tensor(idx[0].astype(np.int64))
    d = (xt[:, None, :] - xt[nb]).norm(dim=2)
    (((d.mean(dim=1) - float(thr)) * torch.as_tensor(w[0], dtype=torch.float64)).sum() / N).backward()
    g64 = xt.grad.numpy()
    deg = M.in_degree(idx, w)[0] + np.where(w[0], k, 0)
    exact = SM.gradient(x, idx, w, exact=True)[1][0]
    assert (np.abs(exact - g64) <= 2.0 ** -50 * deg[:, None] / (N * k)).all()
    assert np.array_equal(out["grad"], out["grad64"].astype(np.float32))
    hinge = np.where(w[0], out["score"][0] - np.float64(thr), 0.0)
    assert abs(out["loss"][0] - hinge.sum() / N) <= 2.0 ** -50


@pytest.mark.parametrize("kind", ["random", "pairs", "lattice"])
@pytest.mark.parametrize("k", [1, 2, 7])
def test_mask_is_numpys_float32_mean(kind, k):
    x = np.stack([SM.cloud_of_kind(kind, N, 60)])
    idx = M.brute_idx(x, k)
    out = SM.surface_loss(x, idx, k, 0.04)
    for thr in (0.04, _median_thr(x, idx, k), out["score32"][0, 17], 0.0, 1e6):
        got = SM.surface_loss(x, idx, k, thr)
        want = np.where(np.mean(out["dist"][0][:, :k], -1) > np.float32(thr))[0]
        assert np.array_equal(np.flatnonzero(got["mask"][0]), want)
        assert got["stats"][0, 3] == len(want) and got["stats"][0, 0] == np.float64(np.float32(thr))
    assert not SM.surface_loss(x, idx, k, out["score32"][0, 17])["mask"][0, 17]         # the strict >
    none = SM.surface_loss(x, idx, k, 1e6)
    assert none["loss"].tobytes() == np.zeros(1).tobytes() and none["grad"].tobytes() == np.zeros((1, N, 3), np.float32).tobytes()
    if k == 7:
        assert 116 <= int(SM.surface_loss(x, idx, k, _median_thr(x, idx, k))["mask"].sum()) <= 128


def test_zero_distances_add_nothing():
    x = np.stack([SM.cloud_of_kind("pairs", N, 61)])
    idx = M.brute_idx(x, 2)
    out = SM.surface_loss(x, idx, 2, 0.0)
    assert (out["dist"][0] == 0).any() and np.isfinite(out["grad"]).all()
    eq = np.stack([SM.cloud_of_kind("equal", N, 0)])
    out = SM.surface_loss(eq, M.brute_idx(eq, 7), 7, 0.0)
    assert not out["mask"].any() and out["grad"].tobytes() == np.zeros((1, N, 3), np.float32).tobytes()


def test_dodecahedron_hub():
    x = np.stack([SM.cloud_of_kind("dodecahedron", N, 62)])
    idx = M.brute_idx(x, 7)
    out = SM.surface_loss(x, idx, 7, 0.5)
    assert int(out["mask"].sum()) == 24 and out["mask"][0, :24].all()
    for v in range(4, 24):
        assert set(range(4)) <= set(idx[0, v].tolist())
    deg = M.in_degree(idx, out["mask"])[0]
    assert (deg[:4] > SM.SEGMENT_CAP).all() and 20 <= deg[:4].min() and deg[:4].max() <= 24
    # every vertex is pulled towards its neighbours (a non-zero gradient); the four centre points, equal and surrounded by the
    # 20 vertices, share one gradient
    assert np.isfinite(out["grad"]).all() and (np.abs(out["grad"][0, 4:24]).max(axis=1) > 0).all()
    assert not out["grad"][0, 24:].any()


# ---- the host-side carriers ---------------------------------------------------------------------------------------------------
def _conf(**kw):
    from geometric_adv_amd.adv_ae import Configuration
    args = dict(batch_size=4, n_points=N, weights=None)
    args.update(kw)
    return Configuration(**args)


def test_configuration_carries_the_rule():
    c = _conf()
    assert (c.knn_rule, c.knn_thresh) == ("sor", 0.04)
    c = _conf(knn_weight=2.0, knn_rule="surface", knn_k=2, knn_thresh=0.1)
    assert (c.knn_rule, c.knn_thresh, c.knn_k) == ("surface", 0.1, 2)
    assert _conf(knn_weight=2.0, knn_rule="surface", knn_k=7, knn_alpha=float("nan")).knn_k == 7      # knn_alpha is not read
    assert _conf(knn_weight=0.0, knn_rule="nonsense", knn_thresh=float("nan")).knn_weight == 0.0      # term off: neither is read


@pytest.mark.parametrize("bad", [dict(knn_rule="hull"), dict(knn_rule=1), dict(knn_rule="surface", knn_k=8),
                                 dict(knn_rule="surface", knn_thresh=-1.0), dict(knn_rule="surface", knn_thresh=float("nan")),
                                 dict(knn_rule="surface", knn_thresh=float("inf"))])
def test_configuration_refuses(bad):
    kw = dict(knn_weight=3.0, knn_k=2)
    kw.update(bad)
    with pytest.raises(ValueError):
        _conf(**kw)


def test_run_attack_has_the_two_flags():
    from geometric_adv_amd import run_attack
    p = run_attack.build_parser()
    d = p.parse_args([])
    assert (d.knn_rule, d.knn_thresh) == ("sor", 0.04)
    f = p.parse_args(["--knn_weight", "2", "--knn_rule", "surface", "--knn_k", "2", "--knn_thresh", "0.05"])
    assert (f.knn_rule, f.knn_thresh, f.knn_k) == ("surface", 0.05, 2)
    with pytest.raises(SystemExit):
        p.parse_args(["--knn_rule", "hull"])


def test_the_mirror_and_the_constant():
    from geometric_adv_amd import _abi, ops
    fields = _abi.AttackConfig._fields_
    names = [f for f, _ in fields]
    assert ("knn_rule", ctypes.c_int) in fields and ("knn_thresh", ctypes.c_float) in fields
    assert names.index("knn_rule") + 1 == names.index("knn_thresh") < names.index("loss_in_scan") == len(names) - 1
    c = _abi.AttackConfig()
    assert (c.knn_rule, c.knn_thresh) == (0, 0.0)
    assert _abi.GEOADV_KNN_LOSS_SURFACE == 0x100 and ops.KNN_LOSS_RULES == {"sor": 0, "surface": 0x100}
