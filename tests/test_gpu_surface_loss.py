"""GPU: the SURFACE rule of geoadv_knn_outlier_loss (GEOADV_KNN_LOSS_SURFACE OR-ed into `kernel`; csrc/knn_loss.hip) straight
through the C interface on guarded, pre-filled buffers, bit for bit against the numpy model of the rule
(tests/_surface_loss_model.py) fed the device's own neighbour indices, which tests/test_gpu_grouping.py pins; the mask against
ops.outlier_filter on ops.knn_dists (the defense the rule is aimed at); repeatability, batch independence, the three search
kernels, non-finite points, the refusals, and the call without the flag.

Shapes: b = 3 clouds of 256 (a quarter of the workgroup), 300 (a partial wave) and 1025 (a second point per thread) points;
k = 1 (no division), 2 (the defense's), 7 (the limit).  A call takes one threshold for its batch; the thresholds are computed
per cloud from the model's scores -- for every cloud c of a batch its median score (about half of ITS points masked) and exactly
one of ITS points' fp32 score (the strict > leaves that point unmasked), each run on the whole batch and held non-vacuous on
cloud c -- and per batch 0.0 and 1e6 (nothing masked)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_loss_model as M  # noqa: E402
import _surface_loss_model as SM  # noqa: E402
from _guarded import DEV, FILL, Buf  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = 1
SURFACE = 0x100
OUTPUTS = ("loss", "grad", "score", "mask", "idx", "stats")
KERNELS = {"auto": 0, "all_points": 1, "grid": 2, "grid_shells": 3}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _lib():
    from geometric_adv_amd import _lib
    return _lib


def _buffers(x, k):
    b, n, _ = x.shape
    need = int(_lib().lib().geoadv_knn_outlier_loss_workspace_bytes(b, n, min(max(k, 1), 15)))
    return dict(xyz=Buf(x.shape, np.float32, x), loss=Buf((b,), np.float64), grad=Buf((b, n, 3), np.float32),
                score=Buf((b, n), np.float64), mask=Buf((b, n), np.uint8), idx=Buf((b, n, k), np.int32),
                stats=Buf((b, 4), np.float64), ws=Buf((need,), np.uint8))


def _call(bufs, b, n, k, alpha, kernel):
    lib = _lib()
    return lib.lib().geoadv_knn_outlier_loss(kernel, b, n, k, float(alpha), bufs["xyz"].ptr, bufs["loss"].ptr, bufs["grad"].ptr,
                                             bufs["score"].ptr, bufs["mask"].ptr, bufs["idx"].ptr, bufs["stats"].ptr, bufs["ws"].ptr,
                                             bufs["ws"].nbytes, lib.stream_handle())


def _run(x, k, thr, kernel=0, flag=SURFACE):
    """One call on fresh guarded buffers -> dict of the outputs."""
    import torch
    b, n, _ = x.shape
    bufs = _buffers(x, k)
    _lib().check(_call(bufs, b, n, k, thr, kernel | flag), "knn_outlier_loss")
    torch.cuda.synchronize()
    bufs["ws"].get()                                          # the workspace's guards
    out = {name: bufs[name].get() for name in ("xyz",) + OUTPUTS}
    assert _same_bits(out.pop("xyz"), x), "the input changed"
    return out


def _check(out, x, k, thr, what, clouds=None):
    """The outputs against the model fed the device's neighbours -> the model's dict.  Loss, score, mask, stats and grad as bytes
    (a NaN score is a NaN on both sides: its sign and payload are no part of the rule)."""
    n = x.shape[1]
    assert ((out["idx"] >= 0) & (out["idx"] < n)).all(), "a neighbour outside the cloud (%s)" % what
    want = SM.surface_loss(x, out["idx"], k, thr)
    sel = slice(None) if clouds is None else clouds
    nan = np.isnan(want["score"])
    assert np.array_equal(np.isnan(out["score"]), nan), "the NaN scores differ from the model's (%s)" % what
    assert _same_bits(np.where(nan, 0.0, out["score"])[sel], np.where(nan, 0.0, want["score"])[sel]), "score differs from the model (%s)" % what
    assert _same_bits(out["mask"][sel], want["mask"].astype(np.uint8)[sel]), "mask differs from the model (%s)" % what
    for name in ("stats", "loss", "grad"):
        assert _same_bits(out[name][sel], want[name][sel]), "%s differs from the model (%s)" % (name, what)
    return want


@functools.lru_cache(maxsize=None)
def _clouds(kind, n):
    """Three clouds of a kind (shared by the tests, never written to)."""
    x = np.stack([SM.cloud_of_kind("random" if kind == "nonfinite" else kind, n, 2000 * n + c) for c in range(3)])
    if kind == "nonfinite":                                  # cloud 1 only: _clouds("random", n) is the same batch without them
        x[1, n - 3, 1] = np.nan
        x[1, n - 7, 0] = np.inf
    x.setflags(write=False)
    return x


def _thresholds(x, idx, k, clouds=(0,)):
    """(name, threshold, the cloud it was computed from, point of that cloud that must stay unmasked or None): the median and
    one point's own score from the model's scores of every cloud in `clouds`, then 0.0 and 1e6"""
    out = []
    for c in clouds:
        s = SM.scores(SM.dists(x[c:c + 1], idx[c:c + 1]), k)[0]
        p = int(np.argsort(s, kind="stable")[len(s) // 3])    # a point a third of the way up: points above it exist
        out += [("median", np.float32(np.median(s)), c, None), ("a point's score", s[p], c, p)]
    return out + [("zero", np.float32(0.0), 0, None), ("1e6", np.float32(1e6), 0, None)]


NS = [256, 300, 1025]
KS = [1, 2, 7]


@pytest.mark.parametrize("kind", ["random", "pairs", "lattice", "equal", "dodecahedron"])
@pytest.mark.parametrize("n", NS)
def test_outputs_are_the_model_bit_for_bit(n, kind):
    x = _clouds(kind, n)
    for k in ([7] if kind == "dodecahedron" else KS):
        idx = _run(x, k, 0.04)["idx"]
        cases = _thresholds(x, idx, k, clouds=(0, 1, 2)) + ([("hub", np.float32(0.5), 0, None)] if kind == "dodecahedron" else [])
        for name, thr, c, unmasked in cases:
            what = "kind=%s n=%d k=%d thr=%s of cloud %d (%.9g)" % (kind, n, k, name, c, thr)
            out = _run(x, k, thr)
            assert _same_bits(out["idx"], idx)
            want = _check(out, x, k, thr, what)
            count = want["mask"].sum(axis=1)
            # the conditions that keep a case from passing vacuously, on the model
            if kind == "equal" or name == "1e6":
                assert not want["mask"].any() and not out["loss"].view(np.uint64).any() and not out["grad"].view(np.uint32).any(), what
            elif name == "median":
                assert 0 < count[c] <= n // 2, "%s masked of cloud %d (%s)" % (count[c], c, what)     # (a lattice's scores tie)
                if n == 256 and k == 7 and c == 0 and kind in ("random", "pairs", "lattice"):
                    assert 116 <= count[0] <= 128, "%s masked (%s)" % (count[0], what)
            elif name == "a point's score":
                assert not want["mask"][c, unmasked] and want["score32"][c, unmasked] == thr and count[c] > 0, what
            elif name == "zero":
                assert (count == (want["score32"] > 0).sum(axis=1)).all() and count.min() > 0, what
            elif name == "hub":
                assert (count == 24).all(), what
                deg = M.in_degree(out["idx"], want["mask"])
                assert (deg[:, :4] > SM.SEGMENT_CAP).all(), "in-degrees %s (%s)" % (deg[:, :4], what)
            if kind == "pairs" and name == "zero":
                assert (want["dist"] == 0).any() and np.isfinite(out["grad"]).all(), what


@pytest.mark.parametrize("n", NS)
def test_mask_is_outlier_filters_outlier_set(n):
    import torch
    from geometric_adv_amd import ops
    for kind in ("random", "pairs", "lattice", "dodecahedron"):
        x = _clouds(kind, n)
        dev = torch.from_numpy(np.array(x)).to(DEV)
        for k in ([7] if kind == "dodecahedron" else KS):
            dists = ops.knn_dists(dev, k)
            idx = _run(x, k, 0.04)["idx"]
            assert _same_bits(SM.dists(x, idx), dists.cpu().numpy()), "d is not what knn_dists writes (%s k=%d)" % (kind, k)
            for name, thr, _, _ in _thresholds(x, idx, k)[:3]:
                out = _run(x, k, thr)
                _, o_idx, o_num, _ = ops.outlier_filter(dev, dists, float(thr), top_k=k)
                o_idx, o_num = o_idx.cpu().numpy(), o_num.cpu().numpy()
                assert out["mask"].any()
                for c in range(3):
                    assert np.array_equal(np.flatnonzero(out["mask"][c]), o_idx[c, :o_num[c]]), (kind, k, name, c)


@pytest.mark.parametrize("kind", ["random", "dodecahedron"])
def test_a_cloud_alone_has_the_bits_it_has_in_a_batch_and_twice_the_same(kind):
    x = _clouds(kind, 1025)
    thr = 0.5 if kind == "dodecahedron" else _thresholds(x, _run(x, 7, 0.04)["idx"], 7)[0][1]
    batch = _run(x, 7, thr)
    again = _run(x, 7, thr)
    assert batch["mask"].any(axis=1).all()
    for name in OUTPUTS:
        assert _same_bits(batch[name], again[name]), "%s differs between two calls" % name
    for c in range(3):
        alone = _run(x[c:c + 1], 7, thr)
        for name in OUTPUTS:
            assert _same_bits(alone[name], batch[name][c:c + 1]), "%s of cloud %d alone" % (name, c)


@pytest.mark.parametrize("n", [300, 1025])
def test_the_three_search_kernels_give_the_same_bytes(n):
    for kind in ("random", "lattice", "pairs"):
        x = _clouds(kind, n)
        for k in (2, 7):
            thr = _thresholds(x, _run(x, k, 0.04)["idx"], k)[0][1]
            first = _run(x, k, thr, kernel=KERNELS["auto"])
            _check(first, x, k, thr, "kind=%s k=%d" % (kind, k))
            for kernel in ("all_points", "grid", "grid_shells"):
                out = _run(x, k, thr, kernel=KERNELS[kernel])
                for name in OUTPUTS:
                    assert _same_bits(out[name], first[name]), "%s with the %s kernel (%s k=%d)" % (name, kernel, kind, k)


@pytest.mark.parametrize("n", [256, 1025])
def test_nonfinite_points(n):
    """Cloud 1 holds a NaN point and an inf point: mask, score and loss follow the model (NaN score: 0; +inf score: 1, and the hinge
    is then +inf); the other clouds have the bytes they have without them."""
    x = _clouds("nonfinite", n)
    clean_x = _clouds("random", n)
    for k in (2, 7):
        thr = _thresholds(clean_x, _run(clean_x, k, 0.04)["idx"], k)[0][1]
        out = _run(x, k, thr)
        want = SM.surface_loss(x, np.clip(out["idx"], 0, n - 1), k, thr)
        nan = np.isnan(want["score"])
        assert nan[1, n - 3] and np.array_equal(np.isnan(out["score"]), nan)
        assert _same_bits(np.where(nan, 0.0, out["score"]), np.where(nan, 0.0, want["score"]))
        assert _same_bits(out["mask"], want["mask"].astype(np.uint8)) and not out["mask"][1, n - 3]
        assert np.isnan(want["loss"][1]) == np.isnan(out["loss"][1])
        if not np.isnan(want["loss"][1]):
            assert _same_bits(out["loss"], want["loss"])
        assert _same_bits(out["stats"], want["stats"]) and out["stats"][1, 2] < n
        inf = np.isposinf(want["score"][1])
        assert (out["mask"][1][inf] == 1).all()
        clean = _run(clean_x, k, thr)
        for name in OUTPUTS:
            assert _same_bits(out[name][[0, 2]], clean[name][[0, 2]]), "%s of clouds 0, 2 (k=%d)" % (name, k)


def test_refusals_leave_the_outputs_untouched():
    import torch
    x = _clouds("random", 256)[:2]
    b, n = 2, 256

    def refused(what, k=2, alpha=0.04, kernel=SURFACE):
        bufs = _buffers(x, k)
        st = _call(bufs, b, n, k, alpha, kernel)
        torch.cuda.synchronize()
        assert st == EINVAL, "%s: status %d" % (what, st)
        assert _lib().lib().geoadv_last_error()
        for name in OUTPUTS + ("ws",):
            assert (bufs[name].get().reshape(-1).view(np.uint8) == FILL).all(), "%s: %s was written" % (what, name)
        assert _same_bits(bufs["xyz"].get(), x)

    refused("k = 8 under the flag", k=8)
    refused("alpha = -1", alpha=-1.0)
    refused("alpha nan", alpha=float("nan"))
    refused("alpha inf", alpha=float("inf"))
    refused("alpha above FLT_MAX", alpha=1e39)
    refused("flag bits 0x200", kernel=0x200)
    refused("flag bits 0x104", kernel=0x104)
    refused("flag bits 0x300", kernel=0x300)
    refused("k = 0 under the flag", k=0)
    # what is refused under the flag only is taken without it, and the same call with nothing wrong is taken
    _lib().check(_call(_buffers(x, 8), b, n, 8, 1.05, 0), "k = 8 without the flag")
    torch.cuda.synchronize()
    out = _run(x, 2, 0.04)
    _check(out, x, 2, 0.04, "after the refusals")


def test_without_the_flag_the_call_is_the_sor_rule():
    """ops.knn_outlier_loss(x, 5, 1.05) -- no rule, no thresh -- has the bytes of the SOR rule's model (what the call computed
    before it knew a flag; tests/test_gpu_knn_loss.py, unchanged, holds the rest), and rule='sor' with any thresh the same."""
    import torch
    from geometric_adv_amd import ops
    x = _clouds("lattice", 1025)
    dev = torch.from_numpy(np.array(x)).to(DEV)
    got = ops.knn_outlier_loss(dev, 5, 1.05, return_parts=True)
    want = M.knn_outlier_loss(x, got[4].cpu().numpy(), 5, 1.05)
    for g, name in zip(got, ("loss", "grad", "score", "mask", "idx", "stats")):
        if name != "idx":
            assert _same_bits(g.cpu().numpy(), want[name]), name
    same = ops.knn_outlier_loss(dev, 5, 1.05, return_parts=True, rule="sor", thresh=123.0)
    raw = _run(x, 5, 1.05, flag=0)
    for a, b, name in zip(got, same, OUTPUTS):
        assert torch.equal(a, b), name
        assert _same_bits(a.cpu().numpy().astype(raw[name].dtype), raw[name]), name


def test_ops_knn_outlier_loss_surface():
    import torch
    from geometric_adv_amd import ops
    x = _clouds("random", 300)
    dev = torch.from_numpy(np.array(x)).to(DEV)
    loss, grad, score, mask, idx, stats = ops.knn_outlier_loss(dev, k=2, rule="surface", thresh=0.04, return_parts=True)
    want = SM.surface_loss(x, idx.cpu().numpy(), 2, 0.04)
    assert want["mask"].any()
    for got, name in ((loss, "loss"), (grad, "grad"), (score, "score"), (mask, "mask"), (stats, "stats")):
        assert _same_bits(got.cpu().numpy(), want[name]), name
    ignored = ops.knn_outlier_loss(dev, k=2, alpha=float("nan"), rule="surface", thresh=0.04)       # alpha is not looked at
    assert torch.equal(ignored[0], loss) and torch.equal(ignored[1], grad)
    only_loss, none = ops.knn_outlier_loss(dev, k=2, rule="surface", want_grad=False)
    assert none is None and torch.equal(only_loss, loss)
    for bad in (dict(k=8), dict(thresh=-1.0), dict(thresh=float("nan")), dict(thresh=float("inf")), dict(rule="hull")):
        kw = dict(k=2, rule="surface")
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.knn_outlier_loss(dev, **kw)
