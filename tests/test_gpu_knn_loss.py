"""GPU: geoadv_knn_outlier_loss straight through the C interface, every buffer inside a guarded allocation and every output
pre-filled with a pattern, bit for bit against the numpy model of the rule (tests/_knn_loss_model.py) fed the device's own
neighbour indices; the search against ops.knn_point, the mask against ops.sor_filter; NULL outputs, batch independence,
repeatability, non-finite points and the refusals."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_loss_model as M  # noqa: E402
from _guarded import DEV, FILL, Buf  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = 1
OUTPUTS = ("loss", "grad", "score", "mask", "idx", "stats")
OPTIONAL = ("grad", "score", "mask", "idx", "stats")
KERNELS = {"auto": 0, "all_points": 1, "grid": 2, "grid_shells": 3}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _lib():
    from geometric_adv_amd import _lib
    return _lib


def _buffers(x, k, ws_bytes=None):
    b, n, _ = x.shape
    need = int(_lib().lib().geoadv_knn_outlier_loss_workspace_bytes(b, n, k))
    return dict(xyz=Buf(x.shape, np.float32, x), loss=Buf((b,), np.float64), grad=Buf((b, n, 3), np.float32),
                score=Buf((b, n), np.float64), mask=Buf((b, n), np.uint8), idx=Buf((b, n, max(k, 0)), np.int32),
                stats=Buf((b, 4), np.float64), ws=Buf((need if ws_bytes is None else ws_bytes,), np.uint8))


def _call(bufs, b, n, k, alpha, kernel=0, arg=None):
    arg = {name: buf.ptr for name, buf in bufs.items()} if arg is None else arg
    lib = _lib()
    return lib.lib().geoadv_knn_outlier_loss(kernel, b, n, k, float(alpha), arg["xyz"], arg["loss"], arg["grad"], arg["score"], arg["mask"],
                                             arg["idx"], arg["stats"], arg["ws"], bufs["ws"].nbytes, lib.stream_handle())


def _run(x, k, alpha, kernel=0, null=()):
    """One call on fresh guarded buffers -> dict of the outputs (None for a NULL one)."""
    import torch
    b, n, _ = x.shape
    bufs = _buffers(x, k)
    arg = {name: (None if name in null else buf.ptr) for name, buf in bufs.items()}
    _lib().check(_call(bufs, b, n, k, alpha, kernel, arg), "knn_outlier_loss")
    torch.cuda.synchronize()
    bufs["ws"].get()                                          # the workspace's guards
    out = {name: bufs[name].get() for name in ("xyz",) + OUTPUTS}
    assert _same_bits(out.pop("xyz"), x), "the input changed"
    for name in OUTPUTS:
        if arg[name] is None:
            assert (out[name].reshape(-1).view(np.uint8) == FILL).all(), "%s was passed as NULL and written" % name
            out[name] = None
    return out


def _check(out, x, k, alpha, what):
    """The outputs against the model fed the device's neighbours -> the model's dict."""
    n = x.shape[1]
    assert ((out["idx"] >= 0) & (out["idx"] < n)).all(), "a neighbour outside the cloud (%s)" % what
    want = M.knn_outlier_loss(x, out["idx"], k, alpha)
    # (a NaN score is a NaN on both sides; its sign and payload are the adder's, x86's or the GPU's, and no part of the rule)
    nan = np.isnan(want["score"])
    assert np.array_equal(np.isnan(out["score"]), nan), "the NaN scores differ from the model's (%s)" % what
    assert _same_bits(np.where(nan, 0.0, out["score"]), np.where(nan, 0.0, want["score"])), "score differs from the model (%s)" % what
    for name in ("stats", "loss", "grad"):
        assert _same_bits(out[name], want[name]), "%s differs from the model (%s)" % (name, what)
    assert _same_bits(out["mask"], want["mask"].astype(np.uint8)), "mask differs from the model (%s)" % what
    return want


@functools.lru_cache(maxsize=None)
def _clouds(kind, n):
    """Three clouds of a kind (shared by the tests, never written to)."""
    x = np.stack([M.cloud_of_kind("random" if kind == "nonfinite" else kind, n, 1000 * n + c) for c in range(3)])
    if kind == "nonfinite":                                  # cloud 0 only: _clouds("random", n) is the same batch without them.
        # Past index k + 1 = 16: knn_point keeps the reference's SelectionSort, in which a NaN distance among the first k + 1
        # columns is never swapped out -- at n = 33 every row would list the NaN point and no score would be finite
        x[0, n - 3, 1] = np.nan
        x[0, n - 7, 0] = np.inf
    x.setflags(write=False)
    return x


KINDS = ["random", "lattice", "hub", "equal", "pairs", "nonfinite"]
NS = [33, 1025, 2048]                                        # a partial wave, the second row of the T-strided sum, the working size
KS = [1, 5, 15]
ALPHAS = [0.0, 1.05, 1e6]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_outputs_are_the_model_bit_for_bit(n, kind):
    for b in (1, 3):
        x = _clouds(kind, n)[:b]
        for k in KS:
            for alpha in ALPHAS:
                what = "kind=%s n=%d b=%d k=%d alpha=%g" % (kind, n, b, k, alpha)
                out = _run(x, k, alpha)
                want = _check(out, x, k, alpha, what)
                # the conditions that keep a case from passing vacuously, on the model
                if kind == "equal":
                    assert not want["mask"].any() and (want["stats"][:, 1] == 0).all() and not out["grad"].view(np.uint32).any()
                elif alpha != 1e6:
                    assert want["mask"].any(axis=1).all(), "an empty mask (%s)" % what
                else:
                    assert not want["mask"].any() and not out["loss"].view(np.uint64).any() and not out["grad"].view(np.uint32).any()
                if alpha != 1e6 and kind in ("lattice", "hub"):
                    deg = M.in_degree(out["idx"], want["mask"]).max(axis=1)
                    assert (deg >= (3 if kind == "lattice" else 12)).all(), "in-degrees %s (%s)" % (deg, what)
                if kind == "nonfinite":
                    bad = [n - 3, n - 7]
                    assert not np.isfinite(want["score"][0, bad]).any() and not want["mask"][0, bad].any()
                    assert not out["grad"][0, bad].view(np.uint32).any(), "a non-finite point with a gradient (%s)" % what
                    assert want["stats"][0, 2] < n
                    if b == 3:                               # the other clouds are what they are without cloud 0's bad points
                        clean = _run(_clouds("random", n), k, alpha)
                        for name in OUTPUTS:
                            assert _same_bits(out[name][1:], clean[name][1:]), "%s of clouds 1, 2 (%s)" % (name, what)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("n", [33, 1025])
def test_search_is_knn_points(n, kernel):
    import torch
    from geometric_adv_amd import ops
    for kind in ("random", "lattice", "pairs"):
        x = _clouds(kind, n)
        for k in (1, 5, 15):
            out = _run(x, k, 1.05, kernel=KERNELS[kernel])
            dev = torch.from_numpy(np.array(x)).to(DEV)
            val, idx = ops.knn_point(k + 1, dev, dev, kernel=kernel)
            assert _same_bits(out["idx"], np.ascontiguousarray(idx.cpu().numpy()[:, :, 1:])), (kind, k)
            assert _same_bits(M.knn_vals(x, out["idx"]), np.ascontiguousarray(val.cpu().numpy()[:, :, 1:])), (kind, k)
            _check(out, x, k, 1.05, "kernel=%s kind=%s k=%d" % (kernel, kind, k))


@pytest.mark.parametrize("n", [33, 2048])
def test_mask_is_sor_filters_outlier_set(n):
    import torch
    from geometric_adv_amd import ops
    for kind in ("random", "lattice", "hub", "pairs"):
        x = _clouds(kind, n)
        for k, alpha in ((1, 0.0), (5, 1.05), (15, 1.05)):
            out = _run(x, k, alpha)
            val = torch.from_numpy(M.knn_vals(x, out["idx"])).to(DEV)
            _, o_idx, o_num, _ = ops.sor_filter(torch.from_numpy(np.array(x)).to(DEV), val, k=k, alpha=alpha)
            o_idx, o_num = o_idx.cpu().numpy(), o_num.cpu().numpy()
            assert out["mask"].any()
            for c in range(3):
                assert np.array_equal(np.flatnonzero(out["mask"][c]), o_idx[c, :o_num[c]]), (kind, k, alpha, c)


@pytest.mark.parametrize("n", [65, 1025])
def test_null_outputs_leave_the_others_unchanged(n):
    x = _clouds("pairs", n)
    full = _run(x, 5, 1.05)
    _check(full, x, 5, 1.05, "n=%d" % n)
    for null in [(name,) for name in OPTIONAL] + [OPTIONAL]:
        out = _run(x, 5, 1.05, null=null)
        assert [name for name in OUTPUTS if out[name] is None] == [name for name in OUTPUTS if name in null]
        for name in OUTPUTS:
            assert out[name] is None or _same_bits(out[name], full[name]), "%s with %s NULL" % (name, null)


@pytest.mark.parametrize("kind", ["random", "hub"])
def test_a_cloud_alone_has_the_bits_it_has_in_a_batch_and_twice_the_same(kind):
    x = _clouds(kind, 1025)
    batch = _run(x, 5, 1.05)
    again = _run(x, 5, 1.05)
    for name in OUTPUTS:
        assert _same_bits(batch[name], again[name]), "%s differs between two calls" % name
    for c in range(3):
        alone = _run(x[c:c + 1], 5, 1.05)
        for name in OUTPUTS:
            assert _same_bits(alone[name], batch[name][c:c + 1]), "%s of cloud %d alone" % (name, c)


def test_ops_knn_outlier_loss():
    import torch
    from geometric_adv_amd import ops
    x = _clouds("lattice", 1025)
    dev = torch.from_numpy(np.array(x)).to(DEV)
    loss, grad, score, mask, idx, stats = ops.knn_outlier_loss(dev, k=5, alpha=1.05, return_parts=True)
    assert loss.dtype == torch.float64 and grad.dtype == torch.float32 and mask.dtype == torch.bool and idx.dtype == torch.int32
    want = M.knn_outlier_loss(x, idx.cpu().numpy(), 5, 1.05)
    for got, name in ((loss, "loss"), (grad, "grad"), (score, "score"), (mask, "mask"), (stats, "stats")):
        assert _same_bits(got.cpu().numpy(), want[name]), name
    only_loss, none = ops.knn_outlier_loss(dev, want_grad=False)
    assert none is None and torch.equal(only_loss, loss)
    two = ops.knn_outlier_loss(dev, kernel="grid_shells")
    assert len(two) == 2 and torch.equal(two[0], loss) and torch.equal(two[1], grad)
    for bad in (dict(k=0), dict(k=16), dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(kernel="fast")):
        with pytest.raises(ValueError):
            ops.knn_outlier_loss(dev, **bad)
    with pytest.raises(ValueError):
        ops.knn_outlier_loss(dev[:, :6], k=5)
    with pytest.raises(ValueError):
        ops.knn_outlier_loss(dev.cpu())


def test_refusals_leave_the_outputs_untouched():
    import torch
    b, n, k = 2, 40, 5
    x = _clouds("random", 33)[:b]
    x = np.concatenate([x, x[:, :7]], axis=1)
    need = int(_lib().lib().geoadv_knn_outlier_loss_workspace_bytes(b, n, k))
    assert need > 256 and int(_lib().lib().geoadv_knn_outlier_loss_workspace_bytes(b, n, 16)) == 256

    def refused(what, b=b, n=n, k=k, alpha=1.05, kernel=0, ws_bytes=None, **ptrs):
        bufs = _buffers(x, 5, ws_bytes)
        arg = {name: buf.ptr for name, buf in bufs.items()}
        arg.update(ptrs)
        if ptrs.get("grad") == "overlap":
            arg["grad"] = C.c_void_p(bufs["xyz"].ptr.value + 4)
        st = _call(bufs, b, n, k, alpha, kernel, arg)
        torch.cuda.synchronize()
        assert st == EINVAL, "%s: status %d" % (what, st)
        assert _lib().lib().geoadv_last_error()
        for name in OUTPUTS + ("ws",):
            assert (bufs[name].get().reshape(-1).view(np.uint8) == FILL).all(), "%s: %s was written" % (what, name)
        assert _same_bits(bufs["xyz"].get(), x)

    refused("b < 0", b=-1)
    refused("k < 1", k=0)
    refused("k > 15", k=16)
    refused("n < k + 2", n=6)
    refused("n > 32767", n=32768)
    refused("alpha < 0", alpha=-0.5)
    refused("alpha nan", alpha=float("nan"))
    refused("alpha inf", alpha=float("inf"))
    refused("xyz NULL", xyz=None)
    refused("loss NULL", loss=None)
    refused("workspace NULL", ws=None)
    refused("workspace too small", ws_bytes=need - 1)
    refused("unknown kernel", kernel=4)
    refused("unknown kernel", kernel=-1)
    refused("grad overlapping xyz", grad="overlap")
    # b == 0 is a no-op, whatever the pointers
    bufs = _buffers(x, 5)
    assert _call(bufs, 0, n, k, 1.05, 0, {name: None for name in bufs}) == 0
    # and the same call with nothing wrong is taken
    out = _run(x, k, 1.05)
    _check(out, x, k, 1.05, "after the refusals")
