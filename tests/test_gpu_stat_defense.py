"""GPU: geoadv_sor_filter and geoadv_random_drop straight through the C interface, every buffer inside a guarded allocation and
every output pre-filled with a pattern, bit for bit against the numpy models of the two rules (tests/_stat_defense_model.py);
and ops.sor_filter with its own kNN distances on a cloud with planted far-off points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stat_defense_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 256                  # guard bytes before and after every buffer
FILL = 0xA5                # guards and unwritten outputs
T = M.T


class Buf:
    """A device allocation of PAD + nbytes + PAD bytes filled with FILL; the payload optionally holds `host`."""

    def __init__(self, shape, dtype, host=None):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.t = torch.full((self.nbytes + 2 * PAD,), FILL, dtype=torch.uint8, device=DEV)
        if host is not None:
            host = np.ascontiguousarray(host, dtype=self.dtype)
            assert host.shape == self.shape
            self.t[PAD:PAD + self.nbytes] = torch.from_numpy(host.reshape(-1).view(np.uint8)).to(DEV)
        self.ptr = C.c_void_p(self.t.data_ptr() + PAD)

    def get(self):
        """-> the payload; asserts both guards first."""
        raw = self.t.cpu().numpy()
        assert (raw[:PAD] == FILL).all() and (raw[PAD + self.nbytes:] == FILL).all(), "a guard changed"
        return raw[PAD:PAD + self.nbytes].view(self.dtype).reshape(self.shape)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _lib():
    from geometric_adv_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------------------
# SOR
# ---------------------------------------------------------------------------------------------------------------------------
KINDS = ["random", "equal", "dyadic", "nonfinite_rows", "all_nan_cloud", "one_finite"]
KS = [1, 2, 8, 63]
ALPHAS = [0.0, 1.1, 1e6]


def _knn_of_kind(kind, base, k, seed):
    """knn [b, n, stride] of a score kind, from the shared random rows `base` (left unchanged)."""
    knn = base.copy()
    b, n, _ = knn.shape
    rng = np.random.default_rng(seed)
    if kind == "equal":
        knn[:] = 0.375
    elif kind == "dyadic":                                   # k equal columns: the score is the column's value exactly
        for c in range(b):
            knn[c, :, :] = M.dyadic_scores(n, seed + c).astype(np.float32)[:, None]
    elif kind == "nonfinite_rows":
        hit = rng.random((b, n)) < 0.2
        hit[:, 0] = True
        knn[:, :, 0][hit] = np.nan
        hit = rng.random((b, n)) < 0.2
        hit[:, -1] = True
        knn[:, :, k - 1][hit] = np.inf
        knn[:, n // 2, 0] = -np.inf
    elif kind == "all_nan_cloud":
        knn[0] = np.nan
    elif kind == "one_finite":
        keep = knn[b - 1, n // 3].copy()
        knn[b - 1] = np.nan
        knn[b - 1, n // 3] = keep
    return knn


def _run_sor(pc, knn, k, alpha, null=(), stats=True):
    """One call of geoadv_sor_filter on fresh guarded buffers -> dict of the outputs (None for a NULL one)."""
    lib = _lib()
    b, n, _ = pc.shape
    stride = knn.shape[2]
    bufs = dict(pc=Buf(pc.shape, np.float32, pc), knn=Buf(knn.shape, np.float32, knn),
                outlier_pc=Buf((b, n, 3), np.float32), outlier_idx=Buf((b, n), np.int16), outlier_num=Buf((b,), np.int16),
                inlier_pc=Buf((b, n, 3), np.float32), stats=Buf((b, 3), np.float64))
    arg = {name: (None if name in null or (name == "stats" and not stats) else buf.ptr) for name, buf in bufs.items()}
    import torch
    st = lib.lib().geoadv_sor_filter(b, n, arg["pc"], arg["knn"], stride, k, C.c_double(alpha), arg["outlier_pc"], arg["outlier_idx"],
                                     arg["outlier_num"], arg["inlier_pc"], arg["stats"], lib.stream_handle())
    lib.check(st, "sor_filter")
    torch.cuda.synchronize()
    out = {name: buf.get() for name, buf in bufs.items()}
    assert _same_bits(out["pc"], pc) and _same_bits(out["knn"], knn), "an input changed"
    for name in bufs:
        if arg[name] is None:
            assert (out[name].reshape(-1).view(np.uint8) == FILL).all(), "%s was passed as NULL and written" % name
            out[name] = None
    return out


def _check_sor(out, want, what):
    o_pc, o_idx, o_num, i_pc, stats = want
    for name, w in (("outlier_pc", o_pc), ("outlier_idx", o_idx), ("outlier_num", o_num), ("inlier_pc", i_pc), ("stats", stats)):
        if out[name] is not None:
            assert _same_bits(out[name], w), "%s differs from the model (%s)" % (name, what)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T - 1, T, T + 1, 2048, 5000, 32767])
def test_sor_is_the_model_bit_for_bit(n):
    rng = np.random.default_rng(n)
    bmax = 3
    pc = (rng.random((bmax, n, 3), dtype=np.float32) - 0.5).astype(np.float32)
    base = rng.random((bmax, n, 64), dtype=np.float32)
    repeated = False
    for ki, kind in enumerate(KINDS):
        for kj, k in enumerate(KS):
            alpha = ALPHAS[(ki + kj) % 3]
            b = (1, 3)[(ki + kj) % 2]
            stride = 64 if k == 63 else k                    # k = 63: the last column is unused
            knn = np.ascontiguousarray(_knn_of_kind(kind, base[:b], k, 100 * n + ki)[:, :, :stride])
            if k == 63:
                knn[:, :, 63] = np.nan                       # unused means unread: a NaN there changes nothing
            want = M.sor_filter(pc[:b], knn, k, alpha)
            what = "n=%d kind=%s k=%d alpha=%g b=%d" % (n, kind, k, alpha, b)
            out = _run_sor(pc[:b], knn, k, alpha)
            _check_sor(out, want, what)
            if kind == "all_nan_cloud":
                assert out["outlier_num"][0] == n and not out["inlier_pc"][0].any() and out["stats"][0].tolist() == [0.0, 0.0, 0.0]
            if kind == "one_finite":
                assert out["stats"][b - 1, 2] == 1.0 and out["stats"][b - 1, 1] == 0.0 and out["outlier_num"][b - 1] == n - 1
            if kind == "dyadic" and n >= 3:
                assert (M.sor_scores(knn, k) == out["stats"][:, 0:1]).any(axis=1).all()        # points exactly at mu
            if kind == "nonfinite_rows" and not repeated:    # a repeated call gives equal bits
                again = _run_sor(pc[:b], knn, k, alpha)
                assert all(_same_bits(out[name], again[name]) for name in out)
                repeated = True


@pytest.mark.parametrize("n", [65, T + 1])
def test_sor_with_null_outputs(n):
    rng = np.random.default_rng(7 + n)
    pc = rng.random((3, n, 3), dtype=np.float32)
    knn = _knn_of_kind("nonfinite_rows", rng.random((3, n, 8), dtype=np.float32), 8, 5)
    want = M.sor_filter(pc, knn, 8, 1.1)
    for null, stats in ((("outlier_pc",), True), (("outlier_idx",), True), (("outlier_num",), True),
                        (("outlier_pc", "outlier_idx", "outlier_num"), True), ((), False)):
        out = _run_sor(pc, knn, 8, 1.1, null=null, stats=stats)
        assert [name for name in out if out[name] is None] == [name for name in out if name in null or (name == "stats" and not stats)]
        _check_sor(out, want, "null=%s stats=%s" % (null, stats))


def test_sor_on_more_clouds_than_a_capped_grid_would_hold():
    b, n, k = 70000, 4, 2
    rng = np.random.default_rng(70)
    pc = rng.random((b, n, 3), dtype=np.float32)
    knn = rng.random((b, n, k), dtype=np.float32)
    knn[rng.random((b, n)) < 0.1, 0] = np.nan
    knn[-1] = [[0.5, 0.5], [0.25, 0.25], [4.0, 4.0], [0.25, 0.25]]                  # the last cloud: a known answer
    out = _run_sor(pc, knn, k, 1.1)
    for c0 in range(0, b, 7000):                                                   # (the model in chunks: it holds T partial sums per cloud)
        want = M.sor_filter(pc[c0:c0 + 7000], knn[c0:c0 + 7000], k, 1.1)
        _check_sor({name: (v[c0:c0 + 7000] if name not in ("pc", "knn") else None) for name, v in out.items()}, want, "clouds from %d" % c0)
    assert out["stats"][-1].tolist() == [1.25, 3.375, 4.0] and out["outlier_num"][-1] == 1 and out["outlier_idx"][-1].tolist() == [2, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# sor_filter with its own kNN
# ---------------------------------------------------------------------------------------------------------------------------
def _planted_cloud(seed=0, n_surface=1000, n_far=20):
    """Points on the unit sphere plus n_far points at radius 3 to 4, shuffled -> (cloud [n,3] float32, planted indices)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_surface + n_far, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[n_surface:] *= rng.uniform(3.0, 4.0, size=(n_far, 1))
    perm = rng.permutation(n_surface + n_far)
    cloud = v[perm].astype(np.float32)
    return cloud, np.sort(np.flatnonzero(perm >= n_surface))


def _brute_knn(cloud, k):
    x = cloud.astype(np.float64)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    return np.sort(d, axis=1)[:, 1:k + 1].astype(np.float32)


def test_sor_filter_with_its_own_knn():
    import torch
    from geometric_adv_amd import ops
    cloud, planted = _planted_cloud()
    # on the CPU, with brute-force float64 distances: the rule removes every planted point, by a wide margin
    inl, (mu, var, m) = M.sor_inliers(M.sor_scores(_brute_knn(cloud, 2)[None], 2), 1.1)
    assert not inl[0][planted].any() and m[0] == len(cloud)
    assert M.sor_scores(_brute_knn(cloud, 2)[None], 2)[0][planted].min() > 2 * (mu[0] + 1.1 * np.sqrt(var[0]))
    rng = np.random.default_rng(1)
    pcs = np.stack([cloud, (rng.random(cloud.shape, dtype=np.float32) - 0.5).astype(np.float32)])
    dev = torch.from_numpy(pcs).to(DEV)
    o_pc, o_idx, o_num, i_pc, stats = ops.sor_filter(dev, k=2, alpha=1.1, return_stats=True)
    knn = ops.knn_dists(dev, 2).cpu().numpy()
    want = M.sor_filter(pcs, knn, 2, 1.1)
    for got, w in zip((o_pc, o_idx, o_num, i_pc, stats), want):
        assert _same_bits(got.cpu().numpy(), w)
    removed = o_idx[0, :int(o_num[0])].cpu().numpy()
    assert np.isin(planted, removed).all() and np.array_equal(removed, np.flatnonzero(~M.sor_inliers(M.sor_scores(knn, 2), 1.1)[0][0]))
    # given distances, a per-point score of the caller's, and no outlier outputs
    a = ops.sor_filter(dev, torch.from_numpy(knn).to(DEV), k=2, alpha=1.1)
    assert all(torch.equal(x, y) for x, y in zip(a, (o_pc, o_idx, o_num, i_pc)))
    score = torch.from_numpy(M.sor_scores(knn, 2).astype(np.float32)).to(DEV)
    none_pc, none_idx, none_num, only_inl = ops.sor_filter(dev, score, alpha=1.1, want_outliers=False)
    assert none_pc is None and none_idx is None and none_num is None
    assert _same_bits(only_inl.cpu().numpy(), M.sor_filter(pcs, score.cpu().numpy()[:, :, None], 1, 1.1)[3])


# ---------------------------------------------------------------------------------------------------------------------------
# SRS
# ---------------------------------------------------------------------------------------------------------------------------
def _run_srs(pc, drop, seed, counter, slot_offset, with_idx=True):
    lib = _lib()
    import torch
    b, n, _ = pc.shape
    src, kept, idx = Buf(pc.shape, np.float32, pc), Buf(pc.shape, np.float32), Buf((b, drop), np.int32)
    st = lib.lib().geoadv_random_drop(b, n, src.ptr, drop, C.c_ulonglong(seed), C.c_ulonglong(counter), C.c_ulonglong(slot_offset),
                                      kept.ptr, idx.ptr if with_idx else None, lib.stream_handle())
    lib.check(st, "random_drop")
    torch.cuda.synchronize()
    assert _same_bits(src.get(), pc), "the input changed"
    got_idx = idx.get()
    if not with_idx:
        assert (got_idx.reshape(-1).view(np.uint8) == FILL).all()
    return kept.get(), got_idx


@pytest.mark.parametrize("n", [1, 2, 64, 65, 1024, 1025, 2048, 32767])
def test_srs_is_the_model_bit_for_bit(n):
    rng = np.random.default_rng(n)
    pc = (rng.random((3, n, 3), dtype=np.float32) - 0.5).astype(np.float32)
    pc[0, 0, 1] = np.float32(np.nan)                         # points are copied, never computed with
    for di, drop in enumerate(sorted({0, 1, n // 2, n - 1} & set(range(n)))):
        for si, seed in enumerate((0, (1 << 64) - 1)):
            counter, slot_offset = ((0, 0), (5, 1000), ((1 << 64) - 1, (1 << 32) - 3))[(di + si) % 3]
            kept, idx = _run_srs(pc, drop, seed, counter, slot_offset)
            w_kept, w_idx = M.random_drop(pc, drop, seed, counter, slot_offset)
            what = "n=%d drop=%d seed=%d counter=%d slot_offset=%d" % (n, drop, seed, counter, slot_offset)
            assert _same_bits(idx, w_idx), "dropped_idx differs from the model (%s)" % what
            assert _same_bits(kept, w_kept), "kept differs from the model (%s)" % what
            if drop == 0:
                assert _same_bits(kept, pc)
    if n >= 2:
        drop = n // 2
        kept, idx = _run_srs(pc, drop, 3, 1, 0)
        again, again_idx = _run_srs(pc, drop, 3, 1, 0)       # a repeated call gives equal bits
        assert _same_bits(kept, again) and _same_bits(idx, again_idx)
        no_idx, _ = _run_srs(pc, drop, 3, 1, 0, with_idx=False)
        assert _same_bits(kept, no_idx)


@pytest.mark.parametrize("n", [65, 2048])
def test_srs_slot_offset_splits_a_batch(n):
    pc = np.random.default_rng(n).random((4, n, 3), dtype=np.float32)
    drop = n // 3
    kept, idx = _run_srs(pc, drop, 11, 2, 0)
    lo, lo_idx = _run_srs(pc[:2], drop, 11, 2, 0)
    hi, hi_idx = _run_srs(pc[2:], drop, 11, 2, 2)
    assert _same_bits(np.concatenate([lo, hi]), kept) and _same_bits(np.concatenate([lo_idx, hi_idx]), idx)
    # the data plays no part in the draw, and neither does torch's generator
    import torch
    from geometric_adv_amd import ops
    torch.manual_seed(123)
    k2, i2 = ops.random_drop(torch.from_numpy(pc * 2 + 1).to(DEV), drop, 11, counter=2, return_idx=True)
    assert _same_bits(i2.cpu().numpy(), idx) and _same_bits(k2.cpu().numpy(), M.random_drop(pc * 2 + 1, drop, 11, 2)[0])
    only = ops.random_drop(torch.from_numpy(pc).to(DEV), drop, 11, counter=2)
    assert _same_bits(only.cpu().numpy(), kept)
