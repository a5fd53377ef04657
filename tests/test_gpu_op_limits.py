"""The reference-shaped ops past the sizes and inputs the other files stop at: NnDistanceGrad beyond the term planes,
SelectionSort beyond one element per lane and on non-finite rows, the k-NN kernels at their size limits and on a dataset
with NaN coordinates, QueryBallPoint at point counts that are no multiple of four, GroupPoint at larger shapes and
GroupPointGrad with out-of-range destinations.

Every comparison is bit for bit (integer and ordered-fp32 operations: no tolerances) against the pinned C oracle, or
against a few lines of numpy restating the reference loop where the oracle cannot express the case.  The branch a case
reaches is named by its condition in the source."""
import os

import numpy as np
import pytest

from test_gpu_grouping import knn_kernel  # noqa: F401  (the fixture: all_points / grid / grid_shells)

pytestmark = pytest.mark.gpu

_REF = {}                                         # oracle results shared between the cases that use the same inputs


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _shared(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _unit(seed, b, n):
    return np.random.default_rng(seed).random((b, n, 3), dtype=np.float32)


# ---------------------------------------------------------------------------------------------
# NnDistanceGrad: chamfer_grad_side with P > CG_TERMS_MAX_P = 8192 (no term planes: the scatter terms on the fly)
# ---------------------------------------------------------------------------------------------
def _grad_case(oracle, kind, b, n, m):
    rng = np.random.default_rng(1000 + n + 7 * m + len(kind))
    x1 = (rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    x2 = (rng.random((b, m, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    if kind == "chain":                           # every x1 point matched to x2[0], every x2 point to x1[n - 1]
        idx1 = np.zeros((b, n), np.int32)
        idx2 = np.full((b, m), n - 1, np.int32)
    else:
        if kind == "duplicates":                  # x2 = x1 with its second half a copy of the first: the lowest index wins
            x2 = x1.copy()
            x2[:, n // 2:] = x2[:, :n // 2]
        _, idx1, _, idx2 = oracle.nn_distance(x1, x2)
        if kind == "duplicates":
            assert idx1.max() < n // 2 and np.array_equal(idx1[0, :n // 2], np.arange(n // 2))
    gd1 = rng.standard_normal((b, n)).astype(np.float32)
    gd2 = rng.standard_normal((b, m)).astype(np.float32)
    return x1, x2, gd1, idx1, gd2, idx2


@pytest.mark.parametrize("kind,b,n,m", [
    ("random", 2, 8193, 300),            # side 2 sorts P = 16384 keys without planes, side 1 (P = 512) keeps them
    ("random", 2, 300, 8193),            # the mirror
    ("random", 1, 16385, 16385),         # P = 32768 on both sides: 128 KB of keys
    ("random", 1, 32768, 40),            # the size limit: matches up to 32767 in the key's high half, ~800 terms per x2 point
    ("chain", 1, 9000, 9000),            # one ordered chain of 9000 terms, 8999 empty segments
    ("duplicates", 1, 9000, 9000)])
def test_nn_distance_grad_without_term_planes(oracle, kind, b, n, m):
    from geometric_adv_amd import ops
    x1, x2, gd1, idx1, gd2, idx2 = _grad_case(oracle, kind, b, n, m)
    want1, want2 = oracle.nn_distance_grad(x1, x2, gd1, idx1, gd2, idx2)
    got1, got2 = ops.nn_distance_grad(_t(x1), _t(x2), _t(gd1), _t(idx1), _t(gd2), _t(idx2))
    assert np.array_equal(got1.cpu().numpy(), want1)
    assert np.array_equal(got2.cpu().numpy(), want2)


def test_nn_distance_autograd_past_the_plane_limit(oracle):
    """(d1.sum() + d2.sum()).backward() at (1, 8193, 300): the registered gradient, upstream gradients of one."""
    from geometric_adv_amd import ops
    rng = np.random.default_rng(8193)
    x1 = (rng.random((1, 8193, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    x2 = (rng.random((1, 300, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    _, idx1, _, idx2 = oracle.nn_distance(x1, x2)
    want1, want2 = oracle.nn_distance_grad(x1, x2, np.ones((1, 8193), np.float32), idx1, np.ones((1, 300), np.float32), idx2)
    a, c = _t(x1).requires_grad_(True), _t(x2).requires_grad_(True)
    d1, i1, d2, i2 = ops.nn_distance_autograd(a, c)
    (d1.sum() + d2.sum()).backward()
    assert np.array_equal(i1.cpu().numpy(), idx1) and np.array_equal(i2.cpu().numpy(), idx2)
    assert np.array_equal(a.grad.cpu().numpy(), want1)
    assert np.array_equal(c.grad.cpu().numpy(), want2)


def test_nn_distance_grad_refuses_more_than_32768_points():
    """n = 32769: refused with the limit in the message, before anything is launched -- the outputs keep their sentinel."""
    import torch
    from geometric_adv_amd import _lib
    n, m = 32769, 40
    x1 = torch.zeros((1, n, 3), device="cuda:0")
    x2 = torch.zeros((1, m, 3), device="cuda:0")
    gd1, gd2 = torch.ones((1, n), device="cuda:0"), torch.ones((1, m), device="cuda:0")
    i1 = torch.zeros((1, n), dtype=torch.int32, device="cuda:0")
    i2 = torch.zeros((1, m), dtype=torch.int32, device="cuda:0")
    g1, g2 = torch.full_like(x1, -7.5), torch.full_like(x2, -7.5)
    for a_n, a, a_gd, a_i, a_g, c_n, c, c_gd, c_i, c_g in ((n, x1, gd1, i1, g1, m, x2, gd2, i2, g2), (m, x2, gd2, i2, g2, n, x1, gd1, i1, g1)):
        st = _lib.lib().geoadv_nn_distance_grad(1, a_n, _lib.ptr(a), c_n, _lib.ptr(c), _lib.ptr(a_gd), _lib.ptr(a_i), _lib.ptr(c_gd),
                                                _lib.ptr(c_i), _lib.ptr(a_g), _lib.ptr(c_g), _lib.stream_handle())
        with pytest.raises(ValueError, match="32768"):
            _lib.check(st, "nn_distance_grad")
    torch.cuda.synchronize()
    assert bool((g1 == -7.5).all()) and bool((g2 == -7.5).all())


# ---------------------------------------------------------------------------------------------
# SelectionSort: geoadv_selection_sort / wave_selection_sort beyond n = 64
# ---------------------------------------------------------------------------------------------
def _rows(kind, b, m, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.random((b, m, n), dtype=np.float32)
    if kind == "eighths":                         # nine distinct values: exact ties across lanes and streams
        return (np.round(rng.random((b, m, n), dtype=np.float32) * np.float32(8)) / np.float32(8)).astype(np.float32)
    assert kind == "descending"                   # every pass takes the last entry of the rest
    return np.ascontiguousarray(np.broadcast_to(np.arange(n, 0, -1, dtype=np.float32), (b, m, n)))


def _check_selection_sort(oracle, k, dist, nan=False):
    from geometric_adv_amd import ops
    want_idx, want_val = oracle.selection_sort(k, dist)
    idx, val = ops.select_top_k(k, _t(dist))
    assert np.array_equal(idx.cpu().numpy(), want_idx)                      # ALL n entries, not just the first k
    assert np.array_equal(val.cpu().numpy(), want_val, equal_nan=nan)
    return want_idx, want_val


@pytest.mark.parametrize("kind", ["random", "eighths", "descending"])
@pytest.mark.parametrize("b,m,n,k", [
    (2, 5, 65, 7),                       # `t < n; t += 64`: a second element in lane 0 only
    (1, 3, 257, 9),                      # `t + 3 * 64 < n`: the first n that enters the four-stream loop (lane 0 of pass 0)
    (2, 4, 1000, 33),
    (1, 2, 300, 300),                    # k == n
    (1, 2, 300, 400),                    # k > n: `s < k && s < n`
    (1, 3, 16384, 40)])                  # ROW_MAX_N: the 128 KB dynamic-LDS launch
def test_selection_sort_long_rows(oracle, kind, b, m, n, k):
    _check_selection_sort(oracle, k, _rows(kind, b, m, n, 100 * n + k))


def test_selection_sort_more_rows_than_the_grid(oracle):
    """1 048 600 rows against the grid cap of 65535 * 16 = 1 048 560: `row += gridDim.x` iterates for the first 40 blocks."""
    rng = np.random.default_rng(3)
    dist = (np.round(rng.random((1, 1048600, 3), dtype=np.float32) * np.float32(4)) / np.float32(4)).astype(np.float32)
    _check_selection_sort(oracle, 2, dist)


def _nonfinite_rows():
    """n = 300, k = 12.  name -> row; `nan_above_k` is the one row whose NaN cannot reach the first k columns (only the
    entry in slot s ever moves up the row, and a NaN is never chosen as a minimum)."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rng = np.random.default_rng(12)
    rows = {}

    def fresh():
        return rng.random(300, dtype=np.float32)
    r = fresh(); r[2] = nan; rows["nan_at_2"] = r
    r = fresh(); r[70] = nan; rows["nan_above_k"] = r
    r = fresh(); r[[2, 70]] = nan; rows["nan_at_2_and_70"] = r
    r = fresh(); r[[1, 5, 11, 12, 40, 130, 299]] = nan; rows["several"] = r
    r = fresh(); r[0] = nan; rows["slot_0"] = r
    rows["all_nan"] = np.full(300, nan, np.float32)
    r = fresh(); r[[3, 7, 200]] = nan; r[[0, 9, 100, 280]] = inf; r[[5, 64, 257]] = -inf; rows["inf_and_nan"] = r
    r = np.full(300, nan, np.float32); r[5] = np.float32(0.5); rows["finite_after_nans"] = r
    r = np.full(300, inf, np.float32); r[[0, 3]] = nan; r[199] = np.float32(0.25); rows["finite_after_nan_among_inf"] = r
    return rows


def test_selection_sort_nonfinite_rows(oracle):
    """A NaN in slot s is never beaten by `p[t] < p[min]` (tf_grouping_g.cu:83-123): it stays in column s.  The lexicographic
    (value, position) minimum alone skips it and pulls the smallest later value forward."""
    rows = _nonfinite_rows()
    names = list(rows)
    dist = np.stack([rows[r] for r in names])[None]
    k = 12
    _, want_val = _check_selection_sort(oracle, k, dist, nan=True)
    for j, name in enumerate(names):                                         # the cases discriminate: the oracle keeps a NaN in the first k
        assert np.isnan(want_val[0, j, :k]).any() == (name != "nan_above_k"), name
    assert np.isnan(want_val[0, names.index("nan_above_k"), 70])


def test_selection_sort_nonfinite_golden():
    """The reference's own CPU selection sort on NaN / +-inf rows (tests/golden/grouping_nonfinite.npz)."""
    from conftest import GOLDEN
    from geometric_adv_amd import ops
    g = np.load(os.path.join(GOLDEN, "grouping_nonfinite.npz"))
    k = int(g["k"])
    assert np.isnan(g["val"][0, :, :k]).any(axis=1).all()
    idx, val = ops.select_top_k(k, _t(g["dist"]))
    assert np.array_equal(idx.cpu().numpy(), g["idx"])
    assert np.array_equal(val.cpu().numpy(), g["val"], equal_nan=True)


def test_selection_sort_refuses_rows_past_the_lds_limit():
    import torch
    from geometric_adv_amd import ops
    with pytest.raises(ValueError, match="16384"):
        ops.select_top_k(3, torch.zeros((1, 1, 16385), device="cuda:0"))


# ---------------------------------------------------------------------------------------------
# k-NN
# ---------------------------------------------------------------------------------------------
def _check_knn_point(oracle, k, x1, x2, key=None, nan=False):
    from geometric_adv_amd import ops
    want_val, want_idx = _shared(key, lambda: oracle.knn_point(k, x1, x2)) if key else oracle.knn_point(k, x1, x2)
    val, idx = ops.knn_point(k, _t(x1), _t(x2))
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(val.cpu().numpy(), want_val, equal_nan=nan)
    return want_val, want_idx


@pytest.mark.parametrize("b,n,m,k", [
    (2, 64, 9000, 17),                   # k + 1 > 17: knn_kernel<0>; b * m > 16384: qper = 2
    (1, 300, 20000, 20),                 # qper = 2 with b = 1
    (1, 64, 33001, 17),                  # cdiv(m, 2) > 16384: qper = 4, m = 4 * 8250 + 1 (the last block has one query)
    (2, 16384, 70, 20)])                 # ROW_MAX_N: 128 KB of LDS per wave
def test_knn_point_generic_kernel(oracle, b, n, m, k):
    from conftest import cloud
    _check_knn_point(oracle, k, cloud(40 + n, b, n), cloud(50 + m, b, m))


@pytest.mark.parametrize("num_knn", [20, 40])
def test_knn_dists_generic_kernel(oracle, num_knn):
    """knn_kernel<1>: num_knn + 1 > 17 list slots."""
    from conftest import cloud
    from geometric_adv_amd import ops
    pc = cloud(600, 2, 600)
    assert np.array_equal(ops.knn_dists(_t(pc), num_knn).cpu().numpy(), oracle.knn_dists(pc, num_knn))


@pytest.mark.parametrize("n", [5000, 16384])
def test_knn_point_list_kernels_past_the_grid_limit(oracle, knn_kernel, n):
    """n > KG_MAX_N = 4096: knn_uses_grid declines the grid even when it is selected; n = ROW_MAX_N for the redo kernel's LDS."""
    from conftest import cloud
    x1 = cloud(60 + n, 1, n)
    x2 = np.concatenate([x1[:, :150], cloud(61 + n, 1, 150)], axis=1)          # half the queries are dataset points
    _check_knn_point(oracle, 9, x1, x2, key=("past_grid", n))


def test_knn_dists_list_kernels_past_the_grid_limit(oracle, knn_kernel):
    from conftest import cloud
    from geometric_adv_amd import ops
    pc = cloud(4097, 1, 4097)
    want = _shared("dists_4097", lambda: oracle.knn_dists(pc, 8))
    assert np.array_equal(ops.knn_dists(_t(pc), 8).cpu().numpy(), want)


def _nan_dataset():
    from conftest import cloud
    x = cloud(71, 2, 700)
    x[0, 2, 1] = np.nan                           # cloud 0 only: cloud 1's queries stay on the list kernels in the same launch
    x[0, 400, 0] = np.nan
    q = np.concatenate([x[:, :450], cloud(72, 2, 50)], axis=1)                 # the NaN points themselves among the queries
    return x, q


@pytest.mark.parametrize("k", [3, 8])
def test_knn_nan_coordinates_follow_the_reference(oracle, knn_kernel, k):
    """A dataset point with a NaN coordinate: its NaN distance sits in slot 2 of every row and is never beaten, so column 2
    of the reference's result is NaN (index 2) -- for every query of that cloud, through knn_redo_kernel."""
    from geometric_adv_amd import ops
    x, q = _nan_dataset()
    want_val, want_idx = _check_knn_point(oracle, k, x, q, key=("nan_point", k), nan=True)
    assert np.isnan(want_val[0, :, 2]).all() and (want_idx[0, :, 2] == 2).all() and not np.isnan(want_val[1]).any()
    want = _shared(("nan_dists", k), lambda: oracle.knn_dists(x, k))
    assert np.isnan(want[0, :, 1]).all() and not np.isnan(want[1]).any()       # (column 0 of the k + 1 is dropped)
    assert np.array_equal(ops.knn_dists(_t(x), k).cpu().numpy(), want, equal_nan=True)


def test_knn_point_nan_coordinates_generic_kernel(oracle):
    x, q = _nan_dataset()
    want_val, _ = _check_knn_point(oracle, 20, x, q, nan=True)
    assert np.isnan(want_val[0, :, 2]).all()


def test_knn_refusals():
    import torch
    from geometric_adv_amd import ops
    big = torch.zeros((1, 16385, 3), device="cuda:0")
    q = torch.zeros((1, 4, 3), device="cuda:0")
    with pytest.raises(ValueError, match="16384"):
        ops.knn_point(3, big, q)
    with pytest.raises(ValueError, match="16384"):
        ops.knn_dists(big, 3)
    small = torch.rand((2, 30, 3), device="cuda:0")
    with pytest.raises(ValueError, match="n=30"):
        ops.knn_point(31, small, small)                                       # k > n
    with pytest.raises(ValueError, match="29"):
        ops.knn_dists(small, 30)                                              # k = n: the self column leaves n - 1


# ---------------------------------------------------------------------------------------------
# QueryBallPoint: query_ball_fast_kernel with n % 4 != 0 (the NaN pad of the float4 reads decides)
# ---------------------------------------------------------------------------------------------
def _check_query_ball(oracle, radius, ns, x1, x2):
    from geometric_adv_amd import ops
    want_idx, want_cnt = oracle.query_ball_point(radius, ns, x1, x2)
    idx, cnt = ops.query_ball_point(radius, ns, _t(x1), _t(x2))
    assert np.array_equal(cnt.cpu().numpy(), want_cnt), (radius, ns)
    hit = want_cnt > 0                                                        # rows without any hit are left untouched by both
    assert np.array_equal(idx.cpu().numpy()[hit], want_idx[hit]), (radius, ns)
    return want_cnt


@pytest.mark.parametrize("n", [1, 3, 1023, 1025, 2051, 4099])        # 1025, 4099: a last tile of one and of three points
def test_query_ball_point_counts_off_the_float4_grid(oracle, n):
    x1, x2 = _unit(80 + n, 2, n), _unit(90 + n, 2, 300)
    for radius, ns in [(0.2, 16), (0.05, 4), (2.0, 7), (0.3, 64)]:
        cnt = _check_query_ball(oracle, radius, ns, x1, x2)
        if radius == 2.0:
            assert (cnt == min(n, ns)).all()              # every point is a hit: a pad that hit would show here
        if radius == 0.05 and n <= 3:
            assert (cnt == 0).mean() > 0.9                # the untouched-row rule


def test_query_ball_lattice_ties_next_to_the_pad(oracle):
    """n = 1027: three points and one pad in the last group, distances that EQUAL the radius around them."""
    rng = np.random.default_rng(1027)
    lat = (rng.integers(-3, 4, size=(2, 1027, 3)) * 0.25).astype(np.float32)
    q = np.ascontiguousarray(lat[:, -100:])
    for radius in (0.25, float(np.nextafter(np.float32(0.25), np.float32(1))), float(np.nextafter(np.float32(0.25), np.float32(0)))):
        for ns in (8, 64, 1100):
            _check_query_ball(oracle, radius, ns, lat, q)


# ---------------------------------------------------------------------------------------------
# GroupPoint / GroupPointGrad
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n,c,m,ns", [(2, 2048, 64, 2048, 32), (3, 300, 5, 77, 9), (1, 130, 1, 4096, 16), (2, 1000, 3, 900, 16)])
def test_group_point_forward_vs_oracle(oracle, b, n, c, m, ns):
    """Valid indices only (the reference reads out of bounds otherwise); several blocks, channel counts 1, 3, 5, 64."""
    from geometric_adv_amd import ops
    rng = np.random.default_rng(n + c)
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    idx[:, 0, 0], idx[:, -1, -1] = 0, n - 1
    points = rng.standard_normal((b, n, c)).astype(np.float32)
    got = ops.group_point(_t(points), _t(idx)).cpu().numpy()
    assert np.array_equal(got, oracle.group_point(points, idx))


def _scatter_valid(n, idx, grad_out):
    """GroupPointGrad over the valid entries only: float32 sums in entry order (test/query_ball_point.cpp:70-84)."""
    b, c = idx.shape[0], grad_out.shape[-1]
    out = np.zeros((b, n, c), np.float32)
    for i in range(b):
        flat, g = idx[i].ravel(), grad_out[i].reshape(-1, c)
        for e in np.flatnonzero((flat >= 0) & (flat < n)):
            out[i, flat[e]] += g[e]
    return out


@pytest.mark.parametrize("b,n,c,m,ns", [(2, 300, 5, 77, 9), (1, 4096, 3, 2048, 8)])       # the second: three radix passes
def test_group_point_grad_ignores_out_of_range_destinations(oracle, b, n, c, m, ns):
    """gpg_pass_kernel, first pass: `(k < 0 || k >= n) ? n : k` -- invalid destinations sort behind the last point and are never
    summed.  The oracle only ever sees the valid entries."""
    from geometric_adv_amd import ops
    rng = np.random.default_rng(n + m)
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    bad = rng.random((b, m, ns)) < 0.1
    idx[bad] = rng.choice(np.array([-1, -7, n, n + 5, 1 << 30], np.int32), size=int(bad.sum()))
    idx[:, 0, 0], idx[:, -1, -1] = -1, 1 << 30                                 # the first and the last entry too
    points = rng.standard_normal((b, n, c)).astype(np.float32)
    grad_out = rng.standard_normal((b, m, ns, c)).astype(np.float32)
    want = _scatter_valid(n, idx, grad_out)
    for i in range(b):                                                        # the restatement is the oracle's on what it may see
        keep = np.flatnonzero((idx[i].ravel() >= 0) & (idx[i].ravel() < n))
        assert 0.85 * m * ns < keep.size < 0.95 * m * ns
        only = oracle.group_point_grad(points[i:i + 1], idx[i].ravel()[keep].reshape(1, -1, 1), grad_out[i].reshape(-1, c)[keep].reshape(1, -1, 1, c))
        assert np.array_equal(only[0], want[i])
    got = ops.group_point_grad(_t(points), _t(idx), _t(grad_out)).cpu().numpy()
    assert np.array_equal(got, want)
