"""GPU: farthest point sampling (csrc/sampling.hip) against the numpy model of tests/_fps_model.py.  Every comparison is exact:
array_equal on idx, bit equality on sampled and mindist.  Inputs sit inside NaN-filled larger buffers, outputs inside
pattern-filled ones, and nothing outside the output extents may change."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _fps_model import fps_batch  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 37                    # floats / ints in front of and behind every buffer (odd: the payload is only 4-byte aligned)
PATTERN = 0x5A5A1234        # what the output buffers hold before the call
FORMS = {"auto": 0, "workgroup": 1, "wave": 2}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def run_raw(x, m, start=None, form="auto", want_sampled=True, want_mindist=True):
    """geoadv_farthest_point_sample through the C ABI on guarded buffers -> (idx (b,m), sampled (b,m,3) or None, mindist (b,n) or None)."""
    from geometric_adv_amd import _lib
    x = np.ascontiguousarray(x, dtype=np.float32)
    b, n, _ = x.shape
    dev = torch.device("cuda:0")
    host_in = np.full(2 * PAD + b * n * 3, np.nan, np.float32)
    host_in[PAD:PAD + b * n * 3] = x.ravel()
    d_in = torch.from_numpy(host_in).to(dev)
    counts = {"idx": b * m, "sampled": b * m * 3, "mindist": b * n}
    bufs = {k: torch.full((2 * PAD + c,), PATTERN, dtype=torch.int32, device=dev) for k, c in counts.items()}
    d_start = None if start is None else torch.from_numpy(np.ascontiguousarray(start, dtype=np.int32)).to(dev)

    def at(t):
        return C.c_void_p(t.data_ptr() + 4 * PAD)
    with torch.cuda.device(dev):
        rc = _lib.lib().geoadv_farthest_point_sample(b, n, at(d_in), m, _lib.ptr(d_start), FORMS[form], at(bufs["idx"]),
                                                     at(bufs["sampled"]) if want_sampled else None,
                                                     at(bufs["mindist"]) if want_mindist else None, _lib.stream_handle())
    _lib.check(rc, "farthest_point_sample")
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy().view(np.int32), host_in.view(np.int32)), "the input buffer changed"
    host = {k: t.cpu().numpy() for k, t in bufs.items()}
    for k, c in counts.items():
        written = c if (k == "idx" or (k == "sampled" and want_sampled) or (k == "mindist" and want_mindist)) else 0
        assert (host[k][:PAD] == PATTERN).all() and (host[k][PAD + written:] == PATTERN).all(), "%s: written outside its extent" % k
    idx = host["idx"][PAD:PAD + b * m].reshape(b, m)
    sampled = host["sampled"][PAD:PAD + b * m * 3].view(np.float32).reshape(b, m, 3) if want_sampled else None
    mindist = host["mindist"][PAD:PAD + b * n].view(np.float32).reshape(b, n) if want_mindist else None
    return idx, sampled, mindist


def same(got, want):
    """(idx, sampled, mindist) triples are equal: the indices, and the floats bit for bit."""
    return (np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[2]), bits(want[2])))


def check(x, m, start=None, form="auto", want=None):
    """One guarded call against the model (computed here unless `want` brings it) -> the model's (idx, sampled, t)."""
    want = fps_batch(x, m, start) if want is None else want
    idx, sampled, mindist = run_raw(x, m, start, form)
    assert np.array_equal(idx, want[0]), "idx differs (form %s)" % form
    assert np.array_equal(bits(sampled), bits(want[1])), "sampled differs (form %s)" % form
    assert np.array_equal(bits(mindist), bits(want[2])), "mindist differs (form %s)" % form
    return want


def forms_for(n):
    return ("auto", "workgroup", "wave") if n <= 1024 else ("auto", "workgroup")


def random_clouds(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def plan_by_the_rule(n, form):
    """The dispatch rule as documented (include/geoadv.h, csrc/sampling.hip): the form, then the smallest instance that holds n."""
    if form == "auto":
        form = "wave" if n <= 256 else "workgroup"
    if form == "wave":
        return ("wave", 1, 1 if n <= 64 else 4 if n <= 256 else 16)
    for limit, waves, ppt in ((256, 4, 1), (1024, 4, 4), (2048, 8, 4), (4096, 16, 4), (8192, 16, 8), (16384, 16, 16)):
        if n <= limit:
            return ("workgroup", waves, ppt)


# the issue's sizes, then every boundary between two instances or forms, +-1, that the list does not hold already
SIZES = [(1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (255, 17), (256, 256), (257, 100), (1023, 1023), (1025, 64), (2048, 2048),
         (4097, 33), (16383, 64), (16384, 2048),
         (1024, 64), (2047, 33), (2049, 33), (4095, 33), (4096, 33), (8191, 33), (8192, 33), (8193, 33)]


@functools.lru_cache(maxsize=None)
def sized_case(n, m):
    x = random_clouds(1000 + n, 3, n)
    start = np.array([0, n // 2, n - 1])
    return x, start, fps_batch(x, m, start)


@pytest.mark.parametrize("n,m", SIZES)
def test_sizes_and_dispatch_boundaries(n, m):
    from geometric_adv_amd import ops
    x, start, want = sized_case(n, m)
    for form in forms_for(n):
        assert ops.farthest_point_sample_plan(n, form) == plan_by_the_rule(n, form)
        check(x, m, start, form, want)                                                    # b = 3
        check(x[:1], m, start[:1], form, tuple(w[:1] for w in want))                      # b = 1
    if n > 1024:
        with pytest.raises(ValueError):
            ops.farthest_point_sample_plan(n, "wave")
    if m == n:                                                                            # the cloud in farthest-point order
        assert all(len(np.unique(c, axis=0)) == n for c in x), "the input points are not distinct"
        assert (np.sort(want[0], axis=1) == np.arange(n)).all()


def test_the_instances_the_sizes_cover():
    """Every kernel instance of the library is reached by the size list, from both sides of each of its limits."""
    reached = {plan_by_the_rule(n, f) for n, _ in SIZES for f in forms_for(n)}
    assert reached == {("wave", 1, 1), ("wave", 1, 4), ("wave", 1, 16), ("workgroup", 4, 1), ("workgroup", 4, 4), ("workgroup", 8, 4),
                       ("workgroup", 16, 4), ("workgroup", 16, 8), ("workgroup", 16, 16)}
    ns = {n for n, _ in SIZES}
    for limit in (64, 256, 1024, 2048, 4096, 8192):
        assert {limit - 1, limit, limit + 1} <= ns
    assert {16383, 16384} <= ns


def test_more_workgroups_than_compute_units():
    x = random_clouds(7, 300, 64)
    start = np.arange(300) % 64
    want = fps_batch(x, 64, start)
    for form in ("auto", "workgroup"):
        check(x, 64, start, form, want)
    assert (np.sort(want[0], axis=1) == np.arange(64)).all()


@pytest.mark.parametrize("n,form", [(1024, "wave"), (1024, "workgroup"), (2000, "workgroup"), (200, "wave"), (200, "workgroup"), (16384, "workgroup")])
def test_farthest_point_at_every_edge_of_the_layout(n, form):
    """A tight cluster and ONE far point, placed at the first and last index, at the first and last lane of a wave, and at the
    first and last slot of a thread's register block (thread j of T holds j, j + T, ...): the second pick is that point."""
    _, waves, ppt = plan_by_the_rule(n, form)
    T = 64 * waves
    spots = {0, 63, 64, T - 1, T, (ppt - 1) * T, (ppt - 1) * T + 63, ppt * T - 1, n - 64, n - 1}
    spots = sorted(p for p in spots if 0 <= p < n)
    start = 101                                                     # none of the spots
    assert start not in spots
    x = np.repeat(random_clouds(n, 1, n) * np.float32(0.01), len(spots), axis=0)
    for c, p in enumerate(spots):
        x[c, p] = (3.0, -2.0, 5.0)
    want = check(x, 3, np.full(len(spots), start), form)
    assert want[0][:, 0].tolist() == [start] * len(spots) and want[0][:, 1].tolist() == spots


@pytest.mark.parametrize("n", [1, 100, 300, 1500])
def test_coincident_cloud_padding_never_wins(n):
    x = np.full((2, n, 3), 0.25, np.float32)
    start = np.array([min(5, n - 1), 0])
    m = min(n, 10)
    for form in forms_for(n):
        want = check(x, m, start, form)
    assert (want[0][:, 1:] == 0).all() and (want[2] == 0).all()


def test_ties_on_the_lattice_and_on_a_repeated_cloud():
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, 512, 3)
    for form in forms_for(512):
        want = check(lattice, 512, None, form)
    assert want[0][0, :5].tolist() == [0, 511, 31, 248, 451]
    assert sorted(want[0][0].tolist()) == list(range(512))
    half = random_clouds(3, 2, 128)
    x = np.concatenate([half, half], axis=1)                        # n = 256: the second half repeats the first
    for form in forms_for(256):
        want = check(x, 200, None, form)
    for row in want[0]:
        assert len(set(row[:128].tolist())) == 128 and (row[:128] < 128).all() and (row[128:] == 0).all()


@pytest.mark.parametrize("n", [200, 700, 5000])
def test_non_finite_points(n):
    good = random_clouds(11, 2, n)
    nan0, inf1, far, allnan, nanstart = (good[0].copy() for _ in range(5))
    nan0[0, 1] = np.nan                                             # a NaN at point 0, with start 0: emitted, then never again
    inf1[n // 3, 2] = np.inf
    inf1[n - 1, 0] = -np.inf
    far[n // 2] = 1e30                                              # finite, but its distances overflow to +inf
    allnan[:] = np.nan
    nanstart[7] = np.nan
    batch = np.stack([good[0], nan0, good[1], allnan, inf1, far, nanstart])
    start = np.array([0, 0, 4, 3, 0, 0, 7])
    m = min(n, 150)
    for form in forms_for(n):
        want = check(batch, m, start, form)
    idx, _, t = want
    assert idx[1, 0] == 0 and (idx[1, 1:] != 0).all() and t[1, 0] == -1
    assert idx[3].tolist() == [3] + [0] * (m - 1) and (t[3] == -1).all()
    assert n // 3 not in idx[4] and n - 1 not in idx[4]
    assert idx[5, 1] == n // 2 and np.isfinite(t[5]).all()
    assert idx[6, 0] == 7 and idx[6, 1] == 0 and 7 not in idx[6, 1:]
    assert not np.isnan(t).any()
    # the finite neighbours of those clouds come out as they do alone
    assert same(run_raw(good, m, start[[0, 2]]), tuple(w[[0, 2]] for w in want))


def test_start_forms_of_the_op():
    from geometric_adv_amd import ops
    n, m = 333, 40
    x = random_clouds(21, 4, n)
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(x).to(dev)

    def call(start):
        idx, pts, md = ops.farthest_point_sample(xd, m, start=start, return_points=True, return_mindist=True)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (4, m) and tuple(pts.shape) == (4, m, 3) and tuple(md.shape) == (4, n)
        return idx.cpu().numpy(), pts.cpu().numpy(), md.cpu().numpy()

    starts = np.array([5, 0, 332, 100])
    want = fps_batch(x, m, starts)
    assert same(call(torch.from_numpy(starts.astype(np.int32)).to(dev)), want)
    assert same(call(torch.from_numpy(starts.astype(np.int64)).to(dev)), want)
    assert same(call(torch.from_numpy(starts.astype(np.int64))), want)                       # a host tensor
    assert same(call(starts), want)                                                          # a numpy array
    assert same(call(starts.tolist()), want)
    assert same(call(17), fps_batch(x, m, 17))
    zero = fps_batch(x, m, None)
    assert same(call(None), zero)
    assert same(call(0), zero)
    for out_of_range in (-1, n, 2 ** 40):                                              # read as 0
        assert same(call(out_of_range), zero)
    mixed = np.array([-1, 5, n, 2 ** 40], dtype=np.int64)
    assert same(call(torch.from_numpy(mixed).to(dev)), fps_batch(x, m, [0, 5, 0, 0]))
    assert same(call(mixed), fps_batch(x, m, [0, 5, 0, 0]))
    assert np.array_equal(ops.farthest_point_sample(xd, m).cpu().numpy(), zero[0])    # idx alone
    idx, md = ops.farthest_point_sample(xd, m, return_mindist=True, form="wave")
    assert np.array_equal(idx.cpu().numpy(), zero[0]) and np.array_equal(bits(md.cpu().numpy()), bits(zero[2]))
    with pytest.raises(ValueError):
        ops.farthest_point_sample(xd, m, start=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.farthest_point_sample(xd, m, start=torch.zeros(4, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        ops.farthest_point_sample(xd, n + 1)
    with pytest.raises(ValueError):
        ops.farthest_point_sample(torch.zeros((1, 1025, 3), device=dev), 4, form="wave")


def test_optional_outputs_may_be_null():
    x = random_clouds(31, 2, 500)
    want = fps_batch(x, 30)
    for sampled, mindist in ((False, False), (True, False), (False, True)):
        idx, s, t = run_raw(x, 30, None, "auto", sampled, mindist)
        assert np.array_equal(idx, want[0])
        assert s is None or np.array_equal(bits(s), bits(want[1]))
        assert t is None or np.array_equal(bits(t), bits(want[2]))


@pytest.mark.parametrize("n", [700, 3000])
def test_independent_of_batch_and_position_and_repeatable(n):
    x = random_clouds(41, 5, n)
    start = np.array([3, 0, n - 1, 17, 200])
    m = 120
    want = check(x, m, start)
    assert same(run_raw(x, m, start), run_raw(x, m, start))       # two calls are bit-equal
    order = np.array([4, 2, 0, 3, 1])
    check(x[order], m, start[order], want=tuple(w[order] for w in want))
    for c in range(5):
        check(x[c:c + 1], m, start[c:c + 1], want=tuple(w[c:c + 1] for w in want))


def test_both_forms_agree_bit_for_bit():
    for n, m in ((64, 64), (200, 200), (1024, 300)):
        x = random_clouds(51 + n, 7, n)
        assert same(run_raw(x, m, None, "workgroup"), run_raw(x, m, None, "wave"))


def test_sampled_is_the_gather_of_the_input():
    x = random_clouds(61, 3, 900)
    x[1, 5] = np.float32(-0.0)                                      # signed zeros and denormals travel as bits
    x[2, 9] = np.float32(1e-41)
    idx, sampled, _ = run_raw(x, 900)
    assert all(len(np.unique(c, axis=0)) == 900 for c in x)
    assert (np.sort(idx, axis=1) == np.arange(900)).all()
    assert np.array_equal(bits(sampled), bits(np.take_along_axis(x, idx[:, :, None].astype(np.int64), axis=1)))


def test_resample_clouds_cli(tmp_path):
    from geometric_adv_amd import resample_clouds
    x = random_clouds(71, 5, 300)
    src, out, sidx = (str(tmp_path / f) for f in ("in.npy", "out.npy", "idx.npy"))
    np.save(src, x)
    resample_clouds.main(["--input", src, "--output", out, "--n_points", "128", "--batch_size", "2", "--save_idx", sidx])
    want = fps_batch(x, 128)
    got, got_idx = np.load(out), np.load(sidx)
    assert got.dtype == np.float32 and got.shape == (5, 128, 3) and got_idx.dtype == np.int32
    assert np.array_equal(got_idx, want[0]) and np.array_equal(bits(got), bits(want[1]))
    starts = np.random.RandomState(3).randint(0, 300, size=5)
    want = fps_batch(x, 128, starts)
    for _ in range(2):                                              # --start random --seed 3 reproduces
        resample_clouds.main(["--input", src, "--output", out, "--n_points", "128", "--start", "random", "--seed", "3", "--save_idx", sidx])
        assert np.array_equal(np.load(sidx), want[0]) and np.array_equal(bits(np.load(out)), bits(want[1]))
    resample_clouds.main(["--input", src, "--output", out, "--n_points", "300"])           # n_points == n reorders only
    full = np.load(out)
    for c in range(5):
        assert sorted(map(tuple, bits(full[c]).tolist())) == sorted(map(tuple, bits(x[c]).tolist()))
    assert np.array_equal(bits(full), bits(fps_batch(x, 300)[1]))
