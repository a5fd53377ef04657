"""CPU: everything geoadv_sor_filter, geoadv_random_drop, their ops and their commands decide before a device is touched, and
the numpy models of both rules (tests/_stat_defense_model.py) against exact arithmetic and at their degenerate inputs.  The
kernels' bits equal the models' (tests/test_gpu_stat_defense.py), so what holds for the models here holds for the kernels."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stat_defense_model as M  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries
# ---------------------------------------------------------------------------------------------------------------------------
def _lib_and_pointers():
    import ctypes as C
    from geometric_adv_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4096)()
    out = (C.c_float * 4096)()
    return C, L, C.cast(buf, C.c_void_p), C.cast(out, C.c_void_p)


def test_sor_entry_refuses_bad_arguments_before_any_launch():
    C, L, p, o = _lib_and_pointers()

    def status(b=1, n=4, pc=p, knn=p, stride=2, k=2, alpha=1.1, inlier=o):
        return L.geoadv_sor_filter(b, n, pc, knn, stride, k, C.c_double(alpha), None, None, None, inlier, None, None)
    for kw in (dict(b=-1), dict(n=0), dict(n=32768), dict(n=-3), dict(k=0), dict(k=3), dict(stride=65, k=2), dict(stride=65, k=65),
               dict(stride=0, k=0), dict(alpha=-0.5), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-float("inf")),
               dict(pc=None), dict(knn=None), dict(inlier=None)):
        assert status(**kw) == 1, kw
        assert b"sor_filter" in L.geoadv_last_error()
    assert status(b=0, pc=None, knn=None, inlier=None) == 0            # no cloud: nothing to do, nothing dereferenced


def test_random_drop_entry_refuses_bad_arguments_before_any_launch():
    C, L, p, o = _lib_and_pointers()
    u64 = C.c_ulonglong

    def status(b=1, n=4, pc=p, drop=2, slot_offset=0, kept=o):
        return L.geoadv_random_drop(b, n, pc, drop, u64(7), u64(0), u64(slot_offset), kept, None, None)
    for kw in (dict(b=-1), dict(n=0), dict(n=32768), dict(drop=-1), dict(drop=4), dict(drop=5), dict(n=1, drop=1),
               dict(slot_offset=1 << 32), dict(slot_offset=(1 << 64) - 1), dict(b=2, slot_offset=(1 << 32) - 1),
               dict(pc=None), dict(kept=None), dict(kept=p), dict(kept=C.c_void_p(p.value + 8))):
        assert status(**kw) == 1, kw
        assert b"random_drop" in L.geoadv_last_error()
    assert status(b=0, pc=None, kept=None) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------------------------------------------------------
class _OnGpu(torch.Tensor):
    """A tensor that claims to live on the GPU: the shape and range checks come after the device check and raise before
    anything asks for its device."""
    is_cuda = True


def _gpu(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(_OnGpu)


def test_sor_filter_op_refuses_bad_inputs_before_any_launch():
    from geometric_adv_amd import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.sor_filter(torch.zeros((2, 16, 3)), torch.zeros((2, 16, 2)))                       # CPU tensors
    with pytest.raises(ValueError):
        ops.sor_filter(_gpu(2, 16, 3, dtype=torch.float64), _gpu(2, 16, 2))
    for pc, knn, kw, msg in ((_gpu(2, 16, 2), _gpu(2, 16, 2), {}, "3d point sets"),
                             (_gpu(16, 3), _gpu(16, 2), {}, "rank"),
                             (_gpu(1, 32768, 3), _gpu(1, 32768, 2), {}, "32767"),
                             (_gpu(2, 0, 3), _gpu(2, 0, 2), {}, "32767"),
                             (_gpu(2, 16, 3), _gpu(2, 16, 2), dict(alpha=-1.0), "alpha"),
                             (_gpu(2, 16, 3), _gpu(2, 16, 2), dict(alpha=float("nan")), "alpha"),
                             (_gpu(2, 16, 3), _gpu(2, 16, 2), dict(alpha=float("inf")), "alpha"),
                             (_gpu(2, 16, 3), _gpu(2, 16, 2), dict(k=3), "k"),
                             (_gpu(2, 16, 3), _gpu(2, 16, 2), dict(k=0), "k"),
                             (_gpu(2, 16, 3), _gpu(2, 16, 65), dict(k=2), "64"),
                             (_gpu(2, 16, 3), _gpu(2, 15, 2), {}, "shape"),
                             (_gpu(2, 16, 3), _gpu(3, 16), {}, "shape"),
                             (_gpu(2, 16, 3), _gpu(2, 16, 2, dtype=torch.float64), {}, "float32"),
                             (_gpu(2, 16, 3), None, dict(k=16), "k"),                        # own kNN: k neighbours need k + 1 points
                             (_gpu(2, 16, 3), None, dict(k=0), "k")):
        with pytest.raises(ValueError, match=msg):
            ops.sor_filter(pc, knn, **kw)


def test_random_drop_op_refuses_bad_inputs_before_any_launch():
    from geometric_adv_amd import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.random_drop(torch.zeros((2, 16, 3)), 4, 0)
    with pytest.raises(ValueError):
        ops.random_drop(_gpu(2, 16, 3, dtype=torch.float64), 4, 0)
    for pc, drop, kw, msg in ((_gpu(2, 16, 2), 4, {}, "3d point sets"), (_gpu(16, 3), 4, {}, "rank"),
                              (_gpu(1, 32768, 3), 4, {}, "32767"), (_gpu(2, 16, 3), 16, {}, "drop"), (_gpu(2, 16, 3), -1, {}, "drop"),
                              (_gpu(2, 1, 3), 1, {}, "drop"), (_gpu(2, 16, 3), 4, dict(seed=-1), "seed"),
                              (_gpu(2, 16, 3), 4, dict(seed=1 << 64), "seed"), (_gpu(2, 16, 3), 4, dict(counter=-1), "counter"),
                              (_gpu(2, 16, 3), 4, dict(counter=1 << 64), "counter"), (_gpu(2, 16, 3), 4, dict(slot_offset=-1), "slot_offset"),
                              (_gpu(2, 16, 3), 4, dict(slot_offset=(1 << 32) - 1), "slot_offset")):
        kw = dict(dict(seed=0), **kw)
        with pytest.raises(ValueError, match=msg):
            ops.random_drop(pc, drop, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# the parsers
# ---------------------------------------------------------------------------------------------------------------------------
def test_parsers_defaults_and_refusals():
    from geometric_adv_amd import run_defense_sor, run_defense_srs, run_defense_surface
    common = ("ae_folder", "attack_pc_idx", "attack_folder", "do_sanity_checks", "top_dir")
    ref = run_defense_surface.build_parser().parse_args([])
    f = run_defense_sor.build_parser().parse_args([])
    assert (f.num_knn_for_defense, f.sor_alpha, f.output_folder_name) == (2, 1.1, "defense_sor_res")
    assert [getattr(f, k) for k in common] == [getattr(ref, k) for k in common]
    f = run_defense_sor.build_parser().parse_args(["--num_knn_for_defense", "8", "--sor_alpha", "0", "--output_folder_name", "x",
                                                   "--do_sanity_checks", "1", "--top_dir", "/t"])
    assert (f.num_knn_for_defense, f.sor_alpha, f.output_folder_name, f.do_sanity_checks, f.top_dir) == (8, 0.0, "x", 1, "/t")
    f = run_defense_srs.build_parser().parse_args([])
    assert (f.drop_num, f.seed, f.output_folder_name) == (500, 0, "defense_srs_res")
    assert [getattr(f, k) for k in common] == [getattr(ref, k) for k in common]
    f = run_defense_srs.build_parser().parse_args(["--drop_num", "40", "--seed", str((1 << 64) - 1)])
    assert (f.drop_num, f.seed) == (40, (1 << 64) - 1)
    # refused before the attack folder is looked for (there is none here)
    for mod, argv, msg in ((run_defense_sor, ["--num_knn_for_defense", "0"], "num_knn_for_defense"),
                           (run_defense_sor, ["--num_knn_for_defense", "65"], "num_knn_for_defense"),
                           (run_defense_sor, ["--sor_alpha", "-1"], "sor_alpha"), (run_defense_sor, ["--sor_alpha", "nan"], "sor_alpha"),
                           (run_defense_sor, ["--sor_alpha", "inf"], "sor_alpha"),
                           (run_defense_srs, ["--drop_num", "-1"], "drop_num"), (run_defense_srs, ["--seed", "-1"], "seed"),
                           (run_defense_srs, ["--seed", str(1 << 64)], "seed")):
        with pytest.raises(SystemExit, match=msg):
            mod.main(argv + ["--top_dir", "/nonexistent"])
    for mod, argv in ((run_defense_sor, ["--sor_alpha", "x"]), (run_defense_sor, ["--knn_dist_thresh", "0.04"]),
                      (run_defense_srs, ["--drop_num", "1.5"]), (run_defense_srs, ["--sor_alpha", "1.1"])):
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(argv)


# ---------------------------------------------------------------------------------------------------------------------------
# the SOR model
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 1000, 1023, 1024, 1025, 4096, 5000, 32767])
def test_sor_model_equals_exact_rational_arithmetic_on_dyadic_scores(n):
    s = M.dyadic_scores(n, n)
    fr = [Fraction(float(v)) for v in s]
    assert all(f.denominator <= 1024 for f in fr)
    total = sum(fr)
    exact_mu = total / n
    assert exact_mu.denominator <= 1024
    mu, var, m = [v[0] for v in M.sor_stats(s[None])]
    assert m == n and Fraction(float(mu)) == exact_mu
    exact_sq = sum((f - exact_mu) ** 2 for f in fr)
    assert var == (float(exact_sq / (n - 1)) if n >= 2 else 0.0)                 # (float(Fraction) rounds correctly, as the one division does)
    if n >= 3:                                                                  # the point at mu: an inlier with alpha = 0
        at_mu = s == mu
        assert at_mu.any()
        inl, _ = M.sor_inliers(s[None], 0.0)
        assert inl[0][at_mu].all() and np.array_equal(inl[0], s <= mu)


def test_sor_model_point_at_the_mean_is_an_inlier_with_alpha_zero():
    s = np.float64([1.0, 2.0, 3.0, 2.0, 1.5, 2.5, 0.25, 3.75])                  # mean 2.0 exactly
    inl, (mu, var, m) = M.sor_inliers(s[None], 0.0)
    assert mu[0] == 2.0 and m[0] == 8 and var[0] > 0
    assert inl[0].tolist() == [True, True, False, True, True, False, True, False]    # s <= mu, the two points AT mu included
    # all equal: var = 0, everything at the mean, all inliers for every alpha
    for alpha in (0.0, 1.1, 1e6):
        inl, (mu, var, m) = M.sor_inliers(np.full((1, 70), 0.375), alpha)
        assert inl.all() and mu[0] == 0.375 and var[0] == 0.0
    # alpha scales the band: 1.1 sigma keeps 3.0 (|d| = 1 <= 1.1 * 1.17), drops 3.75
    inl, (mu, var, m) = M.sor_inliers(s[None], 1.1)
    assert inl[0].tolist() == [True, True, True, True, True, True, True, False]
    inl, _ = M.sor_inliers(s[None], 1e6)
    assert inl.all()


def test_sor_model_non_finite_scores():
    s = M.dyadic_scores(300, 3)
    want = M.sor_stats(s[None])
    bad = np.concatenate([s[:100], [np.nan, np.inf, -np.inf], s[100:]])
    got = M.sor_stats(bad[None])
    # the sums are exact on dyadic scores, so dropping the three non-finite points out of the order changes no bit
    assert got[0][0] == want[0][0] and got[1][0] == want[1][0] and got[2][0] == want[2][0] == 300
    inl, _ = M.sor_inliers(bad[None], 1e6)
    assert not inl[0, 100:103].any() and inl[0, :100].all() and inl[0, 103:].all()
    # through the float32 rows: inf + -inf is NaN, a float32 overflow of the sum cannot happen in float64
    knn = np.float32([[[np.inf, -np.inf], [3e38, 3e38], [1.0, np.nan], [0.5, 0.25]]])
    sc = M.sor_scores(knn, 2)[0]
    assert np.isnan(sc[0]) and sc[1] == float(np.float32(3e38)) and np.isnan(sc[2]) and sc[3] == 0.375
    # m = 0: mu = var = 0, every point an outlier, nothing packed
    pc = np.arange(12, dtype=np.float32).reshape(1, 4, 3)
    o_pc, o_idx, o_num, i_pc, stats = M.sor_filter(pc, np.full((1, 4, 2), np.nan, np.float32), 2, 1.1)
    assert stats[0].tolist() == [0.0, 0.0, 0.0] and o_num[0] == 4 and not i_pc.any()
    assert np.array_equal(o_pc, pc) and o_idx[0].tolist() == [0, 1, 2, 3]
    # m = 1: mu = that score, var = 0, the point is an inlier (s <= mu) and pads the inlier cloud
    knn = np.full((1, 4, 2), np.nan, np.float32)
    knn[0, 2] = [0.5, 1.0]
    o_pc, o_idx, o_num, i_pc, stats = M.sor_filter(pc, knn, 2, 0.0)
    assert stats[0].tolist() == [0.75, 0.0, 1.0] and o_num[0] == 3 and o_idx[0].tolist() == [0, 1, 3, 0]
    assert np.array_equal(i_pc[0], np.tile(pc[0, 2], (4, 1))) and np.array_equal(o_pc[0], pc[0, [0, 1, 3, 3]])


def test_sor_model_summation_order_is_the_rule():
    """The order matters in the last bits, and the model's is the stated one: by p mod T, butterfly, waves ascending."""
    rng = np.random.default_rng(11)
    x = rng.random(5000) * np.exp(rng.normal(0, 8, 5000))
    got = M.fixed_order_sum(x[None])[0]
    acc = np.zeros(M.T)
    for p in range(5000):                                                       # the scalar restatement
        acc[p % M.T] += x[p]
    waves = []
    for w in range(M.T // 64):
        v = acc[64 * w:64 * w + 64].copy()
        for mask in (1, 2, 4, 8, 16, 32):
            v = np.array([v[lane] + v[lane ^ mask] for lane in range(64)])
        assert (v == v[0]).all()                                               # every lane ends with the same bits
        waves.append(v[0])
    total = waves[0]
    for w in waves[1:]:
        total += w
    assert got == total
    assert got != np.sum(x) or got != float(sum(x.tolist()))                    # (and it is not numpy's or the sequential order)


# ---------------------------------------------------------------------------------------------------------------------------
# the SRS model
# ---------------------------------------------------------------------------------------------------------------------------
def test_srs_model_drops_exactly_drop_points_and_splits_by_slot_offset():
    rng = np.random.default_rng(2)
    pc = rng.random((4, 65, 3), dtype=np.float32)
    for drop in (0, 1, 32, 64):
        kept, idx = M.random_drop(pc, drop, seed=5, counter=3)
        assert idx.shape == (4, drop) and idx.dtype == np.int32
        for c in range(4):
            assert len(set(idx[c].tolist())) == drop and (np.diff(idx[c]) > 0).all()
            rest = np.setdiff1d(np.arange(65), idx[c])
            assert np.array_equal(kept[c, :65 - drop], pc[c, rest]) and (kept[c, 65 - drop:] == pc[c, rest[-1]]).all()
        lo = M.random_drop(pc[:2], drop, seed=5, counter=3, slot_offset=0)
        hi = M.random_drop(pc[2:], drop, seed=5, counter=3, slot_offset=2)
        assert np.array_equal(np.concatenate([lo[0], hi[0]]), kept) and np.array_equal(np.concatenate([lo[1], hi[1]]), idx)
    assert np.array_equal(M.random_drop(pc, 0, seed=1)[0].view(np.int32), pc.view(np.int32))      # drop = 0: the bits
    # the draws of a slot are distinct (r is a bijection of p), so (r, p) never needs its second key
    r = M.srs_draws(0, 0, np.arange(8), 32767)
    assert all(len(np.unique(row)) == 32767 for row in r)
    # seeds, counters and slots give different draws
    base = M.srs_dropped(0, 0, [0], 2048, 500)
    for seed, counter, slot in ((1, 0, 0), (0, 1, 0), (0, 0, 1), ((1 << 64) - 1, 0, 0), (0, (1 << 64) - 1, 0)):
        other = M.srs_dropped(seed, counter, [slot], 2048, 500)
        assert not np.array_equal(base, other)
        assert 60 < len(np.intersect1d(base[0], other[0])) < 190               # 500^2 / 2048 = 122 expected in common, sd 8.4
    # stream 48 of batch_gather's key: not the draws of its noise streams 1..3
    import _batch_noise64 as B
    with np.errstate(over="ignore"):
        key = B.mix(B.mix(B.mix(np.uint64(9) + B.G) ^ np.uint64(4)) ^ ((np.uint64(6) << np.uint64(32)) | np.uint64(17)))
        assert M.srs_draws(9, 4, [6], 18)[0, 17] == B.mix(key + np.uint64(48) * B.G)


def test_srs_model_drops_every_point_equally_often():
    """4096 slots x n = 64, drop = 32: every point's drop count is Binomial(4096, 1/2) under a fair draw -- mean 2048, standard
    deviation 32 -- and must lie within 5 standard deviations (a fair draw fails this with probability 64 * 5.7e-7)."""
    idx = M.srs_dropped(seed=0, counter=0, slots=np.arange(4096), n=64, drop=32)
    counts = np.bincount(idx.reshape(-1), minlength=64)
    assert counts.sum() == 4096 * 32
    sd = np.sqrt(4096 * 0.5 * 0.5)
    assert np.abs(counts - 2048).max() <= 5 * sd, counts
