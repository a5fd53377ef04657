"""approx-EMD (csrc/emd.hip) where tests/test_gpu_emd.py stops: the cost and gradient kernels per element at ragged sizes,
the size classes of the level sweeps above 4096 points, which form of a level ran, the argument limits, and non-finite
coordinates.  The reference is the C oracle (oracle/geoadv_oracle.c, the CPU op restated) throughout.

1. emd_cost_partial_kernel / emd_grad1_kernel / emd_grad2_kernel are fed the ORACLE's plan, so nothing of the plan's own
   conditioning is in the comparison:
     grad1  bit-equal: the kernel adds l ascending with `gx -= w * (ox / d)`, contraction off, like the CPU loop;
     cost   rtol 2e-7 (test_gpu_emd.py's number): both sides add the same float products in double, in different orders,
            and round the double once;
     grad2  the kernel's lanes stride k by 64 and fold in six butterfly steps, the CPU adds k ascending: against the float64
            sum of the float32 terms (tests/_emd_model64.py, held to the oracle by tests/test_emd_model_host.py),
                |got - s64| <= (ceil(n / 64) + 8) * 2^-24 * sum_k |t_k|
            per component -- the first-order bound of a recursive sum of ceil(n / 64) terms followed by 6 pairwise steps, plus
            2 units for a last-bit difference in a term.  Derived, not measured.
2. geoadv_debug_emd_sparse_state says which levels walked the cell grid: every sparse-against-dense comparison below first
   asserts that the sparse form RAN (levels 0 and 1; level 2 sits at 0.97 of its threshold at 8192 x 512 and is printed only).
3. The size classes: emd_sparse_bin_kernel<8> (4096 < max(n, m) <= 8192) and the no-scratch path above 8192.
4. Limits: b = 65535 runs, b = 0 touches nothing, b = 65536 / n = 0 / m = 0 / n m > 2^31 are refused before any launch.
5. A NaN or infinite coordinate stays inside its own cloud pair, and that pair's result does not depend on the form.

Every scratch and output buffer of a direct library call sits inside a larger allocation filled with a canary word, at an
address that is only 4-byte aligned (the library's own alignment slack is part of what is checked)."""
import ctypes as C

import numpy as np
import pytest

import _emd_model64 as model

pytestmark = pytest.mark.gpu

REF_TOL = dict(rtol=2e-6, atol=2e-8)            # reference_weights=True against the CPU op, every entry (test_gpu_emd.py)
SP_LEVELS = 3                                   # GEOADV_EMD_SPARSE_LEVELS
SP_MAX_N = 8192                                 # above it there is no sparse scratch (csrc/emd.hip)
CANARY = 0x7FC0DEAD


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class _Guarded:
    """`count` floats inside a larger allocation, everything preset to the canary word."""

    def __init__(self, count, front=65, back=64):
        import torch
        self.front, self.count = front, int(count)
        self.buf = torch.full((front + self.count + back,), CANARY, dtype=torch.int32, device="cuda:0")
        self.t = self.buf[front:front + self.count].view(torch.float32)

    def intact(self):
        return bool((self.buf[:self.front] == CANARY).all()) and bool((self.buf[self.front + self.count:] == CANARY).all())

    def untouched(self):
        return bool((self.buf == CANARY).all())


def _ok(rc):
    from geometric_adv_amd import _lib
    assert rc == 0, _lib.lib().geoadv_last_error()


def _sparse_state(fused, b, n, m, temp):
    from geometric_adv_amd import _lib
    out = (C.c_int * (b * SP_LEVELS * 3))()
    _ok(_lib.lib().geoadv_debug_emd_sparse_state(int(fused), b, n, m, _lib.ptr(temp), out, _lib.stream_handle()))
    return np.ctypeslib.as_array(out).reshape(b, SP_LEVELS, 3).copy()


def _emd(fused, t1, t2, reference_weights, dense_levels=False):
    """geoadv_approx_match_mode (-> (match,)) or geoadv_emd_cost_grad1_mode (-> (cost, grad1)) on guarded buffers, temp of exactly
    *_temp_floats; -> (outputs, sparse state or None for an all-dense call)."""
    from geometric_adv_amd import _lib, ops
    lib = _lib.lib()
    b, n, m = t1.shape[0], t1.shape[1], t2.shape[1]
    mode = ops._emd_mode(reference_weights, dense_levels)
    if fused:
        temp = _Guarded(lib.geoadv_emd_cost_grad1_temp_floats(b, n, m))
        cost, g1 = _Guarded(b), _Guarded(b * n * 3)
        _ok(lib.geoadv_emd_cost_grad1_mode(mode, b, n, m, _lib.ptr(t1), _lib.ptr(t2), _lib.ptr(cost.t), _lib.ptr(g1.t), _lib.ptr(temp.t),
                                           _lib.stream_handle()))
        outs, guards = (cost.t.clone(), g1.t.view(b, n, 3).clone()), (cost, g1, temp)
    else:
        temp = _Guarded(lib.geoadv_approx_match_temp_floats(b, n, m))
        match = _Guarded(b * m * n)
        _ok(lib.geoadv_approx_match_mode(mode, b, n, m, _lib.ptr(t1), _lib.ptr(t2), _lib.ptr(match.t), _lib.ptr(temp.t), _lib.stream_handle()))
        outs, guards = (match.t.view(b, m, n).clone(),), (match, temp)
    state = None if dense_levels else _sparse_state(fused, b, n, m, temp.t)
    for g in guards:
        assert g.intact(), "a canary next to a buffer of %d floats was overwritten" % g.count
    return outs, state


# ---------------------------------------------------------------------------------------------
# 1. cost and gradient kernels, fed the CPU op's own plan
# ---------------------------------------------------------------------------------------------
def _coincident_clouds():
    """The clouds of test_fused_cost_grad1_with_coincident_and_nearly_coincident_points (exact copies, duplicates, a knot within
    1e-20 .. 1e-16 of the origin), built at n = 300, m = 260 so that the oracle stays fast."""
    from conftest import cloud
    rng = np.random.default_rng(77)
    b, n, m = 3, 300, 260
    x1, x2 = cloud(21, b, n).astype(np.float32), cloud(22, b, m).astype(np.float32)
    x2[0, :100] = x1[0, rng.permutation(n)[:100]]
    x2[1, 50:60] = x2[1, 50]
    x1[1, 7] = x2[1, 50]
    x1[2, :40] *= 1e-20
    x2[2, :40] = x1[2, :40][::-1] * np.float32(1.5)
    x2[2, 40:60] = rng.standard_normal((20, 3)).astype(np.float32) * np.float32(3e-17)
    return x1, x2


COST_GRAD_GROUPS = {
    "single_lane_single_row": [(2, 1, 1), (2, 1, 5), (2, 5, 1)],
    "grad2_lanes_and_tails_of_1_and_7": [(2, 63, 17), (2, 65, 7)],
    "workgroup_and_tile_edges": [(2, 255, 1023), (2, 257, 1025), (2, 256, 1024)],
    "second_and_third_tile_ragged": [(2, 300, 1039), (2, 130, 2049)],
    "nine_workgroups_factorr_6": [(3, 2051, 300)],
    "coincident_points": ["coincident"],
}


def _check_cost_and_gradients(oracle, x1, x2):
    from geometric_adv_amd import _lib, ops
    lib = _lib.lib()
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    tag = "b=%d n=%d m=%d" % (b, n, m)
    want = oracle.approx_match(x1, x2)                                   # (b, n, m)
    want_cost = oracle.match_cost(x1, x2, want)
    want_g1, _ = oracle.match_cost_grad(x1, x2, want)
    s64, sabs = model.grad2_f64(model.grad_terms(x1, x2, want))
    t1, t2, mref = _t(x1), _t(x2), _t(want.transpose(0, 2, 1))          # device layout (b, m, n)
    a = (_lib.ptr(t1), _lib.ptr(t2), _lib.ptr(mref))
    st = _lib.stream_handle()
    # the Python ops ...
    cost = ops.match_cost(t1, t2, mref)
    g1, g2 = ops.match_cost_grad(t1, t2, mref)
    # ... and the C entries on guarded buffers: caller-owned workspace, the library's own scratch, grad2 given and NULL
    wf = int(lib.geoadv_match_cost_workspace_floats(b, n, m))
    cost_ws, ws, cost_own = _Guarded(b), _Guarded(wf), _Guarded(b)
    _ok(lib.geoadv_match_cost_ws(b, n, m, *a, _lib.ptr(cost_ws.t), _lib.ptr(ws.t), C.c_size_t(wf), st))
    _ok(lib.geoadv_match_cost(b, n, m, *a, _lib.ptr(cost_own.t), st))
    g1_both, g2_both, g1_only = _Guarded(b * n * 3), _Guarded(b * m * 3), _Guarded(b * n * 3)
    _ok(lib.geoadv_match_cost_grad(b, n, m, *a, _lib.ptr(g1_both.t), _lib.ptr(g2_both.t), st))
    _ok(lib.geoadv_match_cost_grad(b, n, m, *a, _lib.ptr(g1_only.t), None, st))
    for g in (cost_ws, ws, cost_own, g1_both, g2_both, g1_only):
        assert g.intact(), tag
    for name, got in (("ops", cost), ("ws", cost_ws.t), ("own scratch", cost_own.t)):
        np.testing.assert_allclose(got.cpu().numpy(), want_cost, rtol=2e-7, atol=0, err_msg="%s cost (%s)" % (tag, name))
    for name, got in (("ops", g1), ("grad2 given", g1_both.t), ("grad2 NULL", g1_only.t)):
        got = got.cpu().numpy().reshape(b, n, 3)
        assert np.array_equal(got.view(np.int32), want_g1.view(np.int32)), "%s grad1 (%s): %d of %d words differ, max |d| %.3g" % (
            tag, name, (got.view(np.int32) != want_g1.view(np.int32)).sum(), got.size, np.abs(got - want_g1).max())
    bound = model.grad2_bound(sabs, (n + 63) // 64 + 8)
    for name, got in (("ops", g2), ("C entry", g2_both.t)):
        err = np.abs(got.cpu().numpy().reshape(b, m, 3).astype(np.float64) - s64)
        print("%s grad2 (%s): worst error %.3f of the bound" % (tag, name, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), "%s grad2 (%s): %d components outside the bound, worst %.3g against %.3g" % (
            tag, name, (err > bound).sum(), err[err > bound].max(), bound[err > bound].min())


@pytest.mark.parametrize("group", list(COST_GRAD_GROUPS))
def test_cost_and_gradient_kernels_meet_the_cpu_op_on_its_own_plan(oracle, group):
    from conftest import cloud
    for shape in COST_GRAD_GROUPS[group]:
        if shape == "coincident":
            x1, x2 = _coincident_clouds()
        else:
            b, n, m = shape
            x1, x2 = cloud(1000 + n, b, n), cloud(2000 + m, b, m)
        _check_cost_and_gradients(oracle, x1, x2)


# ---------------------------------------------------------------------------------------------
# 3. the size classes above 4096 points (and 2.: the sparse form is seen to run)
# ---------------------------------------------------------------------------------------------
def _blob(seed, b, n, offset):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((b, n, 3)) * 0.022 + offset).astype(np.float32)


def _size_class_clouds(name):
    from conftest import cloud
    if name == "blob6000_in_cube600":            # cells of ~800 points keep the scatter's order; the cube's points next to the blob are heavy
        return _blob(6000, 2, 6000, 0.0), cloud(600, 2, 600)
    if name == "cube600_in_blob6000":            # ... cells of ~3400 points; heavy lists of the small cloud as cloud 1
        return cloud(601, 2, 600), _blob(6001, 2, 6000, 0.1)
    b, n, m = SIZE_CLASSES[name]
    return cloud(n, b, n), cloud(m + 1, b, m)


SIZE_CLASSES = {
    "5000x300": (2, 5000, 300),                  # emd_sparse_bin_kernel<8>, cloud 1 the large one
    "300x5000": (2, 300, 5000),                  # ... cloud 2
    "8192x512": (2, 8192, 512),                  # the last size with scratch
    "4097x4097": (1, 4097, 4097),                # <8> with both clouds large
    "blob6000_in_cube600": (2, 6000, 600),
    "cube600_in_blob6000": (2, 600, 6000),
    "8193x256": (2, 8193, 256),                  # no scratch: every sweep dense
    "256x8200": (2, 256, 8200),
}
FUSED_ONLY = {"64x511": (1, 64, 511), "64x513": (1, 64, 513), "64x1025": (1, 64, 1025),      # PL_TILE: 512 (reference) / 1024 (fast)
              "70x3": (1, 70, 3)}                                                              # fewer points than the 8 waves of a tile walk

_cache = {}


def _case(name):
    """The clouds of a size class on host and device (made once)."""
    key = ("clouds", name)
    if key not in _cache:
        if name in FUSED_ONLY:
            from conftest import cloud
            b, n, m = FUSED_ONLY[name]
            x1, x2 = cloud(n, b, n), cloud(m + 1, b, m)
        else:
            x1, x2 = _size_class_clouds(name)
        _cache[key] = (x1, x2, _t(x1), _t(x2))
    return _cache[key]


def _oracle_plan(name, oracle):
    key = ("oracle", name)
    if key not in _cache:
        x1, x2, _, _ = _case(name)
        _cache[key] = oracle.approx_match(x1, x2)                       # (b, n, m); shared, never written
    return _cache[key]


def _default_run(name, reference_weights):
    """The default (sparse where the device says so) run of both ops, once per size class and weight mode."""
    key = ("run", name, reference_weights)
    if key not in _cache:
        _, _, t1, t2 = _case(name)
        (match,), state = _emd(False, t1, t2, reference_weights)
        (cost, g1), state_fused = _emd(True, t1, t2, reference_weights)
        _cache[key] = dict(match=match, cost=cost, g1=g1, state=state, state_fused=state_fused)
    return _cache[key]


@pytest.mark.parametrize("name", list(SIZE_CLASSES))
def test_size_class_reference_plan_meets_the_cpu_op_on_every_entry(oracle, name):
    """csrc/emd.hip's header: with the CPU op's own weights the plan is within ~2 float ulps of the CPU op on EVERY entry."""
    want = _oracle_plan(name, oracle)
    got = _default_run(name, True)["match"].cpu().numpy().transpose(0, 2, 1)
    np.testing.assert_allclose(got, want, err_msg=name, **REF_TOL)


@pytest.mark.parametrize("reference_weights", [False, True])
@pytest.mark.parametrize("name", list(SIZE_CLASSES))
def test_size_class_sparse_form_runs_and_equals_dense_sweeps(name, reference_weights):
    """The default run against dense_levels=True (the numbers of test_sparse_levels_equal_dense_sweeps), after the sparse form is
    SEEN to have run; a repeat run bit-equal.  Above SP_MAX_N there is no scratch: the temp size is the dense amount, the state
    all zeros, and both runs are the same launches."""
    import torch
    from geometric_adv_amd import _lib
    b, n, m = SIZE_CLASSES[name]
    _, _, t1, t2 = _case(name)
    run = _default_run(name, reference_weights)
    print(name, "use / heavy 1 / heavy 2 per cloud and level:", run["state"].tolist())
    assert np.array_equal(run["state"], run["state_fused"])            # the same decision in both ops
    if max(n, m) > SP_MAX_N:
        dense_floats = 2 * b * (n + m) * 12 + 16                        # remL, remR and 11 levels of fL, fR in doubles, + slack
        assert _lib.lib().geoadv_approx_match_temp_floats(b, n, m) == dense_floats
        assert _lib.lib().geoadv_emd_cost_grad1_temp_floats(b, n, m) == dense_floats + 2 * b * ((n + 63) // 64) + 16
        assert not run["state"].any()
    else:
        assert (run["state"][:, :2, 0] == 1).all(), run["state"].tolist()
        if name.startswith("blob"):
            assert (run["state"][:, :2, 2] > 0).all()                   # the cube's points next to the blob: heavy
        if name.startswith("cube"):
            assert (run["state"][:, :2, 1] > 0).all()
    (md,), _ = _emd(False, t1, t2, reference_weights, dense_levels=True)
    (cd, gd), _ = _emd(True, t1, t2, reference_weights, dense_levels=True)
    torch.testing.assert_close(run["match"], md, rtol=2e-6, atol=2e-8)
    torch.testing.assert_close(run["cost"], cd, rtol=1e-6, atol=0)
    torch.testing.assert_close(run["g1"], gd, rtol=1e-5, atol=1e-7)
    if max(n, m) > SP_MAX_N:
        assert torch.equal(run["match"], md) and torch.equal(run["cost"], cd) and torch.equal(run["g1"], gd)
    (again,), state = _emd(False, t1, t2, reference_weights)
    (cost, g1), _ = _emd(True, t1, t2, reference_weights)
    assert torch.equal(again, run["match"]) and torch.equal(cost, run["cost"]) and torch.equal(g1, run["g1"])
    assert np.array_equal(state, run["state"])


@pytest.mark.parametrize("name", list(SIZE_CLASSES))
def test_size_class_fast_plan_ships_the_capacities(name):
    """Row and column sums against factorl = max(n, m) / n and factorr = max(n, m) / m (integer division), atol 1e-3 as in
    test_approx_match_harness_shape_n4096_m1024.  Where the division leaves a remainder the two sides hold different totals
    (5000 x 300: 5000 sources of capacity 1 against 300 targets of capacity 16 = 4800), so only the side with the smaller total
    can be used up -- that side EQUALS its factor, the other stays at or below its own (the CPU op does the same: its rows fall
    to 0.43 there)."""
    b, n, m = SIZE_CLASSES[name]
    match = _default_run(name, False)["match"].double()                 # (b, m, n)
    big = max(n, m)
    fl, fr = big // n, big // m
    rows, cols = match.sum(1).cpu().numpy(), match.sum(2).cpu().numpy()  # per source k, per target l
    assert (match >= 0).all()
    if n * fl <= m * fr:
        np.testing.assert_allclose(rows, float(fl), rtol=0, atol=1e-3)
    if m * fr <= n * fl:
        np.testing.assert_allclose(cols, float(fr), rtol=0, atol=1e-3)
    assert rows.max() <= fl + 1e-3 and cols.max() <= fr + 1e-3


@pytest.mark.parametrize("reference_weights", [False, True])
@pytest.mark.parametrize("name", list(SIZE_CLASSES) + list(FUSED_ONLY))
def test_size_class_fused_cost_grad1_equals_the_three_ops(name, reference_weights):
    """emd_cost_grad1 against match_cost / match_cost_grad on the same mode's plan (the three ops are pinned by section 1), at the
    numbers of test_fused_cost_grad1_equals_the_three_ops."""
    import torch
    from geometric_adv_amd import ops
    _, _, t1, t2 = _case(name)
    run = _default_run(name, reference_weights)
    want_cost = ops.match_cost(t1, t2, run["match"])
    want_g1, _ = ops.match_cost_grad(t1, t2, run["match"])
    torch.testing.assert_close(run["cost"], want_cost, rtol=2e-6, atol=0)
    sc = want_g1.abs().amax((1, 2), keepdim=True)
    torch.testing.assert_close(run["g1"] / sc, want_g1 / sc, rtol=0, atol=1e-5)


@pytest.mark.parametrize("name", list(SIZE_CLASSES))
def test_size_class_fast_mode_within_the_statistical_bound_of_reference_mode(name):
    """The fast weights against the reference weights (themselves within REF_TOL of the CPU op at these sizes, above): entries
    outside 2e-6 + 2e-5 |ref| are at most 1e-5 of all, and no entry is off by 1e-3 -- the bound of
    test_config3_per_gpu_shape_b128_chamfer_plus_emd, measured there at 2048 x 2048.  Measured here: no entry outside the strict
    bound at any of these sizes, worst difference 4.5e-6 (4097 x 4097)."""
    fast, ref = _default_run(name, False)["match"], _default_run(name, True)["match"]
    diff = (fast - ref).abs()
    share = float((diff > 2e-6 + 2e-5 * ref.abs()).double().mean())
    worst = float(diff.max())
    print("%s: share outside the strict bound %.3g, worst %.3g" % (name, share, worst))
    assert share <= 1e-5, (share, worst)
    assert worst < 1e-3, (share, worst)


# ---------------------------------------------------------------------------------------------
# 4. limits and refusals
# ---------------------------------------------------------------------------------------------
def test_largest_batch_runs(oracle):
    """b = 65535 (the grid's y limit), n = 1, m = 2: factorl = 2, so each target takes one unit of its only source."""
    import torch
    from geometric_adv_amd import ops
    b = 65535
    rng = np.random.default_rng(5)
    x1 = (rng.random((b, 1, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    x2 = (rng.random((b, 2, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    want = oracle.approx_match(x1, x2)                                   # (b, 1, 2)
    np.testing.assert_allclose(want, 1.0, atol=1e-6)
    t1, t2 = _t(x1), _t(x2)
    for reference_weights in (False, True):
        match = ops.approx_match(t1, t2, reference_weights)             # (b, 2, 1)
        np.testing.assert_allclose(match.cpu().numpy().transpose(0, 2, 1), want, **(REF_TOL if reference_weights else dict(rtol=2e-5, atol=2e-6)))
        cost, g1 = ops.emd_cost_grad1(t1, t2, reference_weights)
        want_cost = ops.match_cost(t1, t2, match)
        torch.testing.assert_close(cost, want_cost, rtol=2e-6, atol=0)
    mref = _t(want.transpose(0, 2, 1))
    np.testing.assert_allclose(ops.match_cost(t1, t2, mref).cpu().numpy(), oracle.match_cost(x1, x2, want), rtol=2e-7, atol=0)
    g1, g2 = ops.match_cost_grad(t1, t2, mref)
    w1, w2 = oracle.match_cost_grad(x1, x2, want)
    assert np.array_equal(g1.cpu().numpy().view(np.int32), w1.view(np.int32))
    assert np.array_equal(g2.cpu().numpy().view(np.int32), w2.view(np.int32))          # n = 1: one term, no sum


def _entry_families(b, n, m, bufs):
    """Every EMD entry with the given sizes on the given (small) buffers -> [(name, status)]."""
    from geometric_adv_amd import _lib
    lib = _lib.lib()
    x1, x2, match, out, g1, g2, temp = (_lib.ptr(g.t) for g in bufs)
    st = _lib.stream_handle()
    return [
        ("approx_match_mode fast", lib.geoadv_approx_match_mode(0, b, n, m, x1, x2, match, temp, st)),
        ("approx_match_mode reference", lib.geoadv_approx_match_mode(1, b, n, m, x1, x2, match, temp, st)),
        ("approx_match", lib.geoadv_approx_match(b, n, m, x1, x2, match, temp, st)),
        ("emd_cost_grad1_mode fast", lib.geoadv_emd_cost_grad1_mode(0, b, n, m, x1, x2, out, g1, temp, st)),
        ("emd_cost_grad1_mode reference", lib.geoadv_emd_cost_grad1_mode(1, b, n, m, x1, x2, out, g1, temp, st)),
        ("emd_cost_grad1", lib.geoadv_emd_cost_grad1(b, n, m, x1, x2, out, g1, temp, st)),
        ("match_cost", lib.geoadv_match_cost(b, n, m, x1, x2, match, out, st)),
        ("match_cost_ws", lib.geoadv_match_cost_ws(b, n, m, x1, x2, match, out, temp, C.c_size_t(1 << 20), st)),
        ("match_cost_grad", lib.geoadv_match_cost_grad(b, n, m, x1, x2, match, g1, g2, st)),
        ("match_cost_grad, grad2 NULL", lib.geoadv_match_cost_grad(b, n, m, x1, x2, match, g1, None, st)),
    ]


@pytest.mark.parametrize("b,n,m,says", [(65536, 1, 2, b"exceeds 65535"), (2, 0, 5, b"at least one point"), (2, 5, 0, b"at least one point"),
                                         (1, 65536, 32769, b"n*m too large"), (-1, 5, 5, b"b >= 0")])
def test_emd_sizes_out_of_range_are_refused_before_any_launch(b, n, m, says):
    """emd_check runs before a pointer is used: 64-float dummy buffers, all of them untouched afterwards."""
    import torch
    from geometric_adv_amd import _lib
    bufs = [_Guarded(64) for _ in range(7)]
    for name, rc in _entry_families(b, n, m, bufs):
        msg = _lib.lib().geoadv_last_error()
        assert rc != 0 and says in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in bufs)


def test_empty_batch_is_ok_and_touches_nothing():
    import torch
    bufs = [_Guarded(64) for _ in range(7)]
    for name, rc in _entry_families(0, 5, 7, bufs):
        assert rc == 0, name
    torch.cuda.synchronize()
    assert all(g.untouched() for g in bufs)


# ---------------------------------------------------------------------------------------------
# 5. non-finite coordinates
# ---------------------------------------------------------------------------------------------
def _same_where_finite(a, b, rtol, atol):
    import torch
    assert torch.equal(torch.isnan(a), torch.isnan(b)), "NaN patterns differ: %d against %d" % (int(torch.isnan(a).sum()), int(torch.isnan(b).sum()))
    both = torch.isfinite(a) & torch.isfinite(b)
    torch.testing.assert_close(a[both], b[both], rtol=rtol, atol=atol)


@pytest.mark.parametrize("reference_weights", [False, True])
@pytest.mark.parametrize("which,value", [(1, np.nan), (1, np.inf), (2, np.nan), (2, -np.inf)])
def test_a_non_finite_coordinate_stays_in_its_cloud_pair_and_takes_the_dense_sweeps(which, value, reference_weights):
    """b = 3, one bad coordinate in cloud pair 1.  Pairs 0 and 2 are bit-equal to a run of those two alone; pair 1 keeps the dense
    sweeps at every level (csrc/emd.hip, "Sparse levels": otherwise a NaN point would sit in cell 0 and meet only the points
    around it, where the dense sweep lets it meet every point) and so returns the same NaN pattern and the same finite values
    whether or not the call asks for dense levels.  What the CPU op returns for such a cloud is not reproduced."""
    import torch
    from geometric_adv_amd import ops
    from conftest import cloud
    b, n, m = 3, 300, 200
    x1, x2 = cloud(31, b, n), cloud(32, b, m)
    (x1 if which == 1 else x2)[1, 17, 1] = value
    t1, t2 = _t(x1), _t(x2)
    (match,), state = _emd(False, t1, t2, reference_weights)
    (cost, g1), state_fused = _emd(True, t1, t2, reference_weights)
    mg1, mg2 = ops.match_cost_grad(t1, t2, match)
    torch.cuda.synchronize()                                             # status OK and no fault behind it
    print("use per cloud pair and level:", state[:, :, 0].tolist())
    assert np.array_equal(state, state_fused)
    # the neighbours
    keep = [0, 2]
    k1, k2 = _t(x1[keep]), _t(x2[keep])
    (match_k,), _ = _emd(False, k1, k2, reference_weights)
    (cost_k, g1_k), _ = _emd(True, k1, k2, reference_weights)
    mg1_k, mg2_k = ops.match_cost_grad(k1, k2, match_k)
    assert torch.isfinite(match_k).all() and torch.isfinite(cost_k).all() and torch.isfinite(g1_k).all()
    for got, alone in ((match, match_k), (cost, cost_k), (g1, g1_k), (mg1, mg1_k), (mg2, mg2_k)):
        assert torch.equal(got[keep], alone)
    # the pair with the bad point: the same whichever form was asked for
    (md,), _ = _emd(False, t1, t2, reference_weights, dense_levels=True)
    (cd, gd), _ = _emd(True, t1, t2, reference_weights, dense_levels=True)
    _same_where_finite(match[1], md[1], 2e-6, 2e-8)
    _same_where_finite(cost[1:2], cd[1:2], 1e-6, 0)
    _same_where_finite(g1[1], gd[1], 1e-5, 1e-7)
    # ... because it kept the dense sweeps, while its neighbours walked the grid
    assert (state[1, :, 0] == 0).all() and (state[[0, 2], :2, 0] == 1).all(), state.tolist()
