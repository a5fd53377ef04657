"""GPU parity of approx-EMD against the golden vectors (reference CPU functions,
tf_approxmatch.cpp:23-140).

Tolerances.  The GPU path uses the CPU op's level schedule with fp64 capacities, factors and sums; the pair WEIGHT
exp(level * d2) is fp32 (d2 by FMAs, v_exp_f32) where the CPU op forms d2 in double and calls expf: <= ~3e-6 relative on a
weight.  The plan is a smooth function of the weights except where a nearly exhausted capacity competes with the op's 1e-9
guard; there the weight error is amplified by up to ~10 (csrc/emd.hip header; measured).  So:
  * the reference's golden vectors: rtol 2e-5 / atol 2e-6 on EVERY entry (measured worst case 7e-7 absolute);
  * larger random clouds vs the pinned oracle: the same bound on >= 99.99 % of the entries, and rtol 1e-4 / atol 2e-5 on all
    (measured: 1 entry of 393 216 at 3.0e-5 relative).
With reference_weights=True (GEOADV_EMD_REFERENCE) every pair weight is the CPU op's bit for bit (its double distance, its
float expf argument, glibc's expf algorithm: tests/test_expf_table.py) and the plan's level terms are added in double like
the CPU's: what is left is the order of the fp64 sums, amplified by the same conditioning to at most ~2 float ulps
(measured 2.0e-7 relative over 13 M entries, 40-80 % of them bit-equal).  Held to rtol 2e-6 / atol 2e-8 on EVERY entry at
every size, here and in test_gpu_reference_checks.py.
For scale: the reference's own CPU-vs-GPU check of this op allows 1e-2 ABSOLUTE per entry (approxmatch.cpp:222)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


REF_TOL = dict(rtol=2e-6, atol=2e-8)            # reference_weights=True, every entry


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("reference_weights", [False, True])
def test_approx_match_and_cost_golden(golden_emd, reference_weights):
    from geometric_adv_amd import ops
    g = golden_emd
    for name in g["cases"]:
        x1, x2 = g[f"{name}_xyz1"], g[f"{name}_xyz2"]
        want = g[f"{name}_match_nm"]                                    # CPU layout (b, n, m)
        match = ops.approx_match(_t(x1), _t(x2), reference_weights)     # (b, m, n)
        got = match.cpu().numpy().transpose(0, 2, 1)
        np.testing.assert_allclose(got, want, err_msg=name, **(REF_TOL if reference_weights else dict(rtol=2e-5, atol=2e-6)))
        cost = ops.match_cost(_t(x1), _t(x2), match).cpu().numpy()
        np.testing.assert_allclose(cost, g[f"{name}_cost"], rtol=1e-5, err_msg=name)
        # cost / grad kernels in isolation: feed them the REFERENCE's match
        mref = _t(np.ascontiguousarray(want.transpose(0, 2, 1)))
        cost = ops.match_cost(_t(x1), _t(x2), mref).cpu().numpy()
        np.testing.assert_allclose(cost, g[f"{name}_cost"], rtol=2e-7, err_msg=name)
        g1, g2 = ops.match_cost_grad(_t(x1), _t(x2), mref)
        assert np.array_equal(g1.cpu().numpy(), g[f"{name}_grad1"]), name          # same order => same bits
        np.testing.assert_allclose(g2.cpu().numpy(), g[f"{name}_grad2"], rtol=1e-5, atol=1e-6, err_msg=name)


def test_approx_match_vs_oracle_medium(oracle):
    from geometric_adv_amd import ops
    from conftest import cloud
    x1, x2 = cloud(1, 2, 512), cloud(2, 2, 384)
    want = oracle.approx_match(x1, x2)
    got = ops.approx_match(_t(x1), _t(x2)).cpu().numpy().transpose(0, 2, 1)
    strict = np.abs(got - want) <= 2e-6 + 2e-5 * np.abs(want)
    assert strict.mean() >= 0.9999, strict.mean()
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(got.sum(2), want.sum(2), rtol=1e-4, atol=2e-5)          # mass shipped per source / received per target
    np.testing.assert_allclose(got.sum(1), want.sum(1), rtol=1e-4, atol=2e-5)


def test_approx_match_reference_weights_vs_oracle_every_entry(oracle):
    """The same clouds with the CPU op's own weights: a few float ulps on every entry, plus ragged sizes (tiles of 1024
    staged points, 128 own points per workgroup: 1100 and 300 leave partial ones) and factorl / factorr > 1."""
    from geometric_adv_amd import ops
    from conftest import cloud
    for b, n, m, s1, s2 in [(2, 512, 384, 1, 2), (1, 300, 1100, 5, 6), (1, 1100, 300, 7, 8), (1, 1, 5, 9, 10)]:
        x1, x2 = cloud(s1, b, n), cloud(s2, b, m)
        want = oracle.approx_match(x1, x2)
        got = ops.approx_match(_t(x1), _t(x2), reference_weights=True).cpu().numpy().transpose(0, 2, 1)
        np.testing.assert_allclose(got, want, err_msg=str((n, m)), **REF_TOL)


def test_approx_match_vs_oracle_full_size(oracle):
    """n = m = 2048, two clouds, against the pinned C restatement of the CPU op (well under a second per cloud at -O2), under
    both weight modes' rules: reference_weights=True within REF_TOL on every entry; the fast weights within the strict bound on
    >= 99.99 % of the entries and the loose one on all."""
    from geometric_adv_amd import ops
    from conftest import cloud
    x1, x2 = cloud(11, 2, 2048), cloud(12, 2, 2048)
    want = oracle.approx_match(x1, x2)
    got = ops.approx_match(_t(x1), _t(x2), reference_weights=True).cpu().numpy().transpose(0, 2, 1)
    np.testing.assert_allclose(got, want, **REF_TOL)
    got = ops.approx_match(_t(x1), _t(x2)).cpu().numpy().transpose(0, 2, 1)
    strict = np.abs(got - want) <= 2e-6 + 2e-5 * np.abs(want)
    assert strict.mean() >= 0.9999, strict.mean()
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5)


def test_approx_match_is_a_transport_plan_full_size():
    """n = m = 2048: the plan's own properties (the oracle comparison at this size is the test above)."""
    import torch
    from geometric_adv_amd import ops
    from conftest import cloud
    x1, x2 = _t(cloud(3, 2, 2048)), _t(cloud(4, 2, 2048))
    match = ops.approx_match(x1, x2).double()
    assert (match >= 0).all()
    assert (match.sum(1) <= 1 + 1e-4).all() and (match.sum(2) <= 1 + 1e-4).all()
    torch.testing.assert_close(match.sum((1, 2)), torch.full((2,), 2048.0, dtype=torch.float64, device="cuda:0"), rtol=2e-2, atol=0)
    # identical clouds: the plan is (close to) the identity and the cost (close to) zero
    m2 = ops.approx_match(x1, x1)
    diag = torch.diagonal(m2, dim1=1, dim2=2)              # a few near-coincident pairs legitimately share mass
    assert (diag > 0.45).all() and diag.mean() > 0.99
    assert (ops.match_cost(x1, x1, m2) < 1e-2).all()


def test_match_cost_autograd_scales_by_upstream(golden_emd):
    import torch
    from geometric_adv_amd import ops
    g = golden_emd
    x1 = _t(g["a_xyz1"]).requires_grad_(True)
    x2 = _t(g["a_xyz2"]).requires_grad_(True)
    match = ops.approx_match(x1.detach(), x2.detach())
    cost = ops.match_cost_autograd(x1, x2, match)
    up = torch.tensor([2.0, -0.5], device="cuda:0")
    (cost * up).sum().backward()
    g1, g2 = ops.match_cost_grad(x1.detach(), x2.detach(), match)
    torch.testing.assert_close(x1.grad, g1 * up.view(-1, 1, 1))
    torch.testing.assert_close(x2.grad, g2 * up.view(-1, 1, 1))


def test_emd_argument_errors():
    import torch
    from geometric_adv_amd import ops
    x = torch.rand((2, 10, 3), device="cuda:0")
    with pytest.raises(ValueError):
        ops.match_cost(x, x, torch.rand((2, 10, 9), device="cuda:0"))
    with pytest.raises(ValueError):
        ops.approx_match(x, torch.rand((3, 10, 3), device="cuda:0"))
    from geometric_adv_amd import _lib
    out, temp = torch.empty((2, 10, 10), device="cuda:0"), torch.empty(4096, device="cuda:0")
    rc = _lib.lib().geoadv_approx_match_mode(7, 2, 10, 10, _lib.ptr(x), _lib.ptr(x), _lib.ptr(out), _lib.ptr(temp), None)
    assert rc != 0 and b"unknown weight mode" in _lib.lib().geoadv_last_error()


@pytest.mark.parametrize("reference_weights", [False, True])
@pytest.mark.parametrize("b,n,m", [(2, 2048, 2048), (3, 300, 517), (2, 64, 1100), (1, 1, 5)])
def test_fused_cost_grad1_equals_the_three_ops(b, n, m, reference_weights):
    """The attack loop's fused kernel (plan formed pair by pair in registers, never stored) against approx_match ->
    match_cost / match_cost_grad on the same clouds: same pair arithmetic, different order of the fp32 sums."""
    import torch
    from geometric_adv_amd import ops
    from conftest import cloud
    x1, x2 = _t(cloud(11, b, n)), _t(0.7 * cloud(12, b, m))
    match = ops.approx_match(x1, x2, reference_weights)
    want_cost = ops.match_cost(x1, x2, match)
    want_g1, _ = ops.match_cost_grad(x1, x2, match)
    cost, g1 = ops.emd_cost_grad1(x1, x2, reference_weights)
    torch.testing.assert_close(cost, want_cost, rtol=2e-6, atol=0)
    sc = want_g1.abs().amax((1, 2), keepdim=True)
    torch.testing.assert_close(g1 / sc, want_g1 / sc, rtol=0, atol=1e-5)          # 2048-term fp32 sums in a different order


@pytest.mark.parametrize("reference_weights", [False, True])
def test_fused_cost_grad1_with_coincident_and_nearly_coincident_points(reference_weights):
    """Pairs at distance 0 (the same point in both clouds, duplicated padding points) and at distances around 1e-19 .. 1e-16
    (denormal squared distances, the 1e-20 clamp of matchcostgrad_cpu :117): the fast mode's walk takes d and 1 / d from
    v_rsq_f32, which is no good there, and must fall back to the exact forms for the waves that meet such a pair."""
    import torch
    from geometric_adv_amd import ops
    from conftest import cloud
    rng = np.random.default_rng(77)
    b, n, m = 3, 1100, 900
    x1 = cloud(21, b, n).astype(np.float32)
    x2 = cloud(22, b, m).astype(np.float32)
    x2[0, :300] = x1[0, rng.permutation(n)[:300]]                   # exact copies
    x2[1, 50:60] = x2[1, 50]                                         # padding-style duplicates inside a cloud
    x1[1, 7] = x2[1, 50]
    x1[2, :40] *= 1e-20                                              # a knot of points within ~1e-20 .. 1e-19 of the origin
    x2[2, :40] = x1[2, :40][::-1] * np.float32(1.5)
    x2[2, 40:60] = rng.standard_normal((20, 3)).astype(np.float32) * np.float32(3e-17)
    t1, t2 = _t(x1), _t(x2)
    match = ops.approx_match(t1, t2, reference_weights)
    want_cost = ops.match_cost(t1, t2, match)
    want_g1, _ = ops.match_cost_grad(t1, t2, match)
    cost, g1 = ops.emd_cost_grad1(t1, t2, reference_weights)
    assert torch.isfinite(cost).all() and torch.isfinite(g1).all()
    torch.testing.assert_close(cost, want_cost, rtol=2e-6, atol=0)
    sc = want_g1.abs().amax((1, 2), keepdim=True)
    torch.testing.assert_close(g1 / sc, want_g1 / sc, rtol=0, atol=1e-5)


def test_approx_match_deterministic_and_order_free():
    """Two runs give the same bits (fixed-order folds, no atomics); permuting the clouds permutes the plan (sums run in a
    different order: 1e-5)."""
    import torch
    from geometric_adv_amd import ops
    from conftest import cloud
    x1, x2 = _t(cloud(21, 2, 700)), _t(cloud(22, 2, 900))
    a, b2 = ops.approx_match(x1, x2), ops.approx_match(x1, x2)
    assert torch.equal(a, b2)
    p1, p2 = torch.randperm(700, device="cuda:0"), torch.randperm(900, device="cuda:0")
    c = ops.approx_match(x1[:, p1], x2[:, p2])
    torch.testing.assert_close(c, a[:, p2][:, :, p1], rtol=1e-4, atol=2e-6)


def _sparse_state(x1, x2, reference_weights):
    """Which form the first levels of a default approx_match call take: [cloud pair][level] -> (use, heavy own points of cloud 1,
    of cloud 2), read by geoadv_debug_emd_sparse_state from the temp of a call made here, with temp of our own."""
    import ctypes as C
    import torch
    from geometric_adv_amd import _lib, ops
    lib = _lib.lib()
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    match = torch.empty((b, m, n), device="cuda:0")
    temp = torch.empty(int(lib.geoadv_approx_match_temp_floats(b, n, m)), device="cuda:0")
    rc = lib.geoadv_approx_match_mode(ops._emd_mode(reference_weights, False), b, n, m, _lib.ptr(x1), _lib.ptr(x2), _lib.ptr(match), _lib.ptr(temp), None)
    assert rc == 0, lib.geoadv_last_error()
    out = (C.c_int * (b * 3 * 3))()
    rc = lib.geoadv_debug_emd_sparse_state(0, b, n, m, _lib.ptr(temp), out, None)
    assert rc == 0, lib.geoadv_last_error()
    return np.ctypeslib.as_array(out).reshape(b, 3, 3).copy()


@pytest.mark.parametrize("reference_weights", [False, True])
@pytest.mark.parametrize("kind,b,n,m", [("uniform", 3, 2048, 2048), ("uniform", 2, 700, 1300), ("shell", 2, 1024, 2048),
                                         ("tiny_box", 2, 512, 512), ("flat", 2, 1024, 1024), ("far_apart", 2, 600, 600),
                                         ("blob_in_cube", 3, 2048, 2048), ("cube_in_blob", 2, 1500, 900)])
def test_sparse_levels_equal_dense_sweeps(kind, b, n, m, reference_weights):
    """Round 4: the first three levels' sweeps on a cell grid (weights exactly 0 beyond 0.04 / 0.08 / 0.16) against every sweep
    dense -- the same non-zero terms in another order of fp64 additions, so the plans agree to the conditioning of the
    algorithm on that order (the bound the reference mode is held to against the CPU op: 2 float ulps) and mostly bit for bit;
    cost and gradient of the fused form likewise.  Clouds: uniform cubes (different point counts), a sphere shell, a box so
    small that the device keeps the dense sweeps (nothing to thin out), a flat cloud (one degenerate axis), two clouds a
    whole box apart (no pair within reach at the first levels), and a Gaussian blob of width 0.02 inside a unit cube either way
    round (the attack's random-init reconstruction: the cube's points next to the blob are HEAVY -- thousands of candidates --
    and go through the dense form's workgroups inside the sparse launch; the blob's cells are fuller than the in-cell ranking
    handles)."""
    import torch
    from geometric_adv_amd import ops
    rng = np.random.default_rng(n + m)
    x1 = rng.random((b, n, 3)).astype(np.float32) - np.float32(0.5)
    x2 = rng.random((b, m, 3)).astype(np.float32) - np.float32(0.5)
    if kind == "shell":
        v = rng.standard_normal((b, n, 3)); x1 = (0.4 * v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float32)
        v = rng.standard_normal((b, m, 3)); x2 = (0.41 * v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float32)
    elif kind == "tiny_box":
        x1 *= np.float32(0.2); x2 *= np.float32(0.2)
    elif kind == "flat":
        x1[:, :, 2] = np.float32(0.1); x2[:, :, 2] = np.float32(0.1)
    elif kind == "far_apart":
        x2 += np.float32(1.5)
    elif kind == "blob_in_cube":
        x1 = (rng.standard_normal((b, n, 3)) * 0.022).astype(np.float32)
    elif kind == "cube_in_blob":
        x2 = (rng.standard_normal((b, m, 3)) * 0.022 + 0.1).astype(np.float32)
    out = {}
    for sparse in (False, True):
        ops.emd_sparse_levels(sparse)
        try:
            out[sparse] = (ops.approx_match(_t(x1), _t(x2), reference_weights),) + ops.emd_cost_grad1(_t(x1), _t(x2), reference_weights)
        finally:
            ops.emd_sparse_levels(True)
    md, cd, gd = out[False]
    ms, cs_, gs = out[True]
    # the forms that ran (decided on the device): without this, a device that kept every level dense would compare dense with dense
    state = _sparse_state(_t(x1), _t(x2), reference_weights)
    if kind == "tiny_box":
        assert (state[:, :, 0] == 0).all(), state.tolist()
    elif kind in ("uniform", "shell", "flat"):
        assert (state[:, :2, 0] == 1).all(), state.tolist()
    elif kind == "blob_in_cube":
        assert (state[:, 0, 0] == 1).all() and (state[:, 0, 2] > 0).all(), state.tolist()      # the cube (cloud 2) is the wide one
    elif kind == "cube_in_blob":
        assert (state[:, 0, 0] == 1).all() and (state[:, 0, 1] > 0).all(), state.tolist()      # ... cloud 1
    torch.testing.assert_close(ms, md, rtol=2e-6, atol=2e-8)
    torch.testing.assert_close(cs_, cd, rtol=1e-6, atol=0)
    torch.testing.assert_close(gs, gd, rtol=1e-5, atol=1e-7)
    if kind == "tiny_box":
        assert torch.equal(ms, md)                                      # the device kept the dense sweeps: the same launches
    again = ops.approx_match(_t(x1), _t(x2), reference_weights)         # reproducible run to run (stable binning order)
    assert torch.equal(again, ms)


def test_sparse_levels_equal_dense_sweeps_randomised():
    """Twelve random cloud pairs (n != m, anisotropic boxes from 0.05 to 4 wide, offsets, one cloud inside the other, clusters):
    whatever the device decides per level -- sparse or dense -- the plan, the cost and the gradient agree with the all-dense run
    to the order of fp64 additions."""
    import torch
    from geometric_adv_amd import ops
    rng = np.random.default_rng(77)
    for trial in range(12):
        b = int(rng.integers(1, 4)); n = int(rng.integers(40, 1500)); m = int(rng.integers(40, 1500))
        x1 = ((rng.random((b, n, 3)) - 0.5) * rng.uniform(0.05, 4.0, size=(b, 1, 3))).astype(np.float32)
        x2 = ((rng.random((b, m, 3)) - 0.5) * rng.uniform(0.05, 4.0, size=(b, 1, 3)) + rng.uniform(-0.5, 0.5, size=(b, 1, 3))).astype(np.float32)
        if trial % 3 == 0:
            x1[:, : n // 3] = (x1[:, : n // 3] * 0.05).astype(np.float32)
        out = {}
        for sparse in (False, True):
            ops.emd_sparse_levels(sparse)
            try:
                out[sparse] = (ops.approx_match(_t(x1), _t(x2)),) + ops.emd_cost_grad1(_t(x1), _t(x2))
            finally:
                ops.emd_sparse_levels(True)
        torch.testing.assert_close(out[True][0], out[False][0], rtol=2e-6, atol=2e-8, msg=lambda s: "trial %d: %s" % (trial, s))
        torch.testing.assert_close(out[True][1], out[False][1], rtol=1e-6, atol=0)
        torch.testing.assert_close(out[True][2], out[False][2], rtol=1e-5, atol=1e-7)
