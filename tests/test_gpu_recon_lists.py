"""GPU: ops.nn_distance_lists (csrc/chamfer_lists.hip: the attack loop's neighbour lists as an operator) against ops.nn_distance,
distance bits and indices, and against the numpy model of tests/_recon_lists_model.py.  B in {1, 3}; N in {65, 256, 1000, 2048}:
not a multiple of 64, one workgroup, ragged, full.  The C interface is called on guarded buffers once (tests/_guarded.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _chamfer_hard_clouds as HC  # noqa: E402
import _guarded as G  # noqa: E402
import _recon_lists_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(b, n) for n in (65, 256, 1000, 2048) for b in (1, 3)]


def _run(anchor, c, moved, skin, cap=16, model_clouds=1):
    """-> (state (certified, refused, unlisted), flags); asserts the four outputs against ops.nn_distance bit for bit and, for the
    first `model_clouds` clouds, against the numpy model."""
    import torch
    from geometric_adv_amd import ops
    ta, tc, tm = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (anchor, c, moved))
    d1a, _, d2a, _ = ops.nn_distance(ta, tc)
    got = ops.nn_distance_lists(ta, tc, d1a, d2a, skin, tm, cap)
    want = ops.nn_distance(tm, tc)
    for name, g, w in zip(("dist1", "idx1", "dist2", "idx2"), got[:4], want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), name
    state, flags = got[4].cpu().numpy(), got[5].cpu().numpy()
    b, n = anchor.shape[:2]
    assert state.sum() == 2 * b * n
    for u in range(min(b, model_clouds)):
        L = M.Lists(anchor[u], c[u], float(np.broadcast_to(skin, (b,))[u]), cap)
        m1, j1, m2, j2, info = M.query(L, moved[u])
        assert np.array_equal(j1, got[1][u].cpu().numpy()) and np.array_equal(j2, got[3][u].cpu().numpy())
        assert m1.tobytes() == got[0][u].cpu().numpy().tobytes() and m2.tobytes() == got[2][u].cpu().numpy().tobytes()
    return state, flags


@pytest.mark.parametrize("b,n", SHAPES)
def test_small_motion_is_certified_everywhere(b, n):
    """Motion 1e-4 at skin 1e-2: zero refused and zero unlisted queries -- the anchor's nearest partner is listed and still within
    sqrt(min) + 1e-4, and 17 partners inside a skin of 0.01 do not occur in uniform clouds of up to 2048 points."""
    a, c = M.uniform(100 + n, b, n), M.uniform(200 + n, b, n)
    state, flags = _run(a, c, M.moved_by(a, 300 + n, 1e-4), 1e-2)
    assert tuple(state) == (2 * b * n, 0, 0) and not flags.any()


@pytest.mark.parametrize("b,n", SHAPES)
def test_motion_beyond_the_skin_goes_through_brute_force(b, n):
    a, c = M.uniform(110 + n, b, n), M.uniform(210 + n, b, n)
    state, flags = _run(a, c, M.moved_by(a, 310 + n, 2.0), 1e-2)
    assert state[0] == 0 and flags.all()
    # one skin per cloud: cloud 0 far too small for its motion, the others generous
    if b > 1:
        skin = np.array([1e-5] + [2e-2] * (b - 1), np.float32)
        state, flags = _run(a, c, M.moved_by(a, 311 + n, 3e-3), skin)
        assert flags[0] == 1 and not flags[1:].any()


@pytest.mark.parametrize("b,n", SHAPES)
def test_duplicates_pick_the_lowest_index(b, n):
    a, c = M.duplicated(120 + n, b, n)
    _run(a, c, a.copy(), 2.0 ** -6)                                   # unmoved: exact ties inside the lists (and beyond their capacity)
    _run(a, c, a.copy(), 2.0 ** -6, cap=32)
    _run(a, c, M.moved_by(a, 320 + n, 2.0 ** -12), 2.0 ** -6)


@pytest.mark.parametrize("b,n", SHAPES)
def test_near_ties_of_the_hard_cloud_generators(b, n):
    for log2_rho, swapped in ((-6, False), (-12, True)):
        a, c = HC.shell_and_cluster(b, n, n, 130 + n, log2_rho, swapped)
        _run(a, c, M.moved_by(a, 330 + n, 1e-4), 1e-2)
        _run(a, c, M.moved_by(a, 331 + n, 2.0 ** (log2_rho - 2)), 2.0 ** log2_rho)
    a, c = HC.with_outlier("both", 6, b, n, n, 140 + n)
    _run(a, c, M.moved_by(a, 340 + n, 1e-4), 1e-2)
    a, c = HC.scaled("sphere", 3, b, n, n, 150 + n)
    _run(a, c, M.moved_by(a, 350 + n, 1e-3), 1e-1)


@pytest.mark.parametrize("n", [65, 256, 1000, 2048])
@pytest.mark.parametrize("which", ["closer", "equal", "farther"])
@pytest.mark.parametrize("low_index", [False, True])
def test_a_partner_just_outside_the_list(n, which, low_index):
    """tests/_recon_lists_model.boundary_case: a column just outside row 0's list, and a row just outside column 7's, end up one
    float32 step closer than, exactly as far as, one step farther than the list's best.  The certificate refuses both queries;
    the answers are nn_distance's (asserted by _run), i.e. the outside partner exactly when it is closer or ties with the lower index."""
    a, c, moved, skin, g = M.boundary_case(50, n, which, low_index)
    state, _ = _run(a[None], c[None], moved[None], skin)
    assert state[1] >= 2                                              # row 0 and column 7 are listed and refused


@pytest.mark.parametrize("b,n", SHAPES)
def test_a_dense_blob_overflows_the_far_columns_lists(b, n):
    a, c = M.blob_and_far_column(160 + n, b, n)
    state, flags = _run(a, c, M.moved_by(a, 360 + n, 1e-4), 1e-2)
    assert state[2] > b * n // 2 and flags.all()


@pytest.mark.parametrize("b,n", SHAPES)
def test_a_non_finite_coordinate_terminates_flags_and_stays_in_bounds(b, n):
    """The C entry point on guarded buffers: a NaN and an infinity in the moved rows.  Every query they touch is refused -- all
    columns of that cloud, the cloud's largest displacement being NaN -- the flag is raised, the indices stay in range and no
    byte outside the outputs changes."""
    import torch
    from geometric_adv_amd import _lib, ops
    a, c = M.uniform(170 + n, b, n), M.uniform(270 + n, b, n)
    moved = M.moved_by(a, 370 + n, 1e-4)
    moved[0, 7, 1] = np.nan
    moved[0, n - 1, 2] = np.inf
    d1a, _, d2a, _ = (t.cpu().numpy() for t in ops.nn_distance(torch.from_numpy(a).to(DEV), torch.from_numpy(c).to(DEV)))
    lib = _lib.lib()
    wb = int(lib.geoadv_nn_distance_lists_workspace_bytes(b, n, n, 16))
    bufs = dict(a=G.Buf((b, n, 3), np.float32, a), c=G.Buf((b, n, 3), np.float32, c), d1a=G.Buf((b, n), np.float32, d1a),
                d2a=G.Buf((b, n), np.float32, d2a), skin=G.Buf((b,), np.float32, np.full(b, 1e-2, np.float32)),
                moved=G.Buf((b, n, 3), np.float32, moved), d1=G.Buf((b, n), np.float32), i1=G.Buf((b, n), np.int32),
                d2=G.Buf((b, n), np.float32), i2=G.Buf((b, n), np.int32), state=G.Buf((4,), np.uint64), flags=G.Buf((b,), np.int32),
                ws=G.Buf((wb,), np.uint8))
    p = {k: v.ptr for k, v in bufs.items()}
    with torch.cuda.device(DEV):
        rc = lib.geoadv_nn_distance_lists(b, n, n, p["a"], p["c"], p["d1a"], p["d2a"], p["skin"], 16, p["moved"], p["d1"], p["i1"],
                                          p["d2"], p["i2"], p["state"], p["flags"], p["ws"], wb, _lib.stream_handle())
    _lib.check(rc, "nn_distance_lists")
    torch.cuda.synchronize()
    out = {k: bufs[k].get() for k in bufs}                            # (asserts every guard)
    assert out["flags"][0] == 1 and not out["flags"][1:].any()
    assert out["state"][:3].sum() == 2 * b * n and out["state"][1] >= n
    for k in ("i1", "i2"):
        assert (out[k] >= 0).all() and (out[k] < n).all()
    # the clouds without a non-finite coordinate, and the rows of cloud 0 that have none, are exact
    want = [t.cpu().numpy() for t in ops.nn_distance(torch.from_numpy(moved).to(DEV), torch.from_numpy(c).to(DEV))]
    ok = np.ones(n, bool)
    ok[[7, n - 1]] = False
    assert np.array_equal(out["i1"][0][ok], want[1][0][ok]) and out["d1"][0][ok].tobytes() == want[0][0][ok].tobytes()
    for u in range(1, b):
        for k, w in zip(("d1", "i1", "d2", "i2"), want):
            assert out[k][u].tobytes() == w[u].tobytes()
