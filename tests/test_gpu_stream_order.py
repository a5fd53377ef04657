"""GPU: every entry point of include/geoadv.h that takes a `void *stream` is held to that stream, and to "no host
synchronisation" unless the header says otherwise at its declaration, by the delayed-call protocol of tests/_stream_order.py
(its docstring states the protocol and why it is deterministic; DESIGN.md, 'The stream contract').

COVERED / EXEMPT: test_every_stream_taking_entry_point_has_a_case parses the header the way tests/test_abi.py does and
requires that the functions with a `void *stream` parameter are exactly the union of what the cases below cover and EXEMPT.
A new entry point fails the suite until it has a case.

The two controls prove that the protocol can fail: the null stream does not wait for a side stream on this runtime, the
delay is still pending when the stray work runs, and the comparison sees the difference.

Shapes are the smallest at which a case runs every launch of its path; each builder names the path from the dispatch code.
Stateless operators are called through the C ABI on buffers the case owns (outputs and caller-owned scratch are the same
memory in every step, so what a stray launch finds there is derived from input A); model handles go through their Python
wrappers (the wrapper's stream handle and its torch allocations are under test too, the handle's grow-only workspace is the
stale scratch); trainers and the attack go through their wrappers where those do not synchronise and through the C entry
point where they do (train_step's .item(), .cpu() and host degree checks).
"""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

# Entry points with a `void *stream` for which the protocol is meaningless, each with its reason.
EXEMPT = {}

# The header sentences that excuse an entry point from "the delay is still pending when the call returns".
SYNC_AE_STATUS = "Synchronises `stream`; GEOADV_ERANGE (message in geoadv_last_error; the flag is cleared)"
SYNC_ATTACK_STATUS = "synchronises the stream and returns GEOADV_EHIP"
SYNC_SEARCH_STATE = "Synchronises the stream."
SYNC_EMD_STATE = "Synchronises the stream."
SYNC_EXPORT = "Synchronises `stream` and downloads the current variables"

CASES = {}      # name -> (builder, the entry points it covers, stateful, the excusing header sentence or None)


def case(name, covers, stateful=False, blocks=None):
    def register(build):
        assert name not in CASES
        CASES[name] = (build, tuple(covers), stateful, blocks)
        return build
    return register


# ---- small helpers ---------------------------------------------------------------------------------------------------------------
def L():
    from geometric_adv_amd import _lib
    return _lib.lib()


def P(t):
    from geometric_adv_amd import _lib
    return _lib.ptr(t)


def SH():
    from geometric_adv_amd import _lib
    return _lib.stream_handle()


def ok(status, what):
    from geometric_adv_amd import _lib
    _lib.check(status, what)


def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def clouds(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3)) - 0.5).astype(np.float32)


def normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def feed(a, b):
    """(buffer, A, B) of one input: the buffer starts as A."""
    ta, tb = T(a), T(b)
    return (ta.clone(), ta, tb)


def zf(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.float32, device=DEV)


def zi(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.int32, device=DEV)


def zd(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.float64, device=DEV)


def zs(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.int16, device=DEV)


def zbytes(count):
    import torch
    return torch.zeros((int(count),), dtype=torch.uint8, device=DEV)


def in_device(fn, *args):
    import torch
    with torch.cuda.device(DEV):
        return fn(*args)


# ---- structural losses -----------------------------------------------------------------------------------------------------------
NN = (3, 130, 257)


@case("nn_distance", ["geoadv_nn_distance"])
def _nn_distance():
    """launch_chamfer_scans (both scans in one chamfer_scan_kernel<1, 16> launch: fewer workgroups than the chip holds), then
    nn_nonfinite_redo_kernel."""
    b, n, m = NN
    x1, x2 = feed(clouds(1, b, n), clouds(2, b, n)), feed(clouds(3, b, m), clouds(4, b, m))
    d1, i1, d2, i2 = zf(b, n), zi(b, n), zf(b, m), zi(b, m)

    def call():
        ok(in_device(L().geoadv_nn_distance, b, n, P(x1[0]), m, P(x2[0]), P(d1), P(i1), P(d2), P(i2), SH()), "nn_distance")
        return d1, i1, d2, i2
    return SO.Rig([x1, x2], call)


def _sym_rig(b, n, m, screen):
    x1, x2 = feed(clouds(5, b, n), clouds(6, b, n)), feed(clouds(7, b, m), clouds(8, b, m))
    d1, i1, d2, i2 = zf(b, n), zi(b, n), zf(b, m), zi(b, m)
    wf = int(L().geoadv_nn_distance_sym_workspace_floats(b, n, m))
    ws = zf(wf)

    def call():
        previous = L().geoadv_set_chamfer_screen(1 if screen else 0)
        try:
            ok(in_device(L().geoadv_nn_distance_sym, b, n, P(x1[0]), m, P(x2[0]), P(d1), P(i1), P(d2), P(i2), P(ws), wf, SH()),
               "nn_distance_sym")
        finally:
            L().geoadv_set_chamfer_screen(previous)
        return d1, i1, d2, i2
    return SO.Rig([x1, x2], call, keep=ws)


def _sym_rows(b, n, m, screen):
    """GEOADV_PLAN_ROWS_* of the operator's launch (geoadv_debug_chamfer_sym_plan: host only)."""
    req = (C.c_int * 16)(1, b, n, m, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1 if screen else 0)
    out = (C.c_int * 27)()
    ok(L().geoadv_debug_chamfer_sym_plan(req, out), "debug_chamfer_sym_plan")
    return out[0], out[9]                                   # GEOADV_SYM_OUT_SCREENED, GEOADV_SYM_OUT_ROWS


@case("nn_distance_sym_merge", ["geoadv_nn_distance_sym"])
def _nn_sym():
    """sym_shape: n <= 256 gives one row-wave and eight column-waves, so every row has 8 partials and the operator (which defers
    nothing) takes GEOADV_PLAN_ROWS_MERGE_LAUNCH: chamfer_sym_kernel, chamfer_sym_merge_kernel, nn_nonfinite_redo_kernel."""
    b, n, m = NN
    assert _sym_rows(b, n, m, True) == (0, 3) and L().geoadv_nn_distance_sym_is_screened(b, n, m) == 0
    return _sym_rig(b, n, m, True)


SCREENED = (32, 1025, 1800)    # sym_shape: n > 1024 and ceil(n / 2048) * ceil(m / 256) * b = 1 * 8 * 32 >= 256 CUs


@case("nn_distance_sym_screened", ["geoadv_nn_distance_sym"])
def _nn_sym_screened():
    """The smallest batch of 1025-point clouds that is_screened accepts: chamfer_mx_kernel<8>, the merge launch over its
    column slices, nn_nonfinite_redo_kernel."""
    assert L().geoadv_nn_distance_sym_is_screened(*SCREENED) == 1 and _sym_rows(*SCREENED, True) == (1, 3)
    return _sym_rig(*SCREENED, True)


@case("nn_distance_sym_screen_off", ["geoadv_nn_distance_sym"])
def _nn_sym_unscreened():
    """The same shape with the screen switched off for the call: chamfer_sym_kernel with eight row-waves, the merge launch."""
    assert _sym_rows(*SCREENED, False) == (0, 3)
    return _sym_rig(*SCREENED, False)


@case("chamfer_per_pc", ["geoadv_chamfer_per_pc"])
def _chamfer_per_pc():
    """One launch of chamfer_per_pc_kernel, a workgroup per cloud."""
    b, n, m = NN
    d1, d2 = feed(np.abs(normal(9, b, n)), np.abs(normal(10, b, n))), feed(np.abs(normal(11, b, m)), np.abs(normal(12, b, m)))
    out = zf(b)

    def call():
        ok(in_device(L().geoadv_chamfer_per_pc, b, n, m, P(d1[0]), P(d2[0]), P(out), SH()), "chamfer_per_pc")
        return (out,)
    return SO.Rig([d1, d2], call)


@case("nn_distance_paired", ["geoadv_nn_distance_paired"])
def _nn_paired():
    """launch_chamfer_grid (chamfer_grid_kernel<GR_MAX_N>, both directions, GR_QSPLIT slices), nn_nonfinite_redo_kernel.  The
    clouds are paired like the attack's: xyz1 = xyz2 + a small perturbation."""
    b, n = 3, 257
    base_a, base_b = clouds(13, b, n), clouds(14, b, n)
    x1 = feed(base_a + 0.01 * normal(15, b, n, 3), base_b + 0.01 * normal(16, b, n, 3))
    x2 = feed(base_a, base_b)
    d1, i1, d2, i2 = zf(b, n), zi(b, n), zf(b, n), zi(b, n)

    def call():
        ok(in_device(L().geoadv_nn_distance_paired, b, n, P(x1[0]), P(x2[0]), P(d1), P(i1), P(d2), P(i2), SH()), "nn_distance_paired")
        return d1, i1, d2, i2
    return SO.Rig([x1, x2], call)


@case("nn_distance_grad", ["geoadv_nn_distance_grad"])
def _nn_grad():
    """launch_chamfer_grad: one chamfer_grad_kernel launch, (cloud, side) per workgroup.  The match indices of A and B are the
    nn_distance matches of their own clouds (valid indices either way)."""
    from geometric_adv_amd import ops
    b, n, m = NN
    a1, a2, b1, b2 = clouds(17, b, n), clouds(18, b, m), clouds(19, b, n), clouds(20, b, m)
    _, ia1, _, ia2 = ops.nn_distance(T(a1), T(a2), kernel="scan")
    _, ib1, _, ib2 = ops.nn_distance(T(b1), T(b2), kernel="scan")
    feeds = [feed(a1, b1), feed(a2, b2), feed(normal(21, b, n), normal(22, b, n)), feed(normal(23, b, m), normal(24, b, m)),
             (ia1.clone(), ia1, ib1), (ia2.clone(), ia2, ib2)]
    g1, g2 = zf(b, n, 3), zf(b, m, 3)

    def call():
        x1, x2, gd1, gd2, i1, i2 = (f[0] for f in feeds)
        ok(in_device(L().geoadv_nn_distance_grad, b, n, P(x1), m, P(x2), P(gd1), P(i1), P(gd2), P(i2), P(g1), P(g2), SH()),
           "nn_distance_grad")
        return g1, g2
    return SO.Rig(feeds, call)


@case("chamfer_matrix_chunked", ["geoadv_chamfer_matrix"])
def _chamfer_matrix():
    """geoadv_chamfer_matrix's chunk loop: the workspace holds 5 of the 12 pairs (matrix_floats), so `cnt_ * 7 / 8` shrinks the
    first chunk and the loop runs three times, each a symmetric scan (merge launch) and chamfer_pair_mean_kernel."""
    na, nb, n, m = 3, 4, 130, 257
    A, B = feed(clouds(25, na, n), clouds(26, na, n)), feed(clouds(27, nb, m), clouds(28, nb, m))
    full = int(L().geoadv_chamfer_matrix_workspace_floats(na, nb, n, m))
    one = int(L().geoadv_chamfer_matrix_workspace_floats(1, 1, n, m))
    wf = one + (full - one) * 4 // 11
    assert one < wf < full
    ws, out = zf(wf), zf(na, nb)

    def call():
        ok(in_device(L().geoadv_chamfer_matrix, na, nb, n, m, P(A[0]), P(B[0]), P(out), P(ws), wf, SH()), "chamfer_matrix")
        return (out,)
    return SO.Rig([A, B], call, keep=ws)


# ---- EMD -------------------------------------------------------------------------------------------------------------------------
# Every size runs all 11 levels (emd_run_levels): emd_init_kernel, the binning kernel of the sparse first three levels (when the
# call does not carry GEOADV_EMD_DENSE_LEVELS), the sweeps of every level, emd_level0_kernel and the closing kernel.  300 x 257
# points span more than one 256-thread block in both directions.
EMD = (2, 300, 257)


def _emd_clouds():
    b, n, m = EMD
    return feed(clouds(29, b, n), clouds(30, b, n)), feed(clouds(31, b, m), clouds(32, b, m))


def _approx_match_rig(mode):
    b, n, m = EMD
    x1, x2 = _emd_clouds()
    match, temp = zf(b, m, n), zf(int(L().geoadv_approx_match_temp_floats(b, n, m)))

    def call():
        if mode is None:
            st = in_device(L().geoadv_approx_match, b, n, m, P(x1[0]), P(x2[0]), P(match), P(temp), SH())
        else:
            st = in_device(L().geoadv_approx_match_mode, mode, b, n, m, P(x1[0]), P(x2[0]), P(match), P(temp), SH())
        ok(st, "approx_match")
        return (match,)
    return SO.Rig([x1, x2], call, keep=temp)


@case("approx_match", ["geoadv_approx_match"])
def _approx_match():
    """The FAST mode with the process default of sparse first levels: emd_sparse_bin_kernel<2>, sparse and dense sweeps,
    emd_match_kernel."""
    return _approx_match_rig(None)


@case("approx_match_mode_reference_sparse", ["geoadv_approx_match_mode"])
def _approx_match_ref():
    return _approx_match_rig(1)


@case("approx_match_mode_dense", ["geoadv_approx_match_mode"])
def _approx_match_dense():
    """GEOADV_EMD_DENSE_LEVELS: no binning launch, every sweep dense."""
    return _approx_match_rig(0x100)


def _plan(seed_pair):
    from geometric_adv_amd import ops
    b, n, m = EMD
    return ops.approx_match(T(clouds(seed_pair[0], b, n)), T(clouds(seed_pair[1], b, m)))


def _match_cost_rig(workspace):
    b, n, m = EMD
    x1, x2 = _emd_clouds()
    ma, mb = _plan((29, 31)), _plan((30, 32))
    match = (ma.clone(), ma, mb)
    out = zf(b)
    wf = int(L().geoadv_match_cost_workspace_floats(b, n, m))
    ws = zf(wf)

    def call():
        if workspace:
            st = in_device(L().geoadv_match_cost_ws, b, n, m, P(x1[0]), P(x2[0]), P(match[0]), P(out), P(ws), wf, SH())
        else:
            st = in_device(L().geoadv_match_cost, b, n, m, P(x1[0]), P(x2[0]), P(match[0]), P(out), SH())
        ok(st, "match_cost")
        return (out,)
    return SO.Rig([x1, x2, match], call, keep=ws)


@case("match_cost", ["geoadv_match_cost"])
def _match_cost():
    """hipMallocAsync on the stream, emd_cost_partial_kernel, emd_cost_fold_kernel, hipFreeAsync."""
    return _match_cost_rig(False)


@case("match_cost_ws", ["geoadv_match_cost_ws"])
def _match_cost_ws():
    return _match_cost_rig(True)


@case("match_cost_grad", ["geoadv_match_cost_grad"])
def _match_cost_grad():
    """emd_grad1_kernel and, with grad2 asked for, emd_grad2_kernel."""
    b, n, m = EMD
    x1, x2 = _emd_clouds()
    ma, mb = _plan((29, 31)), _plan((30, 32))
    match = (ma.clone(), ma, mb)
    g1, g2 = zf(b, n, 3), zf(b, m, 3)

    def call():
        ok(in_device(L().geoadv_match_cost_grad, b, n, m, P(x1[0]), P(x2[0]), P(match[0]), P(g1), P(g2), SH()), "match_cost_grad")
        return g1, g2
    return SO.Rig([x1, x2, match], call)


def _cost_grad1_rig(mode):
    b, n, m = EMD
    x1, x2 = _emd_clouds()
    cost, g1, temp = zf(b), zf(b, n, 3), zf(int(L().geoadv_emd_cost_grad1_temp_floats(b, n, m)))

    def call():
        if mode is None:
            st = in_device(L().geoadv_emd_cost_grad1, b, n, m, P(x1[0]), P(x2[0]), P(cost), P(g1), P(temp), SH())
        else:
            st = in_device(L().geoadv_emd_cost_grad1_mode, mode, b, n, m, P(x1[0]), P(x2[0]), P(cost), P(g1), P(temp), SH())
        ok(st, "emd_cost_grad1")
        return cost, g1
    return SO.Rig([x1, x2], call, keep=temp)


@case("emd_cost_grad1", ["geoadv_emd_cost_grad1"])
def _cost_grad1():
    """The levels as above, then emd_plan_cost_grad1_kernel and emd_cost_fold_kernel."""
    return _cost_grad1_rig(None)


@case("emd_cost_grad1_mode_dense", ["geoadv_emd_cost_grad1_mode"])
def _cost_grad1_dense():
    return _cost_grad1_rig(0x100)


@case("emd_cost_grad1_mode_reference_sparse", ["geoadv_emd_cost_grad1_mode"])
def _cost_grad1_ref():
    return _cost_grad1_rig(1)


@case("debug_emd_sparse_state", ["geoadv_approx_match_mode", "geoadv_debug_emd_sparse_state"], blocks=SYNC_EMD_STATE)
def _emd_sparse_state():
    """approx_match_mode with sparse levels, then the reader of its scratch on the same stream: it synchronises (the header
    says so) and must see the scratch of THAT call."""
    b, n, m = EMD
    x1, x2 = _emd_clouds()
    match, temp = zf(b, m, n), zf(int(L().geoadv_approx_match_temp_floats(b, n, m)))

    def call():
        ok(in_device(L().geoadv_approx_match_mode, 0, b, n, m, P(x1[0]), P(x2[0]), P(match), P(temp), SH()), "approx_match_mode")
        out = (C.c_int * (b * 3 * 3))()
        ok(in_device(L().geoadv_debug_emd_sparse_state, 0, b, n, m, P(temp), out, SH()), "debug_emd_sparse_state")
        return match, np.array(list(out), np.int32)
    return SO.Rig([x1, x2], call, keep=temp)


# ---- grouping --------------------------------------------------------------------------------------------------------------------
GRP = (2, 130, 70)          # b, dataset points, queries: two blocks of queries per cloud in every kernel


def _grp_clouds(seed):
    b, n, m = GRP
    return feed(clouds(seed, b, n), clouds(seed + 1, b, n)), feed(clouds(seed + 2, b, m), clouds(seed + 3, b, m))


@case("query_ball_point", ["geoadv_query_ball_point"])
def _query_ball():
    """One launch of query_ball_fast_kernel."""
    b, n, m = GRP
    x1, x2 = _grp_clouds(40)
    idx, cnt = zi(b, m, 8), zi(b, m)

    def call():
        ok(in_device(L().geoadv_query_ball_point, b, n, m, 0.3, 8, P(x1[0]), P(x2[0]), P(idx), P(cnt), SH()), "query_ball_point")
        return idx, cnt
    return SO.Rig([x1, x2], call)


@case("selection_sort", ["geoadv_selection_sort"])
def _selection_sort():
    """One launch of selection_sort_kernel, a wave per row."""
    b, n, m = GRP
    dist = feed(np.abs(normal(44, b, m, n)), np.abs(normal(45, b, m, n)))
    outi, out = zi(b, m, n), zf(b, m, n)

    def call():
        ok(in_device(L().geoadv_selection_sort, b, n, m, 9, P(dist[0]), P(outi), P(out), SH()), "selection_sort")
        return outi, out
    return SO.Rig([dist], call)


def _group_idx(seed, b, n, m, ns):
    return np.random.default_rng(seed).integers(0, n, (b, m, ns)).astype(np.int32)


@case("group_point", ["geoadv_group_point"])
def _group_point():
    """One launch of group_point_kernel."""
    b, n, m = GRP
    pts, idx = feed(normal(46, b, n, 5), normal(47, b, n, 5)), feed(_group_idx(48, b, n, m, 6), _group_idx(49, b, n, m, 6))
    out = zf(b, m, 6, 5)

    def call():
        ok(in_device(L().geoadv_group_point, b, n, 5, m, 6, P(pts[0]), P(idx[0]), P(out), SH()), "group_point")
        return (out,)
    return SO.Rig([pts, idx], call)


def _gpg_rig(workspace):
    """gpg_shape: n = 130 >= 64 needs two 6-bit radix passes (the first shape of test_gpu_op_limits' destination test has two as
    well), each gpg_pass_kernel<false>, gpg_scan_kernel, gpg_pass_kernel<true>; then gpg_bounds_kernel and gpg_sum_kernel."""
    b, n, m = GRP
    c, ns = 5, 9
    go, idx = feed(normal(50, b, m, ns, c), normal(51, b, m, ns, c)), feed(_group_idx(52, b, n, m, ns), _group_idx(53, b, n, m, ns))
    gp = zf(b, n, c)
    wb = int(L().geoadv_group_point_grad_workspace_bytes(b, n, c, m, ns))
    ws = zbytes(wb)

    def call():
        if workspace:
            st = in_device(L().geoadv_group_point_grad_ws, b, n, c, m, ns, P(go[0]), P(idx[0]), P(gp), P(ws), wb, SH())
        else:
            st = in_device(L().geoadv_group_point_grad, b, n, c, m, ns, P(go[0]), P(idx[0]), P(gp), SH())
        ok(st, "group_point_grad")
        return (gp,)
    return SO.Rig([go, idx], call, keep=ws)


@case("group_point_grad", ["geoadv_group_point_grad"])
def _gpg():
    return _gpg_rig(False)


@case("group_point_grad_ws", ["geoadv_group_point_grad_ws"])
def _gpg_ws():
    return _gpg_rig(True)


def _knn_point_rig(kernel, k, workspace=True):
    b, n, m = GRP
    x1, x2 = _grp_clouds(54)
    val, idx = zf(b, m, k), zi(b, m, k)
    wb = int(L().geoadv_knn_workspace_bytes(b, n, m, k))
    ws = zbytes(wb)

    def call():
        if workspace:
            st = in_device(L().geoadv_knn_point_ws, kernel, b, n, m, k, P(x1[0]), P(x2[0]), P(val), P(idx), P(ws), wb, SH())
        else:
            st = in_device(L().geoadv_knn_point, b, n, m, k, P(x1[0]), P(x2[0]), P(val), P(idx), SH())
        ok(st, "knn_point")
        return val, idx
    return SO.Rig([x1, x2], call, keep=ws)


def _knn_dists_rig(kernel, k, workspace=True):
    b, n, _ = GRP
    pc = feed(clouds(58, b, n), clouds(59, b, n))
    out = zf(b, n, k)
    wb = int(L().geoadv_knn_workspace_bytes(b, n, n, k + 1))
    ws = zbytes(wb)

    def call():
        if workspace:
            st = in_device(L().geoadv_knn_dists_ws, kernel, b, n, k, P(pc[0]), P(out), P(ws), wb, SH())
        else:
            st = in_device(L().geoadv_knn_dists, b, n, k, P(pc[0]), P(out), SH())
        ok(st, "knn_dists")
        return (out,)
    return SO.Rig([pc], call, keep=ws)


# launch_knn / launch_knn_fast: the register-list kernels for k (+ 1) <= 17 -- GEOADV_KNN_ALL_POINTS: a memset of the redo counter,
# knn_fast_kernel, knn_redo_kernel; GEOADV_KNN_GRID / _GRID_SHELLS (the grid at every n <= 4096): knn_grid_build_kernel, knn_grid_kernel
# (keyed / lane-first, or the shell walk alone), knn_redo_kernel -- and for longer lists the generic knn_kernel, a wave per query.
for _name, _kern, _k in (("all_points", 1, 5), ("grid", 2, 5), ("grid_shells", 3, 5), ("generic", 0, 20)):
    case("knn_point_ws_" + _name, ["geoadv_knn_point_ws"])(functools.partial(_knn_point_rig, _kern, _k))
    case("knn_dists_ws_" + _name, ["geoadv_knn_dists_ws"])(functools.partial(_knn_dists_rig, _kern, _k))
# the reference-shaped forms: stream-ordered scratch (hipMallocAsync / hipFreeAsync on the stream), the process default (by size:
# the all-points kernel at 130 points)
case("knn_point", ["geoadv_knn_point"])(functools.partial(_knn_point_rig, 0, 5, False))
case("knn_dists", ["geoadv_knn_dists"])(functools.partial(_knn_dists_rig, 0, 5, False))


def _fps_rig(form):
    b, n, m = 5, 130, 20            # five clouds: the wave form packs four per workgroup, so two workgroups
    xyz = feed(clouds(60, b, n), clouds(61, b, n))
    start = feed(np.array([0, 3, 129, 7, 64], np.int32), np.array([5, 0, 1, 100, 2], np.int32))
    idx, sampled, mind = zi(b, m), zf(b, m, 3), zf(b, n)

    def call():
        ok(in_device(L().geoadv_farthest_point_sample, b, n, P(xyz[0]), m, P(start[0]), form, P(idx), P(sampled), P(mind), SH()),
           "farthest_point_sample")
        return idx, sampled, mind
    return SO.Rig([xyz, start], call)


# geoadv_farthest_point_sample: one launch either way -- AUTO at n <= 256 is fps_kernel's wave-per-cloud instance, WORKGROUP its
# workgroup-per-cloud instance
case("farthest_point_sample_wave", ["geoadv_farthest_point_sample"])(functools.partial(_fps_rig, 0))
case("farthest_point_sample_workgroup", ["geoadv_farthest_point_sample"])(functools.partial(_fps_rig, 1))


# ---- defenses --------------------------------------------------------------------------------------------------------------------
DEF = (3, 300)              # one 1024-thread workgroup per cloud in every kernel; 300 points are no multiple of anything


def _def_inputs(seed, k):
    b, n = DEF
    return feed(clouds(seed, b, n), clouds(seed + 1, b, n)), feed(np.abs(normal(seed + 2, b, n, k)), np.abs(normal(seed + 3, b, n, k)))


@case("outlier_filter", ["geoadv_outlier_filter"])
def _outlier_filter():
    """One launch of outlier_filter_kernel."""
    b, n = DEF
    pc, kd = _def_inputs(62, 4)
    o_pc, o_idx, o_num, inl = zf(b, n, 3), zs(b, n), zs(b), zf(b, n, 3)

    def call():
        ok(in_device(L().geoadv_outlier_filter, b, n, P(pc[0]), P(kd[0]), 4, 3, 0.7, P(o_pc), P(o_idx), P(o_num), P(inl), SH()),
           "outlier_filter")
        return o_pc, o_idx, o_num, inl
    return SO.Rig([pc, kd], call)


@case("sor_filter", ["geoadv_sor_filter"])
def _sor_filter():
    """One launch of sor_filter_kernel."""
    b, n = DEF
    pc, kd = _def_inputs(66, 4)
    o_pc, o_idx, o_num, inl, stats = zf(b, n, 3), zs(b, n), zs(b), zf(b, n, 3), zd(b, 3)

    def call():
        ok(in_device(L().geoadv_sor_filter, b, n, P(pc[0]), P(kd[0]), 4, 2, 1.1, P(o_pc), P(o_idx), P(o_num), P(inl), P(stats), SH()),
           "sor_filter")
        return o_pc, o_idx, o_num, inl, stats
    return SO.Rig([pc, kd], call)


@case("random_drop", ["geoadv_random_drop"])
def _random_drop():
    """One launch of random_drop_kernel."""
    b, n = DEF
    pc = feed(clouds(70, b, n), clouds(71, b, n))
    kept, dropped = zf(b, n, 3), zi(b, 37)

    def call():
        ok(in_device(L().geoadv_random_drop, b, n, P(pc[0]), 37, 12345, 7, 2, P(kept), P(dropped), SH()), "random_drop")
        return kept, dropped
    return SO.Rig([pc], call)


@case("critical_split", ["geoadv_critical_split"])
def _critical_split():
    """One launch of critical_split_kernel.  max_idx of A and B are valid point indices."""
    b, n = DEF
    c = 128
    rng = np.random.default_rng(72)
    pc = feed(clouds(73, b, n), clouds(74, b, n))
    mv = feed(normal(75, b, c), normal(76, b, c))
    mi = feed(rng.integers(0, n, (b, c)).astype(np.int32), rng.integers(0, n, (b, c)).astype(np.int32))
    outs = (zf(b, c, 3), zs(b, c), zs(b), zf(b, n, 3), zf(b, n, 3))

    def call():
        ok(in_device(L().geoadv_critical_split, b, n, c, P(pc[0]), P(mv[0]), P(mi[0]), *[P(o) for o in outs], SH()), "critical_split")
        return outs
    return SO.Rig([pc, mv, mi], call)


def _knn_loss_rig(debug_launch):
    """geoadv_knn_outlier_loss: the search (launch_knn's all-points list kernels at 300 points: memset, knn_fast_kernel,
    knn_redo_kernel) and the loss launch; the debug entry point is that last launch alone on the neighbours the full call left
    in the workspace."""
    b, n = DEF
    k = 5
    pc = feed(clouds(77, b, n), clouds(78, b, n))
    loss, grad, score, mask, idx, stats = zd(b), zf(b, n, 3), zd(b, n), zbytes(b * n), zi(b, n, k), zd(b, 4)
    wb = int(L().geoadv_knn_outlier_loss_workspace_bytes(b, n, k))
    ws = zbytes(wb)
    loss2, grad2 = zd(b), zf(b, n, 3)

    def call():
        ok(in_device(L().geoadv_knn_outlier_loss, 0, b, n, k, 1.05, P(pc[0]), P(loss), P(grad), P(score), P(mask), P(idx), P(stats),
                     P(ws), wb, SH()), "knn_outlier_loss")
        if not debug_launch:
            return loss, grad, score, mask, idx, stats
        ok(in_device(L().geoadv_debug_knn_outlier_loss_launch, b, n, k, 1.05, P(pc[0]), P(loss2), P(grad2), P(ws), wb, SH()),
           "debug_knn_outlier_loss_launch")
        return loss, grad, loss2, grad2
    return SO.Rig([pc], call, keep=ws)


case("knn_outlier_loss", ["geoadv_knn_outlier_loss"])(functools.partial(_knn_loss_rig, False))
case("debug_knn_outlier_loss_launch", ["geoadv_knn_outlier_loss", "geoadv_debug_knn_outlier_loss_launch"])(
    functools.partial(_knn_loss_rig, True))


# ---- data ------------------------------------------------------------------------------------------------------------------------
@case("sort_axes", ["geoadv_sort_axes"])
def _sort_axes():
    """One launch of sort_axes_kernel."""
    b, n = DEF
    stretch = np.array([1.0, 2.0, 1.0], np.float32)
    pc = feed(clouds(79, b, n), clouds(80, b, n) * stretch)
    out, axes = zf(b, n, 3), zi(b, 3)

    def call():
        ok(in_device(L().geoadv_sort_axes, b, n, P(pc[0]), P(out), P(axes), 1, SH()), "sort_axes")
        return out, axes
    return SO.Rig([pc], call)


def _rotations(seed, count):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((count, 3, 3)))
    return np.ascontiguousarray(q, np.float64)


@case("batch_gather_noise_rotation", ["geoadv_batch_gather"])
def _batch_gather():
    """One launch of the gather kernel with noise and one rotation per cloud.  A and B differ in the resident clouds, the index
    (valid rows either way) and the rotations."""
    from geometric_adv_amd import _abi
    clouds_n, b, n = 7, 4, 300
    data = feed(clouds(81, clouds_n, n), clouds(82, clouds_n, n))
    index = feed(np.array([6, 0, 3, 3], np.int32), np.array([1, 5, 2, 0], np.int32))
    rot = feed(_rotations(83, b), _rotations(84, b))
    aug = _abi.BatchAugment(seed=9, counter=4, slot_offset=8, noise_mu=0.0, noise_sigma=0.02, noise_clip=0.05, rot_count=b, rotate_first=0)
    clean, fed = zf(b, n, 3), zf(b, n, 3)

    def call():
        ok(in_device(L().geoadv_batch_gather, b, n, P(data[0]), clouds_n, P(index[0]), C.byref(aug), P(rot[0]), P(clean), P(fed), SH()),
           "batch_gather")
        return clean, fed
    return SO.Rig([data, index, rot], call, keep=aug)


def _normalize_rig(kind):
    b, n = DEF
    pc = feed(clouds(85, b, n), clouds(86, b, n) * 3.0 + 1.0)
    out = zf(b, n, 3)

    def call():
        ok(in_device(L().geoadv_normalize_clouds, b, n, kind, P(pc[0]), P(out), SH()), "normalize_clouds")
        return (out,)
    return SO.Rig([pc], call)


# one launch of normalize_clouds_kernel; the two kinds with statistics
case("normalize_clouds_unit_ball", ["geoadv_normalize_clouds"])(functools.partial(_normalize_rig, 1))
case("normalize_clouds_bounding_box", ["geoadv_normalize_clouds"])(functools.partial(_normalize_rig, 2))


@case("augment_batch", ["geoadv_augment_batch"])
def _augment_batch():
    """One launch: gather, re-sampling to 200 of 300 points, every operator of the Augmenter drawn on the device."""
    from geometric_adv_amd import _abi
    clouds_n, b, n_src, n_out = 7, 4, 300, 200
    data = feed(clouds(87, clouds_n, n_src), clouds(88, clouds_n, n_src))
    index = feed(np.array([6, 0, 3, 3], np.int32), np.array([1, 5, 2, 0], np.int32))
    cfg = _abi.CloudAugment(seed=5, counter=3, slot_offset=2, sample=1, rot_axes=7, range_rot=360.0, rot_3d=1, scale=1, scale_min=0.75,
                            scale_max=1.25, flip_axes=5, translate=1, translate_scale=0.03)
    out, params = zf(b, n_out, 3), zf(b, 45)

    def call():
        ok(in_device(L().geoadv_augment_batch, b, n_out, P(data[0]), clouds_n, n_src, P(index[0]), C.byref(cfg), None, P(params), P(out),
                     SH()), "augment_batch")
        return out, params
    return SO.Rig([data, index], call, keep=cfg)


@case("rotate_y", ["geoadv_rotate_y"])
def _rotate_y():
    """One launch of the rotation kernel."""
    b, n = DEF
    pc = feed(clouds(89, b, n), clouds(90, b, n))
    out = zf(b, n, 3)

    def call():
        ok(in_device(L().geoadv_rotate_y, b, n, P(pc[0]), float(np.cos(0.7)), float(np.sin(0.7)), P(out), SH()), "rotate_y")
        return (out,)
    return SO.Rig([pc], call)


@case("latent_dist_matrix", ["geoadv_latent_dist_matrix"])
def _latent_dist():
    """One launch of latent_dist_kernel over a 3 x 2 grid of tiles."""
    na, nb, d = 70, 40, 128
    a, b = feed(normal(91, na, d), normal(92, na, d)), feed(normal(93, nb, d), normal(94, nb, d))
    out = zf(na, nb)

    def call():
        ok(in_device(L().geoadv_latent_dist_matrix, na, nb, d, P(a[0]), P(b[0]), P(out), SH()), "latent_dist_matrix")
        return (out,)
    return SO.Rig([a, b], call)


@case("debug_h2_split", ["geoadv_debug_h2_split"])
def _h2_split():
    """One launch of h2_split_debug_kernel."""
    n = 300
    vals = feed(normal(95, 2 * n), normal(96, 2 * n))
    import torch
    w = [torch.zeros((n,), dtype=torch.int32, device=DEV) for _ in range(3)]

    def call():
        ok(in_device(L().geoadv_debug_h2_split, P(vals[0]), n, P(w[0]), P(w[1]), P(w[2]), SH()), "debug_h2_split")
        return w
    return SO.Rig([vals], call)


# ---- training-step kernels on their own --------------------------------------------------------------------------------------------
def _gemm_rig(kernel, M, N, K, batch):
    A, B = feed(normal(97, batch, M, K), normal(98, batch, M, K)), feed(normal(99, batch, K, N), normal(100, batch, K, N))
    bias = feed(normal(101, N), normal(102, N))
    Cm = zf(batch, M, N)
    nf = int(L().geoadv_train_gemm_partial_floats()) if kernel == 0 else 0
    part = zf(nf) if nf else None
    split = C.c_int(0)

    def call():
        ok(in_device(L().geoadv_train_gemm, kernel, P(A[0]), K, 1, M * K, P(B[0]), N, 1, K * N, P(Cm), N, M * N, P(bias[0]), 0, M, N, K,
                     batch, P(part), nf, C.byref(split), SH()), "train_gemm")
        return Cm, split.value
    return SO.Rig([A, B, bias], call, keep=part)


@case("train_gemm_splitk", ["geoadv_train_gemm"])
def _gemm_split():
    """Kernel 0 at 64 x 65 x 129: two blocks, K >= 128, so ct_ksplit gives a split of 2 -- ct_gemm_kernel into the partials and
    ct_splitk_reduce."""
    rig = _gemm_rig(0, 64, 65, 129, 1)
    inner = rig.call

    def call():
        out = inner()
        assert out[1] == 2, "the shape no longer splits its K range: %r" % (out[1],)
        return out
    rig.call = call
    return rig


@case("train_gemm_tile", ["geoadv_train_gemm"])
def _gemm_tile():
    """Kernel 1: one at_gemm_kernel launch, 129 x 130 over three groups (ragged 128-tiles)."""
    return _gemm_rig(1, 129, 130, 33, 3)


FOLD_POOL = (3, 63, 128)


@functools.lru_cache(maxsize=None)
def _pool_graph():
    import _fold_pool_model as PM
    b, n, c = FOLD_POOL
    adj = PM.build_adjacency(b, n, 401, True)
    cols = PM.build_cols(adj, 501)
    _, win = PM.pool(PM.pool_input("tied", b, n, c, 601), cols)
    return adj, cols, win


@case("fold_train_pool", ["geoadv_fold_train_pool"])
def _fold_pool():
    """One launch of ft_graph_pool_kernel.  A and B are two kinds of activations over two valid column sets."""
    import _fold_pool_model as PM
    b, n, c = FOLD_POOL
    adj, cols_a, _ = _pool_graph()
    h = feed(PM.pool_input("tied", b, n, c, 311), PM.pool_input("distinct", b, n, c, 312))
    cols = feed(cols_a, PM.build_cols(adj, 777))
    g, win = zf(b * n, c), zi(b * n, c)

    def call():
        ok(in_device(L().geoadv_fold_train_pool, b, n, c, P(h[0]), P(cols[0]), P(g), P(win), SH()), "fold_train_pool")
        return g, win
    return SO.Rig([h, cols], call)


@case("fold_train_pool_grad", ["geoadv_fold_train_pool_grad"])
def _fold_pool_grad():
    """One launch of ft_pool_bwd_kernel on a fixed adjacency and winners; A and B are two gradients."""
    import _fold_pool_model as PM
    b, n, c = FOLD_POOL
    adj, _, win = _pool_graph()
    off, deg, col = (T(a) for a in PM.csr(adj))
    col.clamp_(min=0)                                       # the unused tail of a row block: valid rows, never read
    wd = T(win.astype(np.int32))
    dg = feed(PM.grad_input("integer", b, n, c, 701), PM.grad_input("float", b, n, c, 801))
    dh = zf(b * n, c)

    def call():
        ok(in_device(L().geoadv_fold_train_pool_grad, b, n, c, P(dg[0]), P(wd), P(off), P(deg), P(col), P(dh), SH()), "fold_train_pool_grad")
        return (dh,)
    return SO.Rig([dg], call, keep=(off, deg, col, wd))


@case("fold_train_gmax", ["geoadv_fold_train_gmax"])
def _fold_gmax():
    """One launch of the global-maximum kernel over 70 rows (no multiple of its four row phases)."""
    import _fold_pool_model as PM
    b, n, c = 2, 70, 128
    a1, inv1, sh1 = PM.gmax_input(b, n, c, 901)
    a2, inv2, sh2 = PM.gmax_input(b, n, c, 902)
    feeds = [feed(a1, a2), feed(inv1, inv2), feed(sh1, sh2)]
    pooled, arg = zf(b, c), zi(b, c)

    def call():
        a, inv, sh = (f[0] for f in feeds)
        ok(in_device(L().geoadv_fold_train_gmax, b, n, c, P(a), P(inv), P(sh), P(pooled), P(arg), SH()), "fold_train_gmax")
        return pooled, arg
    return SO.Rig(feeds, call)


# ---- models (through their wrappers: the handle's grow-only workspace is the stale scratch) -----------------------------------------
AE_N = 256


@functools.lru_cache(maxsize=None)
def _ae_weights():
    from geometric_adv_amd import weights as W
    return W.synthetic_weights(AE_N, seed=3)


@functools.lru_cache(maxsize=None)
def _ae(arith):
    """None where the model does not admit the arithmetic (geoadv_ae_set_encoder_arith refuses it)."""
    from geometric_adv_amd.autoencoder import PointNetAE
    try:
        return PointNetAE(_ae_weights(), AE_N, encoder_arith=arith)
    except ValueError:
        return None


def _ae_forward_rig(arith):
    """run_forward: the encoder launch of the arithmetic, the decoder launches, the latent's copy."""
    ae = _ae(arith)
    pc = feed(clouds(110, 3, AE_N), clouds(111, 3, AE_N))

    def call():
        recon, latent = ae.forward(pc[0])
        return recon, latent
    return SO.Rig([pc], call, keep=ae)


ARITHS = ("f32", "bf16x3", "f16x2")
for _arith in ARITHS:
    case("ae_forward_" + _arith, ["geoadv_ae_forward"])(functools.partial(_ae_forward_rig, _arith))


@case("ae_critical", ["geoadv_ae_critical"])
def _ae_critical():
    """The encoder launch alone and the two copies out of the scratch."""
    ae = _ae("bf16x3")
    pc = feed(clouds(112, 3, AE_N), clouds(113, 3, AE_N))
    return SO.Rig([pc], lambda: ae.max_and_argmax(pc[0]), keep=ae)


@case("ae_decode", ["geoadv_ae_decode"])
def _ae_decode():
    """The decoder launches alone."""
    ae = _ae("bf16x3")
    z = feed(np.abs(normal(114, 3, 128)), np.abs(normal(115, 3, 128)))
    return SO.Rig([z], lambda: (ae.decode_tensor(z[0]),), keep=ae)


@case("ae_status", ["geoadv_ae_forward", "geoadv_ae_status"], blocks=SYNC_AE_STATUS)
def _ae_status():
    """A forward and the range check behind it on the same stream: the check synchronises (the header says so)."""
    ae = _ae("bf16x3")
    pc = feed(clouds(116, 3, AE_N), clouds(117, 3, AE_N))

    def call():
        recon, latent = ae.forward(pc[0])
        return recon, latent, in_device(L().geoadv_ae_status, ae.handle, SH())
    return SO.Rig([pc], call, keep=ae)


@functools.lru_cache(maxsize=None)
def _clf():
    from geometric_adv_amd import cls_weights as CW
    from geometric_adv_amd.classifier import PointNetClassifier
    return PointNetClassifier(None, num_classes=13, weights=CW.synthetic_weights(13, seed=13))


CLS = (3, 300)


def _labels(seed, b):
    return np.random.default_rng(seed).integers(0, 13, b).astype(np.int32)


@case("cls_forward", ["geoadv_cls_forward"])
def _cls_forward():
    """The memset of the pooled keys, cls_chain_kernel<1>, the T-Net head, the second chain and head, the closing chain and head
    (csrc/classifier.hip's launch list), with both transforms returned."""
    clf = _clf()
    b, n = CLS
    pc = feed(clouds(118, b, n), clouds(119, b, n))
    return SO.Rig([pc], lambda: clf.forward(pc[0], transforms=True), keep=clf)


@case("cls_input_grad", ["geoadv_cls_input_grad"])
def _cls_input_grad():
    """The forward with stored winners (their 0x7f memset first) and the backward chain through both T-Nets, CW targeted loss."""
    clf = _clf()
    b, n = CLS
    pc, y = feed(clouds(120, b, n), clouds(121, b, n)), feed(_labels(122, b), (_labels(122, b) + 5) % 13)
    return SO.Rig([pc, y], lambda: clf.input_gradient(pc[0], y[0], "cw_targeted", 0.5, return_logits=True, return_winners=True), keep=clf)


@case("cls_evaluate_votes", ["geoadv_cls_evaluate"])
def _cls_evaluate():
    """Three votes: the memsets of pred_sum and vote_counts, then per vote the rotation, the forward's launches and the closing
    kernel."""
    clf = _clf()
    b, n = CLS
    pc, y = feed(clouds(123, b, n), clouds(124, b, n)), feed(_labels(125, b), (_labels(125, b) + 3) % 13)
    return SO.Rig([pc, y], lambda: clf.evaluate_batch(pc[0], y[0], 3), keep=clf)


@functools.lru_cache(maxsize=None)
def _atlas():
    from geometric_adv_amd import atlas_weights as AW
    from geometric_adv_amd.atlasnet import AtlasNetAE
    opt, state = AW.synthetic_state(4, 1, True, seed=5, number_points_eval=400)
    return AtlasNetAE(options=opt, state=state)


@case("atlas_forward", ["geoadv_atlas_forward"])
def _atlas_forward():
    """The memset of the pooled keys, atlas_enc_kernel, the two fc_batched_kernel launches, atlas_decoder_kernel."""
    ae = _atlas()
    pc = feed(clouds(126, 3, 300), clouds(127, 3, 300))
    return SO.Rig([pc], lambda: ae.forward(pc[0]), keep=ae)


@functools.lru_cache(maxsize=None)
def _fold():
    from geometric_adv_amd import fold_weights as FW
    from geometric_adv_amd.foldingnet import FoldingNetAE
    return FoldingNetAE(state=FW.synthetic_state(7), seed=5)


@case("fold_graph", ["geoadv_fold_graph"])
def _fold_graph():
    """The kNN search, the adjacency count (its memset first) and the covariance launches of build_graph."""
    ae = _fold()
    pc = feed(clouds(128, 3, 300), clouds(129, 3, 300))
    return SO.Rig([pc], lambda: ae.graph(pc[0]), keep=ae)


@case("fold_forward", ["geoadv_fold_forward"])
def _fold_forward():
    """The graph as above, the device draw of the picks, both pools, the pooled keys' memset, the fc layers and both folds; the
    picks, columns, code, fold1's output and the reconstruction all come back."""
    ae = _fold()
    pc = feed(clouds(130, 3, 300), clouds(131, 3, 300))

    def call():
        r = ae.forward(pc[0], cloud_offset=11, p1=True)
        return r["picks"], r["cols"], r["code"], r["p1"], r["recon"]
    return SO.Rig([pc], call, keep=ae)


# ---- the attack handle (stateful: every step of the protocol gets a twin from the same initial state) ------------------------------
ATT_B, ATT_N = 3, 256
ATTACK_FORMS = {       # name: loss_adv_type, loss_in_scan, encoder_backward, chamfer_kernel
    "chamfer_own_launch_masked": ("chamfer", False, "masked", "two_scan"),
    "chamfer_in_scan_jacobian": ("chamfer", "always", "jacobian", "symmetric"),
    "latent_own_launch_jacobian": ("latent", False, "jacobian", "symmetric"),
    "latent_in_scan_masked": ("latent", "always", "masked", "symmetric"),
}


def _attack_handle(form, chamfer_prune=True):
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    adv, in_scan, bwd, kern = ATTACK_FORMS[form]
    conf = Configuration(batch_size=ATT_B, n_points=ATT_N, weights=None, loss_adv_type=adv, loss_in_scan=in_scan, encoder_backward=bwd,
                         chamfer_kernel=kern, chamfer_prune=chamfer_prune, num_iterations=3, num_iterations_thresh=1)
    return AdvAE("stream-order", conf, ae=_ae("bf16x3"))


def _attack_feeds():
    B, n = ATT_B, ATT_N
    rng = np.random.default_rng(140)
    return [feed(clouds(141, B, n), clouds(142, B, n)), feed(clouds(143, B, n), clouds(144, B, n)),
            feed(np.abs(normal(145, B, 128)), np.abs(normal(146, B, 128))),
            feed(np.array([1.0, 0.5, 2.0], np.float32), np.array([0.25, 1.5, 1.0], np.float32)),
            feed(0.01 * normal(147, B, n, 3), 0.01 * normal(148, B, n, 3)),
            feed(0.01 + rng.random(B).astype(np.float32), 0.02 + rng.random(B).astype(np.float32))]


def _attack_rig(form):
    """set_inputs (copies, the grid box launch, memsets), init_pert (copies, fill_kernel, memsets), three iterations of run (the
    launch chain of the form), then get_best, peek, test_loss_state and test_plan -- none of which may block.  Adam's moments
    are not readable through the ABI: they are held through the perturbation of iterations 2 and 3, which they determine."""
    import torch
    at = _attack_handle(form)
    feeds = _attack_feeds()
    B, n = ATT_B, ATT_N
    hist = zf(3, 6, B)
    losses, r1, a1 = zf(8, B), zf(B, n), zf(B, n)

    def call():
        x, gt, tz, w, init, ref = (f[0] for f in feeds)
        at.set_inputs(x, gt, tz, w)
        at.init_pert(init, reset_optimizer=True)
        at.run(0, 3, 1, hist)
        metrics, adv, recon = at.get_best(ref)
        peek = at.peek()
        with torch.cuda.device(DEV):
            ok(L().geoadv_attack_test_loss_state(at._h, None, None, P(losses), P(r1), P(a1), SH()), "attack_test_loss_state")
        plan = at._test_plan()
        jstar = plan.pop("jstar")
        return [hist, metrics, adv, recon, losses, r1, a1, jstar, repr(sorted(plan.items()))] + [peek[k] for k in sorted(peek)]
    return SO.Rig(feeds, call, keep=at)


for _form in ATTACK_FORMS:
    case("attack_" + _form, ["geoadv_attack_set_inputs", "geoadv_attack_init_pert", "geoadv_attack_run", "geoadv_attack_get_best",
                             "geoadv_attack_peek", "geoadv_attack_test_loss_state", "geoadv_attack_test_plan"], stateful=True)(
        functools.partial(_attack_rig, _form))


def _attack_sync_rig(which):
    at = _attack_handle("chamfer_in_scan_jacobian", chamfer_prune="always")      # "always": the paired search at this size too
    feeds = _attack_feeds()

    def call():
        x, gt, tz, w, init, ref = (f[0] for f in feeds)
        at.set_inputs(x, gt, tz, w)
        at.init_pert(init, reset_optimizer=True)
        at.run(0, 1, 1)
        if which == "status":
            host = in_device(L().geoadv_attack_status, at._h, SH())
        else:
            host = at.search_state()
        peek = at.peek()
        return [host] + [peek[k] for k in sorted(peek)]
    return SO.Rig(feeds, call, keep=at)


case("attack_status", ["geoadv_attack_status"], stateful=True, blocks=SYNC_ATTACK_STATUS)(functools.partial(_attack_sync_rig, "status"))
case("attack_search_state", ["geoadv_attack_search_state"], stateful=True, blocks=SYNC_SEARCH_STATE)(
    functools.partial(_attack_sync_rig, "search"))


# ---- trainers (stateful) ---------------------------------------------------------------------------------------------------------
TR_B, TR_N = 4, 256


def _ae_trainer(loss="chamfer"):
    from geometric_adv_amd.trainer import PointNetAETrainer, initial_weights
    return PointNetAETrainer(initial_weights(TR_N, seed=1), TR_N, batch_size=TR_B, loss=loss)


def _ae_trainer_state(tr):
    def state():
        w = tr.export_weights()                              # synchronous: called after the comparison's synchronisation only
        return [tr.parameter_buffer(), tr.gradient_buffer()] + [w[k] for k in sorted(w) if "moving" in k]
    return state


def _ae_trainer_rig(how):
    """Two steps, so that Adam's moments (not readable through the ABI) show in the second step's parameters.
    step: geoadv_trainer_step; halves: forward_backward + apply through the wrapper; phases: every run_phase in order, fetch and
    apply (what the synchronised-batch-norm step does between its all-reduces)."""
    import torch
    tr = _ae_trainer()
    x = feed(clouds(150, TR_B, TR_N), clouds(151, TR_B, TR_N))
    loss, recon = zf(2), zf(2, TR_B, TR_N, 3)

    def call():
        for s in range(2):
            with torch.cuda.device(DEV):
                if how == "step":
                    ok(L().geoadv_trainer_step(tr._h, P(x[0]), None, P(loss[s:]), P(recon[s]), SH()), "trainer_step")
                elif how == "halves":
                    ok(L().geoadv_trainer_forward_backward(tr._h, P(x[0]), None, P(loss[s:]), P(recon[s]), SH()), "trainer_forward_backward")
                    tr.apply(1.0)
                else:
                    for p in range(L().geoadv_trainer_num_phases()):
                        ok(L().geoadv_trainer_run_phase(tr._h, p, P(x[0]), None, SH()), "trainer_run_phase")
                    ok(L().geoadv_trainer_fetch(tr._h, P(loss[s:]), P(recon[s]), SH()), "trainer_fetch")
                    tr.apply(1.0)
        return loss, recon
    return SO.Rig([x], call, state=_ae_trainer_state(tr), keep=tr)


case("trainer_step", ["geoadv_trainer_step"], stateful=True)(functools.partial(_ae_trainer_rig, "step"))
case("trainer_forward_backward_apply", ["geoadv_trainer_forward_backward", "geoadv_trainer_apply"], stateful=True)(
    functools.partial(_ae_trainer_rig, "halves"))
case("trainer_run_phases", ["geoadv_trainer_run_phase", "geoadv_trainer_fetch", "geoadv_trainer_apply"], stateful=True)(
    functools.partial(_ae_trainer_rig, "phases"))


@case("trainer_step_emd", ["geoadv_trainer_step"], stateful=True)
def _ae_trainer_emd():
    """The EMD loss's launches (the levels, the fused cost and gradient) in place of the Chamfer scan."""
    import torch
    tr = _ae_trainer("emd")
    x = feed(clouds(152, TR_B, TR_N), clouds(153, TR_B, TR_N))
    loss, recon = zf(1), zf(TR_B, TR_N, 3)

    def call():
        with torch.cuda.device(DEV):
            ok(L().geoadv_trainer_step(tr._h, P(x[0]), None, P(loss), P(recon), SH()), "trainer_step")
        return loss, recon
    return SO.Rig([x], call, state=_ae_trainer_state(tr), keep=tr)


@case("trainer_export", ["geoadv_trainer_step", "geoadv_trainer_export"], stateful=True, blocks=SYNC_EXPORT)
def _ae_trainer_export():
    """A step and the download behind it on the same stream: export synchronises (the header says so) and must return the
    variables of THAT step."""
    import torch
    tr = _ae_trainer()
    x = feed(clouds(154, TR_B, TR_N), clouds(155, TR_B, TR_N))
    loss = zf(1)

    def call():
        with torch.cuda.device(DEV):
            ok(L().geoadv_trainer_step(tr._h, P(x[0]), None, P(loss), None, SH()), "trainer_step")
        w = tr.export_weights()
        return [loss] + [w[k] for k in sorted(w)]
    return SO.Rig([x], call, keep=tr)


def _layer_state(tr, names, layers):
    """Host copies (LayerTrainer.state synchronises: called after the comparison's synchronisation only) of the whole parameter,
    gradient and slot arenas and the moving statistics of every layer that has them."""
    def state():
        out = [tr._host(tr._params_ptr), tr._host(tr._grads_ptr), tr.state("slot1"), tr.state("slot2"), np.array(tr.counters())]
        for l in layers:
            out += [np.asarray(tr.state(name, l)) for name in names]
        return out
    return state


def _cls_trainer_rig(optimizer):
    """geoadv_cls_trainer_step directly (train_step reads the labels' range on the host before the launch and the loss after
    it): the label copy, the forward and backward chains, the optimizer's launch, the copies of loss and pred."""
    import torch
    from geometric_adv_amd import cls_weights as CW
    from geometric_adv_amd.cls_trainer import PointNetClassifierTrainer
    tr = PointNetClassifierTrainer(weights=CW.synthetic_weights(13, 4), num_points=TR_N, batch_size=TR_B, num_classes=13,
                                   optimizer=optimizer, seed=3, decay_step=8)
    x, y = feed(clouds(156, TR_B, TR_N), clouds(157, TR_B, TR_N)), feed(_labels(158, TR_B), (_labels(158, TR_B) + 4) % 13)
    loss, pred = zf(1), zi(TR_B)
    bn_layers = [l for l, (_, _, _, bn, _) in enumerate(tr._shapes()) if bn]

    def call():
        with torch.cuda.device(DEV):
            ok(L().geoadv_cls_trainer_step(tr._h, P(x[0]), P(y[0]), P(loss), P(pred), SH()), "cls_trainer_step")
        return loss, pred
    return SO.Rig([x, y], call, state=_layer_state(tr, ("moving_mean", "moving_var"), bn_layers), keep=tr)


case("cls_trainer_step_adam", ["geoadv_cls_trainer_step"], stateful=True)(functools.partial(_cls_trainer_rig, "adam"))
case("cls_trainer_step_momentum", ["geoadv_cls_trainer_step"], stateful=True)(functools.partial(_cls_trainer_rig, "momentum"))


@case("fold_trainer_step", ["geoadv_fold_trainer_step"], stateful=True)
def _fold_trainer():
    """geoadv_fold_trainer_step directly (train_step downloads the losses), picks drawn on the device and returned: the graph,
    both pools, the folds, the Chamfer loss, the backward and Adam."""
    import torch
    from geometric_adv_amd import fold_weights as FW
    from geometric_adv_amd.fold_trainer import FoldingNetTrainer
    tr = FoldingNetTrainer(weights=FW.synthetic_state(0), num_points=TR_N, batch_size=TR_B, seed=5)
    x = feed(clouds(159, TR_B, TR_N), clouds(160, TR_B, TR_N))
    loss, picks = zf(2), zi(2, TR_B, TR_N, 16)

    def call():
        with torch.cuda.device(DEV):
            ok(L().geoadv_fold_trainer_step(tr._h, P(x[0]), 1, P(picks), P(loss), P(loss[1:]), SH()), "fold_trainer_step")
        return loss, picks
    return SO.Rig([x], call, state=_layer_state(tr, ("running_mean", "running_var"), range(6)), keep=tr)


def _atlas_trainer_rig(decoder_bn):
    """geoadv_atlas_trainer_step directly (train_step downloads the loss), the template drawn on the device and returned:
    at_template_kernel, the encoder and the per-primitive decoder GEMMs, the Chamfer loss, the backward and Adam."""
    import torch
    from geometric_adv_amd import atlas_weights as AW
    from geometric_adv_amd.atlas_trainer import AtlasNetTrainer
    nb, p = 2, 50
    opt, w = AW.synthetic_state(nb, 1, decoder_bn, seed=9, number_points_eval=nb * p)
    opt["number_points"] = nb * p
    tr = AtlasNetTrainer(weights=w, options=opt, num_points=TR_N, batch_size=TR_B, seed=6)
    x = feed(clouds(161, TR_B, TR_N), clouds(162, TR_B, TR_N))
    loss, tmpl = zf(1), zf(nb, p, 2)
    bn_layers = [l for l, layer in enumerate(tr.layers) if layer[4]]

    def call():
        with torch.cuda.device(DEV):
            ok(L().geoadv_atlas_trainer_step(tr._h, P(x[0]), 0, P(tmpl), P(loss), SH()), "atlas_trainer_step")
        return loss, tmpl
    return SO.Rig([x], call, state=_layer_state(tr, ("running_mean", "running_var"), bn_layers), keep=tr)


case("atlas_trainer_step_decoder_bn", ["geoadv_atlas_trainer_step"], stateful=True)(functools.partial(_atlas_trainer_rig, True))
case("atlas_trainer_step_no_decoder_bn", ["geoadv_atlas_trainer_step"], stateful=True)(functools.partial(_atlas_trainer_rig, False))


# ---- the tests -------------------------------------------------------------------------------------------------------------------
PROBES = ("cls_trainer_step_adam", "fold_trainer_step", "attack_chamfer_in_scan_jacobian")


def _probe():
    """The largest host-side enqueue time, in ms, of the slowest covered calls (measured: _stream_order.ENQUEUE_NOTE), each
    timed the way the protocol meets it: the first call of a twin handle, after another handle has run the same kernels."""
    import time
    import torch
    worst = 0.0
    for name in PROBES:
        build = CASES[name][0]
        for attempt in range(2):
            rig = build()
            rig.load("B")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rig.call()
            took = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            if attempt:                                     # the first handle only warms the kernels up
                worst = max(worst, took)
    return worst


@pytest.fixture(scope="module")
def delay():
    return SO.session_delay(_probe)


def test_control_a_stray_launch_on_the_null_stream_is_seen(delay):
    import torch
    y, a, b, pending = SO.control(delay, on_side_stream=False)
    vacuous = ("EVERY CASE OF THIS FILE IS VACUOUS: a multiply queued on the default stream while a side stream was still behind "
               "its delay did not read the stale input -- ")
    assert pending, vacuous + "the delay of %.0f ms had already run out" % delay.ms
    assert torch.equal(y, 2 * a), vacuous + ("the null stream waited for the side stream" if torch.equal(y, 2 * b) else
                                              "the result is neither 2 A nor 2 B")
    assert not torch.equal(y, 2 * b)


def test_control_the_same_launch_on_the_side_stream_is_in_order(delay):
    import torch
    y, a, b, pending = SO.control(delay, on_side_stream=True)
    assert pending, "the delay of %.0f ms had run out before the multiply was queued" % delay.ms
    assert torch.equal(y, 2 * b)


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_point_keeps_to_its_stream(name, delay):
    build, _, stateful, blocks = CASES[name]
    if name.startswith("ae_forward_"):
        arith = name[len("ae_forward_"):]
        if _ae(arith) is None:                              # the model does not admit this arithmetic: the library refuses it
            assert arith == "f16x2" and _ae("f32") is not None and _ae("bf16x3") is not None
            return
    SO.check(name, build, delay, stateful=stateful, blocks=blocks)


def test_forward_after_status_keeps_its_bits_and_its_flag(delay):
    """geoadv_ae_status clears the range flag on the stream it was given, so a forward queued on that stream directly behind it
    keeps the flag it raises: status (raised by an out-of-range cloud) -> cleared; behind a delay the same cloud again ->
    the forward's bits, and the next status reports the range error again."""
    import torch
    ERANGE = 4                                              # include/geoadv.h: GEOADV_ERANGE
    ae = _ae("f16x2")
    assert ae is not None, "the synthetic model admits f16x2"
    good, bad = T(clouds(170, 2, AE_N)), T(clouds(171, 2, AE_N) * 3.0e4)
    recon, latent = ae.forward(bad)
    torch.cuda.synchronize()
    want = (recon.clone(), latent.clone())
    assert bool(torch.isinf(want[1]).any()), "the cloud was meant to leave the f16x2 range"
    with torch.cuda.device(DEV):
        assert L().geoadv_ae_status(ae.handle, SH()) == ERANGE
        assert L().geoadv_ae_status(ae.handle, SH()) == 0                       # cleared
    x = good.clone()
    ae.forward(x)                                                               # the scratch now holds a good cloud's values
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    e_delay = torch.cuda.Event()
    with torch.cuda.stream(side), torch.cuda.device(DEV):
        assert L().geoadv_ae_status(ae.handle, SH()) == 0
        delay()
        x.copy_(bad)
        e_delay.record(side)
        assert not e_delay.query()
        got = ae.forward(x)
        assert not e_delay.query(), "ae_forward blocked the host"
        side.synchronize()
        assert not SO.differences(list(got), list(want))
        assert L().geoadv_ae_status(ae.handle, SH()) == ERANGE, "the forward's flag was lost"
        assert L().geoadv_ae_status(ae.handle, SH()) == 0


def _stream_functions():
    """Every function of include/geoadv.h with a `void *stream` parameter (parsed the way tests/test_abi.py parses it)."""
    text = open(os.path.join(ROOT, "include", "geoadv.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = re.findall(r"\b(geoadv_\w+)\s*\(([^;{}]*?)\)\s*;", text)
    return {name for name, args in protos if re.search(r"\bvoid\s*\*\s*stream\b", args)}


def test_every_stream_taking_entry_point_has_a_case():
    declared = _stream_functions()
    assert len(declared) >= 69
    covered = {f for _, covers, _, _ in CASES.values() for f in covers}
    assert not covered & set(EXEMPT), "covered and exempt at once: %s" % sorted(covered & set(EXEMPT))
    assert all(isinstance(r, str) and r.strip() for r in EXEMPT.values()), "every exemption carries its reason"
    missing, stale = declared - covered - set(EXEMPT), (covered | set(EXEMPT)) - declared
    assert not missing, "stream-taking entry points without a case in tests/test_gpu_stream_order.py: %s" % sorted(missing)
    assert not stale, "cases for functions the header no longer declares with a stream: %s" % sorted(stale)


def test_excuses_quote_the_header():
    """An entry point may block the host only if the header says so at its declaration: every excuse is a sentence of it."""
    text = " ".join(open(os.path.join(ROOT, "include", "geoadv.h")).read().replace("*", " ").split())
    for name, (_, _, _, blocks) in CASES.items():
        if blocks is not None:
            assert " ".join(blocks.replace("*", " ").split()) in text, (name, blocks)


def test_report_enqueue_times(delay):
    """Prints (-s) what the helper's docstring records: the delay chosen and every case's host-side enqueue time."""
    times = sorted(SO.ENQUEUE_MS.items(), key=lambda kv: -kv[1])
    print("\ndelay %.1f ms (probe %.3f ms); slowest enqueues: %s" % (delay.ms, delay.probe_ms or -1.0,
                                                                   ", ".join("%s %.3f" % kv for kv in times[:8])))
    assert SO.MIN_DELAY_MS <= delay.ms <= SO.MAX_DELAY_MS
