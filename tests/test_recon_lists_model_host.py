"""CPU: the neighbour-list certificate of csrc/chamfer_lists.hip, as modelled in tests/_recon_lists_model.py, never certifies a wrong
index -- on random clouds at several motions and skins and on the adversarial cases the GPU tests run (duplicates, near ties,
a partner just outside a list that moves to within one float32 step of the list's best, a dense blob against far columns, a NaN)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _chamfer_hard_clouds as HC  # noqa: E402
import _recon_lists_model as M  # noqa: E402


def _exact(anchor, c, moved, skin, cap=16):
    L = M.Lists(anchor, c, skin, cap)
    d1, i1, d2, i2, info = M.query(L, moved)
    r1, j1, r2, j2 = M.reference(moved, c)
    assert np.array_equal(i1, j1) and np.array_equal(i2, j2)
    assert d1.tobytes() == r1.tobytes() and d2.tobytes() == r2.tobytes()
    return info


@pytest.mark.parametrize("n", [65, 256, 700])
@pytest.mark.parametrize("step,skin", [(1e-4, 1e-2), (3e-3, 1e-2), (9e-3, 1e-2), (2e-2, 1e-2), (1e-4, 0.0), (0.0, 5e-3)])
def test_random_clouds_are_answered_exactly(n, step, skin):
    a, c = M.uniform(10 + n, 1, n)[0], M.uniform(20 + n, 1, n)[0]
    info = _exact(a, c, M.moved_by(a, 30 + n, step), skin)
    if step == 1e-4 and skin == 1e-2:
        # structurally: the anchor's nearest partner is in the list and still within sqrt(min) + step, so
        # sqrt(best) + step <= sqrt(min) + 2 step < sqrt(min) + skin - margin; a list overflows only with 17 partners inside the skin
        assert info["cert_row"].all() and info["cert_col"].all()


def test_motion_beyond_the_skin_refuses_everything():
    a, c = M.uniform(1, 1, 256)[0], M.uniform(2, 1, 256)[0]
    # (a displacement beyond every sqrt(tau): sqrt(best) + displacement < sqrt(tau) cannot hold for any query)
    info = _exact(a, c, M.moved_by(a, 3, 2.0), 1e-2)
    assert not info["cert_row"].any() and not info["cert_col"].any() and info["flagged"]


@pytest.mark.parametrize("n", [65, 256])
def test_duplicates_pick_the_lowest_index(n):
    a, c = M.duplicated(5, 1, n)
    info = _exact(a[0], c[0], a[0], 2.0 ** -6)
    assert info["cert_row"].any() or info["unlisted_row"].any()
    info = _exact(a[0], c[0], M.moved_by(a[0], 6, 2.0 ** -12), 2.0 ** -6)


@pytest.mark.parametrize("log2_rho", [-6, -10, -14])
@pytest.mark.parametrize("swapped", [False, True])
def test_near_ties_of_the_hard_cloud_generators(log2_rho, swapped):
    a, c = HC.shell_and_cluster(1, 256, 256, 41, log2_rho, swapped)
    _exact(a[0], c[0], M.moved_by(a[0], 42, 1e-4), 1e-2)
    _exact(a[0], c[0], M.moved_by(a[0], 43, 2.0 ** (log2_rho - 2)), 2.0 ** log2_rho)
    a, c = HC.with_outlier("both", 6, 1, 256, 256, 44)
    _exact(a[0], c[0], M.moved_by(a[0], 45, 1e-4), 1e-2)


@pytest.mark.parametrize("which", ["closer", "equal", "farther"])
@pytest.mark.parametrize("low_index", [False, True])
def test_a_partner_just_outside_the_list_is_never_certified_away(which, low_index):
    a, c, moved, skin, g = M.boundary_case(50, 65, which, low_index)
    L = M.Lists(a, c, skin)
    row, inside, outside = g["row"]
    col, r_in, r_out = g["col"]
    assert list(L.rows[row]) == [inside] and outside not in L.rows[row]
    assert list(L.cols[col]) == [r_in]
    info = _exact(a, c, moved, skin)
    assert not info["cert_row"][row] and not info["cert_col"][col]
    _, i1, _, i2 = M.reference(moved, c)
    want_out = which == "closer" or (which == "equal" and low_index)
    assert i1[row] == (outside if want_out else inside)
    assert i2[col] == (r_out if want_out else r_in)


def test_a_dense_blob_overflows_the_far_columns_lists():
    a, c = M.blob_and_far_column(60, 1, 256)
    info = _exact(a[0], c[0], M.moved_by(a[0], 61, 1e-4), 1e-2)
    assert info["unlisted_col"].mean() > 0.5 and not info["cert_col"][info["unlisted_col"]].any()


def test_a_nan_is_refused():
    a, c = M.uniform(70, 1, 65)[0], M.uniform(71, 1, 65)[0]
    moved = M.moved_by(a, 72, 1e-4)
    moved[7, 1] = np.nan
    L = M.Lists(a, c, 1e-2)
    _, i1, _, i2, info = M.query(L, moved)
    assert not info["cert_row"][7] and not info["cert_col"].any()          # the cloud's largest displacement is NaN
    assert (0 <= i1).all() and (i1 < 65).all() and (0 <= i2).all() and (i2 < 65).all()
