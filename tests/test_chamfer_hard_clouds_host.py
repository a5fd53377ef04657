"""CPU: the hard-cloud generators of tests/_chamfer_hard_clouds.py held to their own claims, so that the GPU tests built on them
(tests/test_gpu_chamfer_mx_hard.py) cannot go vacuous: the float32 model equals the C oracle bit for bit on every family; every
tie the deterministic family lists IS an exact float32 tie (or, broken, a win of the highest index by less than 2^-30) between
exactly the listed candidates, in the layout class it is listed under; plain queries have their second neighbour a lattice step
away; the list loads are the ones asked for -- by construction AND by the predictor that evaluates the kernel's own eps formula
on the float32 distances; and no plan ever asks for a screened kernel other than the 256-column one."""
import numpy as np
import pytest

import _chamfer_hard_clouds as hc
from test_chamfer_sym_plan_host import BATCHES, SIZES, _plan, lib  # noqa: F401  (lib: the fixture)

GPU_SHAPES = [(32, 2048, 2048), (64, 2048, 2048), (128, 2048, 2048), (64, 1990, 1000), (8, 4096, 4096), (10, 2049, 5000)]
TABLE = {(32, 2048, 2048): (1, 8, 1), (64, 2048, 2048): (2, 4, 1), (128, 2048, 2048): (4, 2, 1), (64, 1990, 1000): (1, 4, 1),
         (8, 4096, 4096): (1, 16, 2), (10, 2049, 5000): (2, 10, 2)}                    # S, column slices, row super-tiles
SEED = 20


def _families(n, m):
    """Two clouds of every family at (n, m); the deterministic one from the plan of a batch that reaches the screened kernel."""
    plan = hc.plan_of(64, n, m)
    out = {}
    for near in (False, True):
        cs = hc.constellations(plan, n, m, SEED, clouds=2, near=near)
        out["constellations_near" if near else "constellations"] = (cs.a, cs.c)
    if n == m == 2048:
        cs = hc.constellations(plan, n, m, SEED, clouds=2, capacity=True)
        out["capacity"] = (cs.a, cs.c)
    for log2_rho in (-2, -10, -16):
        for swapped in (False, True):
            out["shell%d%s" % (log2_rho, "s" if swapped else "")] = hc.shell_and_cluster(2, n, m, SEED, log2_rho, swapped)
    for kind, e in (("uniform", -41), ("sphere", -40), ("uniform", 39), ("sphere", 41)):
        out["scaled_%s_%d" % (kind, e)] = hc.scaled(kind, e, 2, n, m, SEED)
    for where, e in (("rows", 6), ("cols", 12), ("both", 20)):
        out["outlier_%s_%d" % (where, e)] = hc.with_outlier(where, e, 2, n, m, SEED)
    return out


@pytest.mark.parametrize("b,n,m", [(2, 2048, 2048), (1, 1990, 1000), (1, 2049, 700)])
def test_model32_is_the_oracle(oracle, b, n, m):
    for name, (a, c) in _families(n, m).items():
        assert np.isfinite(a).all() and np.isfinite(c).all(), name
        got, want = hc.nn_model32(a[:b], c[:b]), oracle.nn_distance(a[:b], c[:b])
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.int32), w.view(np.int32)), name


def test_layout_mirrors_the_header_constants():
    import os
    import re
    text = open(os.path.join(os.path.dirname(hc.__file__), "..", "geometric_adv_amd", "csrc", "chamfer_mx.h")).read()
    val = lambda name: re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1).strip()
    assert val("MX_RT") == "8" and val("MX_WROWS") == "32 * MX_RT" and val("MX_WAVES") == "8" and val("MX_ROWS") == "MX_WAVES * MX_WROWS"
    assert (hc.MX_WROWS, hc.MX_ROWS) == (256, 2048)
    assert int(val("MX_ICAP")) == hc.MX_ICAP and int(val("MX_CCAP")) == hc.MX_CCAP and int(val("MX_CMAX")) == 256
    assert val("MX_ROW_IDMASK") == "31u" and val("MX_COL_IDMASK") == "127u"


def _check_classes(L, cs, hosted):
    assert sorted(cs.classes) == sorted(hosted)
    dist = [hc.dist32(cs.a[u], cs.c[u]) for u in range(cs.a.shape[0])]
    for cls, items in cs.classes.items():
        assert items, cls
        lowest_at = set()
        for ci, direction, q, cand in items:
            cand = np.array(cand)
            line = dist[ci][q] if direction == "row" else dist[ci][:, q]
            assert (L.row_class(cand) if direction == "row" else L.col_class(cand)) == cls, (cls, ci, q)
            best = line.min()
            if not cs.near:
                assert np.array_equal(np.flatnonzero(line == best), cand), (cls, ci, q)      # exactly these, exactly equal
                assert line.argmin() == cand.min()
                pts = cs.c[ci][cand] if direction == "row" else cs.a[ci][cand]
                me = cs.a[ci][q] if direction == "row" else cs.c[ci][q]
                off = np.round((pts[0].astype(np.float64) - me) / hc.D).astype(int)
                lowest_at.add(tuple(off))
            else:
                assert line.argmin() == cand.max() and (line == best).sum() == 1, (cls, ci, q)
                rest = line[cand[:-1]].astype(np.float64)
                assert (rest == rest[0]).all() and 0 < rest[0] - best < 2.0 ** -30, (cls, ci, q)
                assert np.partition(line, len(cand))[len(cand)] - best >= 2.0 ** -9 - 2.0 ** -12
        if not cs.near and len(items) >= 6:
            assert len(lowest_at) >= len(items[0][3]), (cls, lowest_at)           # the lowest index took every position
    for (ci, rows), (_, cols) in zip(cs.plain_rows, cs.plain_cols):
        assert len(rows) >= 256 and len(cols) >= 256
        p = np.partition(dist[ci][rows].astype(np.float64), 1, axis=1)
        assert (p[:, 1] - p[:, 0] >= 2.0 ** -9).all()
        p = np.partition(dist[ci][:, cols].astype(np.float64), 1, axis=0)
        assert (p[1] - p[0] >= 2.0 ** -9).all()


@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("b,n,m", GPU_SHAPES)
def test_constellation_classes_are_what_they_say(b, n, m, near):
    plan = hc.plan_of(b, n, m)
    assert (plan["S"], plan["cslices"], plan["rtiles"]) == TABLE[(b, n, m)] and plan["screened"] == 1
    L = hc.layout(plan, n, m)
    cs = hc.constellations(plan, n, m, SEED, near=near)
    hosted = hc.hosted_classes(plan)
    assert ("c" in hosted) == (plan["S"] >= 2) == ("e" in hosted) and ("d" in hosted) and ("j" in hosted) == (plan["rtiles"] >= 2)
    _check_classes(L, cs, hosted)
    # the ties must meet the kernel's certified paths, not a wave that redoes all of its rows or columns: the lists stay short
    with np.errstate(invalid="ignore"):
        for u in (0, 5):
            pl = hc.predict_lists(plan, cs.a[u], cs.c[u])
            for rt in range(plan["rtiles"]):
                for w in range(8):
                    real = min(max(n - rt * hc.MX_ROWS - w * hc.MX_WROWS, 0), hc.MX_WROWS)
                    if real:                                                         # (a ragged last wave lists its padding rows too)
                        assert pl["rows_hi"][rt, :, w].max() <= hc.MX_ICAP // 2 + (hc.MX_WROWS - real) * plan["S"], (rt, w)
            assert pl["cols_hi"].max() <= hc.MX_CCAP // 2


@pytest.mark.parametrize("b", [32, 64, 128])
def test_list_loads_are_the_ones_asked_for(b):
    n = m = 2048
    plan = hc.plan_of(b, n, m)
    L = hc.layout(plan, n, m)
    cs = hc.constellations(plan, n, m, SEED, capacity=True)
    _check_classes(L, cs, sorted(cs.classes))
    assert {"b"} | ({"g", "h"} if plan["S"] >= 2 else set()) <= set(cs.classes) <= {"a", "a'", "b", "g", "h"}
    rows = {k: v for k, v in cs.capacity.items() if k[1] == "row"}
    cols = {k: v for k, v in cs.capacity.items() if k[1] == "col"}
    assert set(rows.values()) == set(range(152, 169)) and len(rows) == 64
    assert (set(cols.values()) == set(range(28, 37)) and len(cols) == 16) if plan["S"] >= 2 else not cols
    # by construction: the class-b rows of a wave, the class g / h columns a wave serves in a workgroup
    for (ci, _, w, sl), k in rows.items():
        mine = [q for c2, d, q, cand in cs.classes["b"] if c2 == ci and L.row(q)["wave"] == w]
        assert len(mine) == k and all(L.col(cand[0])["slice"] == sl for c2, d, q, cand in cs.classes["b"] if c2 == ci and L.row(q)["wave"] == w)
    for (ci, _, w, sl), k in cols.items():
        mine = [q for cls in "gh" for c2, d, q, cand in cs.classes[cls] if c2 == ci and L.col(q)["wave"] == w and L.col(q)["slice"] == sl]
        assert len(mine) == k
    # ... and by the kernel's eps formula on the float32 distances: what must be listed = what may be listed = k, nothing else anywhere
    for ci in range(cs.a.shape[0]):
        with np.errstate(invalid="ignore"):
            pl = hc.predict_lists(plan, cs.a[ci], cs.c[ci])
        want_r, want_c = np.zeros_like(pl["rows_lo"]), np.zeros_like(pl["cols_lo"])
        for (c2, _, w, sl), k in rows.items():
            if c2 == ci:
                want_r[0, sl, w] = k
        for (c2, _, w, sl), k in cols.items():
            if c2 == ci:
                want_c[0, sl, w] = k
        assert np.array_equal(pl["rows_lo"], want_r) and np.array_equal(pl["rows_hi"], want_r), ci
        assert np.array_equal(pl["cols_lo"], want_c) and np.array_equal(pl["cols_hi"], want_c), ci
    assert any(k < hc.MX_ICAP for k in rows.values()) and any(k > hc.MX_ICAP for k in rows.values()) and hc.MX_ICAP in rows.values()
    assert not cols or (min(cols.values()) < hc.MX_CCAP < max(cols.values()) and hc.MX_CCAP in cols.values())


def test_gap_scale_and_outlier_families():
    a, c = hc.shell_and_cluster(2, 300, 200, SEED, -10)
    assert np.abs(a - hc.C0).max() <= 2.0 ** -11 + 1e-7 and np.allclose(np.linalg.norm(c - hc.C0, axis=2), 0.4, atol=1e-6)
    a, c = hc.shell_and_cluster(2, 300, 200, SEED, -10, swapped=True)
    assert np.abs(c - hc.C0).max() <= 2.0 ** -11 + 1e-7 and np.allclose(np.linalg.norm(a - hc.C0, axis=2), 0.4, atol=1e-6)
    for e in (-41, -40, -39, 39, 40, 41):
        for kind in ("uniform", "sphere"):
            a, c = hc.scaled(kind, e, 2, 2048, 2048, SEED)
            big = [hc.centred_big(a[u], c[u]) for u in range(2)]
            assert all(2.0 ** e <= v < 2.0 ** (e + 1) for v in big)
            assert all((2.0 ** -40 <= v <= 2.0 ** 40) == (-40 <= e <= 39) for v in big)
            d1 = hc.nn_model32(a[:1], c[:1])[0]
            assert np.isfinite(d1).all() and (d1[d1 > 0] >= 2.0 ** -126).all()              # finite and normal
    for where in ("rows", "cols", "both"):
        for e in (6, 12, 20):
            a, c = hc.with_outlier(where, e, 2, 2048, 2048, SEED)
            far_r = (np.linalg.norm(a.astype(np.float64), axis=2) > 2.0).sum(1)
            far_c = (np.linalg.norm(c.astype(np.float64), axis=2) > 2.0).sum(1)
            assert (far_r == (where != "cols")).all() and (far_c == (where != "rows")).all()
            assert np.isclose(max(np.abs(a).max(), np.abs(c).max()), 2.0 ** e, rtol=0.5)


def test_every_screened_plan_is_the_256_column_kernel(lib):  # noqa: F811
    """The sweep of test_plan_invariants_and_scratch_bound: were a request to give a screened plan with narrower stages, the
    instantiations chamfer_mx_kernel<4> and <2> would have to come back."""
    screened = 0
    for n in SIZES:
        for b in BATCHES:
            for np_ in (1, 2):
                for loop in (0, 1):
                    for q in (0, 40):
                        p = _plan(lib, np=np_, b=b, n=n, m=n, loop=loop, q_clouds=q)
                        if p["screened"]:
                            screened += 1
                            assert p["C"] == 256 and p["kernel"] == 8, (n, b, np_, loop, q)
                        else:
                            assert p["kernel"] == 0
    assert screened > 1000
