"""GPU: the matrix-pipe-screened symmetric Chamfer scan (csrc/chamfer_mx.h) on inputs that sit ON the boundaries of its layout and
of its error bound (tests/_chamfer_hard_clouds.py; their claims are checked on the CPU by test_chamfer_hard_clouds_host.py):
exact ties by layout class, the same ties broken in favour of the highest index by 2^-33 in the squared distance, per-wave lists
loaded to just below and just above MX_ICAP / MX_CCAP, the best-to-second gap swept through eps, the data-derived scale at the
edges of its sane range, and one outlier that owns the scale.

Every case: the shape reaches the screened kernel and has the plan it was written for (asserted from the plan ABI); the
operator's entry point geoadv_nn_distance_sym -- what ops.nn_distance(kernel="symmetric") calls -- runs with its four outputs and
its scratch between canaries; the whole batch must be the two-scan kernel's bits (kernel="scan"), and clouds 0, b - 1 and two
others the float32 model's and the C oracle's.  8 distinct clouds per case, repeated to fill the batch (the scan's group-to-XCD
mapping spreads them over the chip anyway).

Which test caught which injected fault, and how far eps can shrink before these tests notice, is recorded in DESIGN.md (5)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _chamfer_hard_clouds as hc

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0DEAD
SEED = 20
TABLE = {(32, 2048, 2048): (1, 8, 1), (64, 2048, 2048): (2, 4, 1), (128, 2048, 2048): (4, 2, 1), (64, 1990, 1000): (1, 4, 1),
         (8, 4096, 4096): (1, 16, 2), (10, 2049, 5000): (2, 10, 2)}                    # S, column slices, row super-tiles
SHAPES = list(TABLE)
SQUARE = SHAPES[:3]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class _Guarded:
    """`count` words inside a larger allocation, everything preset to the canary word."""

    def __init__(self, count, dtype, front=65, back=64):
        import torch
        self.front, self.count = front, int(count)
        self.buf = torch.full((front + self.count + back,), CANARY, dtype=torch.int32, device="cuda:0")
        self.t = self.buf[front:front + self.count].view(dtype)

    def intact(self):
        return bool((self.buf[:self.front] == CANARY).all()) and bool((self.buf[self.front + self.count:] == CANARY).all())


def _sym_guarded(x1, x2):
    import torch
    from geometric_adv_amd import _lib
    lib = _lib.lib()
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    wf = int(lib.geoadv_nn_distance_sym_workspace_floats(b, n, m))
    d1, i1, d2, i2 = _Guarded(b * n, torch.float32), _Guarded(b * n, torch.int32), _Guarded(b * m, torch.float32), _Guarded(b * m, torch.int32)
    ws = _Guarded(wf, torch.float32)
    rc = lib.geoadv_nn_distance_sym(b, n, _lib.ptr(x1), m, _lib.ptr(x2), _lib.ptr(d1.t), _lib.ptr(i1.t), _lib.ptr(d2.t), _lib.ptr(i2.t),
                                    _lib.ptr(ws.t), C.c_size_t(wf), _lib.stream_handle())
    assert rc == 0, lib.geoadv_last_error()
    torch.cuda.synchronize()
    for g in (d1, i1, d2, i2, ws):
        assert g.intact(), "a canary next to a buffer of %d words was overwritten" % g.count
    return d1.t.view(b, n).clone(), i1.t.view(b, n).clone(), d2.t.view(b, m).clone(), i2.t.view(b, m).clone()


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _run(oracle, b, n, m, a8, c8, label=None):
    """a8, c8: the distinct clouds.  label(cloud, 'row' | 'col', query) -> what to call a differing query in the report."""
    from geometric_adv_amd import _lib, ops
    plan = hc.plan_of(b, n, m)
    assert _lib.lib().geoadv_nn_distance_sym_is_screened(b, n, m) == 1 and plan["screened"] == 1 and plan["kernel"] == 8
    if (b, n, m) in TABLE:
        assert (plan["S"], plan["cslices"], plan["rtiles"]) == TABLE[(b, n, m)]
    rep = np.arange(b) % a8.shape[0]
    x1, x2 = _t(a8[rep]), _t(c8[rep])
    got = [g.cpu().numpy() for g in _sym_guarded(x1, x2)]
    ref = [g.cpu().numpy() for g in ops.nn_distance(x1, x2, kernel="scan")]

    def same(got_, want_, clouds, against):
        for u, (g, w) in enumerate(zip(got_, want_)):
            bad = np.argwhere(_bits(g) != _bits(w))
            if len(bad):
                ci, q = int(bad[0][0]), int(bad[0][1])
                direction = "row" if u < 2 else "col"
                what = label(int(rep[clouds[ci]]), direction, q) if label else "-"
                raise AssertionError("%s: %d of %d %s queries differ in %s; first: cloud %d %s %d (class %s): got %r, want %r"
                                     % (against, len(bad), g.size, direction, ("dist1", "idx1", "dist2", "idx2")[u], clouds[ci], direction, q,
                                        what, g[ci, q], w[ci, q]))

    same(got, ref, np.arange(b), "two-scan kernel")
    pick = sorted({0, b // 3, (2 * b) // 3, b - 1})
    same([g[pick] for g in got], hc.nn_model32(a8[rep[pick]], c8[rep[pick]]), pick, "float32 model")
    same([g[pick] for g in got], oracle.nn_distance(a8[rep[pick]], c8[rep[pick]]), pick, "C oracle")


@functools.lru_cache(maxsize=4)
def _constellations(b, n, m, near, capacity):
    return hc.constellations(hc.plan_of(b, n, m), n, m, SEED, near=near, capacity=capacity)


def _labeller(cs):
    by = {(ci, d, q): cls for cls, items in cs.classes.items() for ci, d, q, cand in items}
    return lambda ci, d, q: by.get((ci, d, q), "none: plain or unplanned")


@pytest.mark.parametrize("b,n,m", SHAPES)
def test_constellation_ties_by_class(oracle, b, n, m):
    """Exact float32 ties placed in every layout class the shape hosts (the host test asserts which): same chunk / lane pair / chunks
    of a stage / stages / slices / three-way for rows; chunk / two and three chunks of a wave / waves / super-tiles for columns; the
    lowest index in every position."""
    cs = _constellations(b, n, m, False, False)
    assert sorted(cs.classes) == hc.hosted_classes(hc.plan_of(b, n, m))
    _run(oracle, b, n, m, cs.a, cs.c, _labeller(cs))


@pytest.mark.parametrize("b,n,m", SQUARE)
def test_list_capacities_straddled(oracle, b, n, m):
    """k = 152 ... 168 listed rows per wave around MX_ICAP = 160, and (S >= 2) k' = 28 ... 36 deferred columns per wave around MX_CCAP =
    32, in ONE launch: waves that answer from their lists next to waves that overflow and redo all of their rows or columns.  By
    construction (and by the CPU predictor, test_chamfer_hard_clouds_host.py): the kernel reports no counts."""
    cs = _constellations(b, n, m, False, True)
    ks = [v for k, v in cs.capacity.items() if k[1] == "row"]
    assert min(ks) < hc.MX_ICAP < max(ks) and hc.MX_ICAP in ks and hc.MX_ICAP + 1 in ks
    _run(oracle, b, n, m, cs.a, cs.c, _labeller(cs))


@pytest.mark.parametrize("b,n,m", SHAPES)
def test_near_ties_one_ulp_apart(oracle, b, n, m):
    """The same constellations with every tie broken in favour of the HIGHEST index by the smallest step every site coordinate can
    take (2^-24, one ulp at the clouds' edge: 2^-33 in the squared distance, 10^5 times below eps): the reference answers the
    highest index (asserted on the CPU), a kernel that trusts its approximation or its index order answers another.  The list-load
    clouds run in this form too."""
    cs = _constellations(b, n, m, True, False)
    _run(oracle, b, n, m, cs.a, cs.c, _labeller(cs))
    if (b, n, m) in SQUARE:
        cs = _constellations(b, n, m, True, True)
        _run(oracle, b, n, m, cs.a, cs.c, _labeller(cs))


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("log2_rho", [-2, -4, -6, -8, -10, -12, -14, -16])
@pytest.mark.parametrize("b,n,m", SQUARE[:2])
def test_gap_sweep_shell_and_cluster(oracle, b, n, m, log2_rho, swapped):
    """A cube of edge rho against a shell of radius 0.4 around it: the share of queries whose two best chunks lie within 2 eps goes
    from under 1 % (rho = 2^-2) through both sides of MX_ICAP in one launch (2^-10) to all of them (2^-14 and below)."""
    a, c = hc.shell_and_cluster(8, n, m, SEED, log2_rho, swapped)
    _run(oracle, b, n, m, a, c)


@pytest.mark.parametrize("kind", ["uniform", "sphere"])
@pytest.mark.parametrize("log2_big", [-41, -40, -39, 39, 40, 41])
def test_scale_at_the_edges_of_the_sane_range(oracle, kind, log2_big):
    """The largest centred coordinate just inside and just outside [2^-40, 2^40]: screened with a scale of 2^53 ... 2^-26, or every
    chunk a candidate; the reference's squares (2^-82 ... 2^82) stay finite and normal."""
    a, c = hc.scaled(kind, log2_big, 8, 2048, 2048, SEED)
    _run(oracle, 32, 2048, 2048, a, c)


@pytest.mark.parametrize("where", ["rows", "cols", "both"])
@pytest.mark.parametrize("log2_far", [6, 12, 20])
@pytest.mark.parametrize("b,n,m", [(32, 2048, 2048), (8, 4096, 4096)])
def test_one_outlier_owns_the_scale(oracle, b, n, m, log2_far, where):
    """One point at distance 2^6 / 2^12 / 2^20 from a unit cloud pair, in the rows (every workgroup of the super-tile sees it), in the
    columns (one column slice does) or in both: there the rest of the cloud collapses below eps, next door it screens normally."""
    a, c = hc.with_outlier(where, log2_far, 8, n, m, SEED)
    _run(oracle, b, n, m, a, c)
