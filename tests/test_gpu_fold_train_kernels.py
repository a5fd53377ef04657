"""GPU: the graph pool, its backward gather and the global maximum of the FoldingNet training step on their own
(geoadv_fold_train_pool / _pool_grad / _gmax through ops, each through the launch the step itself uses), against the plain numpy
statement of their rules in tests/_fold_pool_model.py, BIT FOR BIT, on inputs built so that the rules matter: most maxima are tied,
zeros carry both signs, sources share destinations, a hub has n - 1 sources, the global maximum's ties fall across all four row
phases.  tests/test_fold_pool_model_host.py shows on the CPU that these very inputs (the case lists of the model module) tell
each rule from its near misses.  Every output lies between two sentinel zones that must come back untouched.

Why not a whole training step on clouds with duplicated halves, as the classifier's tests have: a point and its twin get the
same 16 neighbours, but their covariances are summed in different orders, so their features need not agree to the bit, and
"every maximum is attained twice" does not hold for this model.  The tie rules are therefore held here, on the kernels, and in
test_gpu_fold_train.py from the state every step stores."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fold_pool_model as P  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 67                    # elements in front of and behind every output (odd: the payload is only 4-byte aligned)
F_SENTINEL, I_SENTINEL = np.float32(-12345.5), np.int32(-54321)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Out:
    """An output of `count` elements inside a sentinel-filled allocation."""
    def __init__(self, count, dtype):
        self.count, self.fill = count, F_SENTINEL if dtype == torch.float32 else I_SENTINEL
        self.whole = torch.full((count + 2 * PAD,), self.fill.item(), dtype=dtype, device=DEV)
        self.t = self.whole[PAD:PAD + count]

    def read(self, shape):
        torch.cuda.synchronize()
        raw = self.whole.cpu().numpy()
        assert (raw[:PAD] == self.fill).all() and (raw[PAD + self.count:] == self.fill).all(), "written outside the output"
        return raw[PAD:PAD + self.count].reshape(shape).copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run_pool(h, cols):
    from geometric_adv_amd import ops
    b, n, c = h.shape
    g, win = _Out(h.size, torch.float32), _Out(h.size, torch.int32)
    ops.fold_train_pool(b, n, c, _dev(h), _dev(cols.astype(np.int32)), g.t, win.t)
    return g.read(h.shape), win.read(h.shape)


def run_pool_grad(dg, win, adjacency):
    from geometric_adv_amd import ops
    b, n, c = dg.shape
    off, deg, col = P.csr(adjacency)
    dh = _Out(dg.size, torch.float32)
    ops.fold_train_pool_grad(b, n, c, _dev(dg), _dev(win.astype(np.int32)), _dev(off), _dev(deg), _dev(col), dh.t)
    return dh.read(dg.shape)


def run_gmax(a, inv, shift):
    from geometric_adv_amd import ops
    b, n, c = a.shape
    pooled, arg = _Out(b * c, torch.float32), _Out(b * c, torch.int32)
    ops.fold_train_gmax(b, n, c, _dev(a), _dev(inv), _dev(shift), pooled.t, arg.t)
    return pooled.read((b, c)), arg.read((b, c))


_CASES = {}
POOL_IDS = [s + (kind,) for s in P.POOL_SHAPES for kind in P.POOL_INPUTS]
GRAD_IDS = [s + (with_self,) for s in P.POOL_SHAPES for with_self in (True, False)]


def _cases(which):
    """The model module's case lists, built once on first use: {case id: its inputs}."""
    if which not in _CASES:
        _CASES[which] = {name: rest for name, *rest in {"pool": P.pool_cases, "grad": P.grad_cases, "gmax": P.gmax_cases}[which]()}
    return _CASES[which]


@pytest.mark.parametrize("case", POOL_IDS, ids=lambda k: "%dx%dx%d-%s" % k)
def test_pool_winner_and_value_equal_the_rule(case):
    """The winner rule of ft_graph_pool_kernel: the point itself first, then the lowest slot, strict >; -1 and +0 unless the
    maximum is positive (a maximum of -0.0 or +0.0 is not)."""
    h, cols = _cases("pool")[case]
    want_g, want_win = P.pool(h, cols)
    g, win = run_pool(h, cols)
    assert np.array_equal(win, want_win), (case, float(np.mean(win != want_win)))
    assert np.array_equal(_bits(g), _bits(want_g)), case


def _conserved(dh, dg, win):
    """sum over points of dh == sum of dg over the elements that have a winner, per cloud and channel."""
    return dh.astype(np.float64).sum(1), np.where(win >= 0, dg, 0).astype(np.float64).sum(1)


@pytest.mark.parametrize("case", GRAD_IDS, ids=lambda k: "%dx%dx%d-%s" % (k[:3] + ("self" if k[3] else "noself",)))
def test_pool_gradient_gather_equals_the_scatter(case):
    """ft_pool_bwd_kernel's gather by destination against the scatter by source: every source of a destination is found in its row
    (a hub with n - 1 of them included), the point itself counts once whether or not its row holds it, and the float32 sum runs
    self first, then in ascending order of the source.  Winners: those of a tied pool (many sources per destination), none, and
    every point its own."""
    adj, win, dgi, dgf = _cases("grad")[case]
    b, n, c = dgi.shape
    own = np.broadcast_to(np.arange(n, dtype=np.int32)[None, :, None], win.shape)
    for name, w in (("pool", win), ("none", np.full_like(win, -1)), ("own", own)):
        got = run_pool_grad(dgi, w, adj)
        assert np.array_equal(got, P.pool_grad64(dgi, w, adj)), (case, name)            # integer-valued: any order is exact
        s, t = _conserved(got, dgi, w)
        assert np.array_equal(s, t), (case, name)                                       # nothing lost, nothing doubled
        got = run_pool_grad(dgf, w, adj)
        want = P.pool_grad32(dgf, w, adj)
        assert np.array_equal(_bits(got), _bits(want)), (case, name, float(np.mean(got != want)))
        # float32 sums of k terms: each partial sum is rounded once, |error| <= (k - 1) 2^-24 sum |terms| (1 + O(k 2^-24)) per
        # destination; over a channel's destinations that is the bound below, and float64 adds nothing visible to it
        k = P.pool_grad64(np.ones_like(dgf), w, adj)
        bound = (np.maximum(k - 1, 0) * 2.0 ** -24 * 1.001 * P.pool_grad64(np.abs(dgf), w, adj)).sum(1)
        s, t = _conserved(got, dgf, w)
        assert (np.abs(s - t) <= bound + 1e-12 * np.abs(dgf).astype(np.float64).sum(1)).all(), (case, name)


@pytest.mark.parametrize("case", P.GMAX_SHAPES, ids=lambda k: "%dx%dx%d" % k)
def test_global_maximum_takes_the_first_maximal_row(case):
    """tb_gmax_kernel (fold_train.hip's copy): the first row that attains the maximum of a * inv + shift, with ties in every row
    phase, a first maximum in phase 3 with its copy in phase 0 one row later, n below 4 and no multiple of 4, inv of both signs
    and 0, and a column whose maximum is a zero of either sign (the first row's sign is kept)."""
    a, inv, shift = _cases("gmax")[case]
    want_pooled, want_arg = P.gmax(a, inv, shift)
    pooled, arg = run_gmax(a, inv, shift)
    assert np.array_equal(arg, want_arg), (case, float(np.mean(arg != want_arg)))
    assert np.array_equal(_bits(pooled), _bits(want_pooled)), case


def test_entries_refuse_null_pointers_and_sizes_outside_the_trainers():
    from geometric_adv_amd import _lib, ops
    L = _lib.lib()
    f = torch.zeros(64 * 17, dtype=torch.float32, device=DEV)
    i = torch.zeros(64 * 17, dtype=torch.int32, device=DEV)
    p, q, st = f.data_ptr(), i.data_ptr(), _lib.stream_handle()

    def refused(rc, word):
        assert rc != 0
        assert word in L.geoadv_last_error().decode(), (word, L.geoadv_last_error())

    with torch.cuda.device(DEV):
        refused(L.geoadv_fold_train_pool(1, 17, 4, None, q, p, q, st), "null")
        refused(L.geoadv_fold_train_pool(1, 17, 4, p, q, p, None, st), "null")
        refused(L.geoadv_fold_train_pool_grad(1, 17, 4, p, q, q, q, None, p, st), "null")
        refused(L.geoadv_fold_train_gmax(1, 17, 4, p, p, None, p, q, st), "null")
        for call in (lambda b, n, c: L.geoadv_fold_train_pool(b, n, c, p, q, p, q, st),
                     lambda b, n, c: L.geoadv_fold_train_pool_grad(b, n, c, p, q, q, q, q, p, st),
                     lambda b, n, c: L.geoadv_fold_train_gmax(b, n, c, p, p, p, p, q, st)):
            refused(call(0, 17, 4), "[1, 1024]")
            refused(call(1025, 17, 4), "[1, 1024]")
            refused(call(1, 0, 4), "n 0")
            refused(call(9, 16384, 4), "2^17")
            refused(call(1, 17, 0), "c 0")
        torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.fold_train_pool(1, 17, 4, f, f, f, i)              # cols must be int32
    assert (f.cpu().numpy() == 0).all() and (i.cpu().numpy() == 0).all()          # nothing was launched
