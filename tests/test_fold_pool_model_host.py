"""CPU: the inputs of tests/test_gpu_fold_train_kernels.py (built by tests/_fold_pool_model.py) can tell a right kernel from a
wrong one.  Each near miss of a rule is stated here in numpy and must change at least SHARE of the elements of the model's
output on at least one of the GPU test's own inputs; the gather summed in descending order must change at least one bit of a
float32 result.  An input that does not discriminate is a reason to change the input, never the bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fold_pool_model as P  # noqa: E402

SHARE = 0.01


def _wrong_pool(h, cols, rule):
    """The pool with one rule stated wrongly -> win."""
    win = np.full(h.shape, -1, np.int32)
    for k in range(h.shape[0]):
        rows, cand = P.candidates(h[k], cols[k])
        if rule == "last_slot":                 # the point itself first, then the HIGHEST slot
            order = np.r_[0, np.arange(P.K, 0, -1)]
        elif rule == "neighbours_first":        # the slots in order, the point itself last
            order = np.r_[np.arange(1, P.K + 1), 0]
        elif rule == "greater_equal":           # u >= v: the LAST candidate that attains the maximum
            order = np.arange(P.K, -1, -1)
        else:
            order = np.arange(P.K + 1)
        rows, cand = rows[:, order], cand[:, order]
        first = np.argmax(cand, axis=1)
        best = np.take_along_axis(cand, first[:, None, :], 1)[:, 0, :]
        who = np.take_along_axis(rows, first.reshape(len(rows), -1), 1).reshape(first.shape)
        win[k] = who if rule == "no_positivity" else np.where(best > 0, who, -1)
    return win


@pytest.mark.parametrize("rule", ["last_slot", "neighbours_first", "greater_equal", "no_positivity"])
def test_pool_inputs_tell_the_winner_rule_from(rule):
    worst = 0.0
    for name, h, cols in P.pool_cases():
        _, win = P.pool(h, cols)
        assert np.array_equal(_wrong_pool(h, cols, "none"), win), name       # the harness itself restates the rule
        worst = max(worst, float(np.mean(_wrong_pool(h, cols, rule) != win)))
    assert worst >= SHARE, (rule, worst)


def test_pool_inputs_have_what_they_claim():
    for (b, n, c, kind), h, cols in P.pool_cases():
        g, win = P.pool(h, cols)
        assert cols.min() >= 0 and cols.max() < n
        own = cols == np.arange(n)[None, :, None]
        assert own.any() and any(len(set(r)) < P.K for r in cols.reshape(-1, P.K))         # self slots, repeated slots
        assert (g[win < 0] == 0).all() and not np.signbit(g[win < 0]).any()
        assert (g[win >= 0] > 0).all()
        if kind == "signed":
            assert np.signbit(h[h == 0]).any() and not np.signbit(h[h == 0]).all()          # -0.0 and +0.0
            assert 0.2 < np.mean(win < 0) < 0.8
        if kind == "distinct":
            assert len(np.unique(h)) == h.size
        if kind == "tied":
            rows, cand = P.candidates(h[0], cols[0])
            assert np.mean((cand == cand.max(1, keepdims=True)).sum(1) > 1) > 0.5             # most maxima are attained twice


def test_adjacency_is_symmetric_sorted_and_has_its_hub():
    for (b, n, c, with_self), adj, win, _, _ in P.grad_cases():
        off, deg, col = P.csr(adj)
        assert deg.reshape(b, n).sum(1).max() <= 32 * n
        assert deg[b - 1, 0] == n - 1 + int(with_self)
        if n >= 300:
            assert deg[b - 1, 0] > 64
        for k in range(b):
            for j, row in enumerate(adj[k]):
                assert np.array_equal(row, np.unique(row)) and ((j in row) == with_self)
                assert all(j in adj[k][i] for i in row)
                assert np.array_equal(col[k, off[k, j]:off[k, j] + deg[k, j]], row)
        # many sources share a destination, and every source lies in its destination's row
        w = win[b - 1]
        src = np.flatnonzero((w[:, 0] >= 0) & (w[:, 0] != np.arange(n)))
        assert all(i in adj[b - 1][w[i, 0]] for i in src)
        assert np.bincount(w[:, 0][w[:, 0] >= 0], minlength=n).max() >= 3


def test_grad_inputs_tell_the_self_term_counted_twice_and_the_descending_order():
    twice, bits = 0.0, 0
    for (b, n, c, with_self), adj, win, dgi, dgf in P.grad_cases():
        right = P.pool_grad64(dgi, win, adj)
        assert np.array_equal(P.pool_grad32(dgi, win, adj), right)                              # integers: every order is exact
        assert np.array_equal(right.sum(1), np.where(win >= 0, dgi, 0).astype(np.float64).sum(1))
        wrong = P._scatter(dgi, win, adj, np.float64, self_twice=True)
        assert with_self or np.array_equal(wrong, right)
        twice = max(twice, float(np.mean(wrong != right)))
        up, down = P.pool_grad32(dgf, win, adj), P._scatter(dgf, win, adj, np.float32, descending=True)
        bits += int((up.view(np.int32) != down.view(np.int32)).sum())
        assert np.abs(up - P.pool_grad64(dgf, win, adj)).max() <= 2.0 ** -23 * n * np.abs(dgf).max()
    assert twice >= SHARE, twice
    assert bits >= 1, bits


def _wrong_gmax(a, inv, shift, rule):
    v = P.pre(a, inv, shift)
    n = v.shape[1]
    if rule == "last_row":
        return n - 1 - np.argmax(v[:, ::-1], axis=1)
    # "lowest_phase": each phase r % 4 keeps its first maximum; the merge takes the lowest PHASE that attains the maximum
    best = v.max(1)
    out = np.full(best.shape, -1, np.int64)
    for ph in range(min(4, n) - 1, -1, -1):
        sub = v[:, ph::4]
        first = ph + 4 * np.argmax(sub, axis=1)
        out = np.where(sub.max(1) == best, first, out)
    return out


@pytest.mark.parametrize("rule", ["last_row", "lowest_phase"])
def test_gmax_inputs_tell_the_first_row_from(rule):
    worst = 0.0
    for (b, n, c), a, inv, shift in P.gmax_cases():
        _, arg = P.gmax(a, inv, shift)
        worst = max(worst, float(np.mean(_wrong_gmax(a, inv, shift, rule) != arg)))
    assert worst >= SHARE, (rule, worst)


def test_gmax_inputs_have_what_they_claim():
    for (b, n, c), a, inv, shift in P.gmax_cases():
        pooled, arg = P.gmax(a, inv, shift)
        v = P.pre(a, inv, shift)
        assert (inv > 0).any() and (inv < 0).any() and (inv[::16] == 0).all()
        assert (arg[:, ::16] == 0).all() and np.array_equal(pooled[:, ::16], np.broadcast_to(shift[::16], (b, len(shift[::16]))))
        if c > 5:
            zero = v[:, :, 5] == 0
            assert (pooled[:, 5] == 0).all() or n < 3
            if n >= 1000:
                assert np.signbit(v[:, :, 5][zero]).any() and not np.signbit(v[:, :, 5][zero]).all()
                assert np.array_equal(np.signbit(pooled[:, 5]), np.signbit(v[np.arange(b), arg[:, 5], 5]))
        if n >= 5:
            cols = [k for k in range(3, c, 8) if inv[k] != 0 and k != 5]
            assert cols and (arg[:, cols] == 3).all() and (v[:, 4, cols] == pooled[:, cols]).all()      # phase 3 first, phase 0 tied later
        if n >= 1000:
            ties = (v == pooled[:, None, :])
            for ph in range(4):
                assert ties[:, ph::4].any(1).mean() > 0.9                                           # ties across all four phases
