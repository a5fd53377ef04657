"""The rules of three kernels of the FoldingNet training step (csrc/fold_train.hip, csrc/train_bn.h) stated in plain numpy, and the
inputs on which tests/test_gpu_fold_train_kernels.py holds the kernels to them bit for bit.  tests/test_fold_pool_model_host.py
shows on the CPU that these very inputs tell each rule from its near misses.

    pool(h, cols)              the graph pool: candidates = the point itself, then its 16 columns; the FIRST maximum wins
    pool_grad32 / pool_grad64  its backward as a SCATTER (the kernel gathers): every (i, c) with a winner adds dg[i, c] there
    gmax(a, inv, shift)        the first maximal row of a * inv + shift (two rounded float32 operations) and its value

None of them restates a kernel's loop: the maxima are np.argmax (first occurrence), the backward runs over sources, not
destinations."""
import numpy as np

K = 16          # columns per point (FT_NB)


# ---- the rules ------------------------------------------------------------------------------------------------------------------
def candidates(h, cols):
    """(rows (n, 17), values (n, 17, c)) of one cloud: the point itself, then its columns in slot order."""
    n = h.shape[0]
    rows = np.concatenate([np.arange(n)[:, None], np.asarray(cols, np.int64)], 1)
    return rows, h[rows]


def pool(h, cols):
    """h (b, n, c) float32, cols (b, n, 16) rows of the same cloud -> g (b, n, c) float32, win (b, n, c) int32: g = the maximum
    of the candidates where it is > 0, else +0; win = the row of the first candidate that attains it, or -1."""
    h = np.asarray(h, np.float32)
    g, win = np.zeros(h.shape, np.float32), np.full(h.shape, -1, np.int32)
    for k in range(h.shape[0]):
        rows, cand = candidates(h[k], cols[k])
        first = np.argmax(cand, axis=1)                                   # (n, c): first occurrence of the maximum
        best = np.take_along_axis(cand, first[:, None, :], 1)[:, 0, :]
        who = np.take_along_axis(rows, first.reshape(len(rows), -1), 1).reshape(first.shape)
        pos = best > 0
        g[k] = np.where(pos, best, np.float32(0))
        win[k] = np.where(pos, who, -1)
    return g, win


def _scatter(dg, win, adjacency, dtype, descending=False, self_twice=False):
    b, n, c = dg.shape
    dh = np.zeros((b, n, c), dtype)
    ch = np.arange(c)
    for k in range(b):
        member = np.zeros((n, n), bool)                     # member[j, i]: i is in j's row
        for j, row in enumerate(adjacency[k]):
            member[j, np.asarray(row, np.int64)] = True
        w = np.asarray(win[k], np.int64)
        own = w == np.arange(n)[:, None]
        dh[k][own] = dg[k][own].astype(dtype)               # the point itself first
        if self_twice:
            again = own & member[np.arange(n), np.arange(n)][:, None]
            dh[k][again] += dg[k][again].astype(dtype)
        for i in (range(n - 1, -1, -1) if descending else range(n)):      # then the other sources, in ascending order
            sel = (w[i] >= 0) & (w[i] != i)
            sel[sel] = member[w[i][sel], i]                 # a destination only sees the sources of its row
            dh[k][w[i][sel], ch[sel]] += dg[k][i][sel].astype(dtype)      # one channel each: no destination twice in one add
    return dh


def pool_grad32(dg, win, adjacency):
    """dg (b, n, c) float32, win (b, n, c), adjacency[k][j] = the sorted row of point j of cloud k -> dh (b, n, c) float32: every
    (i, c) with win >= 0 adds dg[i, c] to dh[win, c], each destination taking the point itself first and then the sources i of
    its row in ascending order, every sum rounded to float32."""
    return _scatter(np.asarray(dg, np.float32), win, adjacency, np.float32)


def pool_grad64(dg, win, adjacency):
    """The same scatter in float64 (the second opinion: exact where dg is integer-valued, whatever the order)."""
    return _scatter(np.asarray(dg, np.float32), win, adjacency, np.float64)


def pre(a, inv, shift):
    """a * inv + shift as the device forms it (tb_pre; the library is built without contraction): two rounded float32 operations."""
    return (np.asarray(a, np.float32) * np.asarray(inv, np.float32)).astype(np.float32) + np.asarray(shift, np.float32)


def gmax(a, inv, shift):
    """a (b, n, c) float32, inv / shift (c,) -> (pooled (b, c) float32, arg (b, c) int32): the first row of each cloud that attains
    the maximum of pre(a, inv, shift), and that row's value."""
    v = pre(a, inv, shift)
    arg = np.argmax(v, axis=1)
    return np.take_along_axis(v, arg[:, None, :], 1)[:, 0, :], arg.astype(np.int32)


# ---- the inputs of the kernel tests -----------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 17, 64), (3, 63, 128), (2, 300, 100), (2, 1000, 1)]
GMAX_SHAPES = [(2, 1, 64), (2, 3, 70), (3, 5, 1024), (2, 1001, 128), (1, 2048, 1024)]
POOL_INPUTS = ("tied", "signed", "distinct")


def build_adjacency(b, n, seed, with_self):
    """adjacency[k][j] = sorted unique row of point j: the symmetric closure of one random 16-member set per point (15 others and
    the point itself with_self, else 16 others; at n = 17 that is every other point).  Point 0 of the LAST cloud is a hub that
    every other point of its cloud lists: its degree is n - 1 (+ 1 with_self).  The degrees of a cloud sum to at most 32 n."""
    rng = np.random.default_rng(seed)
    others = K - 1 if with_self else K
    out = []
    for k in range(b):
        member = np.zeros((n, n), bool)
        for j in range(n):
            pool_ = np.delete(np.arange(n), j)
            mine = rng.choice(pool_, min(others, n - 1), replace=False)
            if k == b - 1 and j != 0 and 0 not in mine:
                mine[0] = 0                                 # the hub
            member[j, mine] = True
        member |= member.T
        member[np.arange(n), np.arange(n)] = with_self
        rows = [np.flatnonzero(member[j]).astype(np.int32) for j in range(n)]
        assert sum(len(r) for r in rows) <= 32 * n, "the CSR layout holds 32 n entries per cloud"
        assert k != b - 1 or len(rows[0]) == n - 1 + int(with_self)
        out.append(rows)
    return out


def csr(adjacency):
    """(off (b, n), deg (b, n), col (b, 32 n)) int32 in the layout of csrc/fold_graph.h; unused entries of col hold -7."""
    b, n = len(adjacency), len(adjacency[0])
    off, deg, col = np.zeros((b, n), np.int32), np.zeros((b, n), np.int32), np.full((b, 32 * n), -7, np.int32)
    for k, rows in enumerate(adjacency):
        at = 0
        for j, r in enumerate(rows):
            off[k, j], deg[k, j] = at, len(r)
            col[k, at:at + len(r)] = r
            at += len(r)
    return off, deg, col


def build_cols(adjacency, seed):
    """cols (b, n, 16) int32: 16 draws WITH replacement from each point's row (so slots repeat within a row), and every fifth
    slot on average replaced by the point itself.  Every column is a row of [0, n) and a member of the point's adjacency row or
    the point: by the symmetry of the adjacency every point that can pick j is in j's row."""
    rng = np.random.default_rng(seed)
    b, n = len(adjacency), len(adjacency[0])
    cols = np.zeros((b, n, K), np.int32)
    for k in range(b):
        for j in range(n):
            cols[k, j] = rng.choice(adjacency[k][j], K, replace=True)
            cols[k, j][rng.random(K) < 0.2] = j
    return cols


def pool_input(kind, b, n, c, seed):
    """h (b, n, c) float32.  "tied": drawn from {0, 0.25, 0.5, 1}, so that most maxima are attained more than once; "signed":
    mostly from {-1, -0.25, -0.0, +0.0} with a positive value in one element of 25, so that about half of the maxima are -0.0 or
    +0.0 (no winner) and the rest tied; "distinct": distinct random floats of both signs."""
    rng = np.random.default_rng(seed)
    if kind == "tied":
        return rng.choice(np.array([0, 0.25, 0.5, 1], np.float32), (b, n, c))
    if kind == "signed":
        h = rng.choice(np.array([-1, -0.25, -0.0, 0.0], np.float32), (b, n, c))
        return np.where(rng.random((b, n, c)) < 0.04, rng.choice(np.array([0.5, 1], np.float32), (b, n, c)), h)
    h = rng.permutation(b * n * c).astype(np.float32).reshape(b, n, c)
    return ((h - np.float32(b * n * c // 3)) / np.float32(b * n * c)).astype(np.float32)


def grad_input(kind, b, n, c, seed):
    """dg (b, n, c) float32: "integer" = whole numbers in [-8, 8] (every order of adding them is exact), "float" = normal draws."""
    rng = np.random.default_rng(seed)
    if kind == "integer":
        return rng.integers(-8, 9, (b, n, c)).astype(np.float32)
    return rng.standard_normal((b, n, c)).astype(np.float32)


def gmax_input(b, n, c, seed):
    """(a (b, n, c), inv (c,), shift (c,)) float32.  a is drawn from four values, so every column's maximum of a * inv + shift is
    attained in many rows of every phase r % 4; inv has both signs, is 0 in every 16th column (every row ties at shift: row 0)
    and 1 in column 5, where shift is -0.0 and a holds only -1, -0.0 and +0.0 (the maximum is a zero of either sign: its first row
    wins and its sign is kept).  From n = 5 on, the columns c % 8 == 3 are engineered: the maximum sits in row 3 (phase 3) and again
    in row 4 (phase 0) and nowhere before, so the phase merge must prefer the lower ROW, not the lower phase."""
    rng = np.random.default_rng(seed)
    values = np.array([-1, -0.5, 0.5, 1], np.float32)
    a = rng.choice(values, (b, n, c))
    inv = ((0.5 + rng.random(c)) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    shift = rng.standard_normal(c).astype(np.float32)
    inv[::16] = 0
    if c > 5:
        inv[5], shift[5] = 1, -0.0
        a[:, :, 5] = rng.choice(np.array([-1, -0.0, 0.0], np.float32), (b, n))
    if n >= 5:
        for col in range(3, c, 8):
            if inv[col] == 0 or col == 5:
                continue
            top = np.float32(1 if inv[col] > 0 else -1)     # the value of a whose image is the column's maximum
            tied = a[:, :, col] == top
            tied[:, 3:5] = False
            a[:, :, col][tied] = np.float32(0.5) * top
            a[:, 3:5, col] = top
            a[:, 5:, col][rng.random((b, n - 5)) < 0.3] = top     # and more copies further on
    return a, inv, shift


# ---- the cases themselves: the GPU test runs them, the host test shows that they discriminate ---------------------------------------
def pool_cases():
    """((b, n, c, kind), h, cols) for every shape and kind of input of the pool forward."""
    for si, (b, n, c) in enumerate(POOL_SHAPES):
        cols = build_cols(build_adjacency(b, n, 100 + si, with_self=False), 200 + si)
        for ki, kind in enumerate(POOL_INPUTS):
            yield (b, n, c, kind), pool_input(kind, b, n, c, 300 + 10 * si + ki), cols


def grad_cases():
    """((b, n, c, with_self), adjacency, win, integer dg, float dg) of the pool backward; win = the pool of a tied input over
    columns drawn from the adjacency, so many sources share a destination and every source lies in its destination's row."""
    for si, (b, n, c) in enumerate(POOL_SHAPES):
        for with_self in (True, False):
            adj = build_adjacency(b, n, 400 + si, with_self)
            _, win = pool(pool_input("tied", b, n, c, 600 + si), build_cols(adj, 500 + si))
            yield (b, n, c, with_self), adj, win, grad_input("integer", b, n, c, 700 + si), grad_input("float", b, n, c, 800 + si)


def gmax_cases():
    """((b, n, c), a, inv, shift) of the global maximum."""
    for si, (b, n, c) in enumerate(GMAX_SHAPES):
        yield ((b, n, c),) + gmax_input(b, n, c, 900 + si)
