"""The neighbour lists of csrc/chamfer_lists.hip as a numpy float32 model: the build (every partner whose ANCHOR distance is below
tau = (sqrt(minimum) + skin)^2, at most `cap` of them), the certificate and the brute-force fallback.  Distances are the
reference's float32 arithmetic (tests/_chamfer_hard_clouds.dist32), the certificate is evaluated in float32 with the kernel's
margin; numpy's square root is correctly rounded where the kernel's is good to one ulp, which the margin covers (DESIGN 4,
'Neighbour lists'), so the two may decide a borderline query differently -- never its answer."""
import numpy as np

from _chamfer_hard_clouds import dist32, nn_model32

F = np.float32
MARGIN = F(2.0 ** -18)
TAU_MIN = F(2.0 ** -80)
BLOCK, BLOCK_CAP = 256, 64


def tau_of(dmin, skin):
    t = np.sqrt(np.asarray(dmin, F)) + F(skin)
    return (t * t).astype(F)


class Lists:
    """The lists of ONE cloud pair: rows[i] / cols[k] = index arrays (None: unlisted), tau_row, tau_col, the anchor."""

    def __init__(self, anchor, c, skin, cap=16, d1=None, d2=None):
        anchor, c = np.asarray(anchor, F), np.asarray(c, F)
        D = dist32(anchor, c)
        d1 = D.min(1) if d1 is None else np.asarray(d1, F)
        d2 = D.min(0) if d2 is None else np.asarray(d2, F)
        self.anchor, self.c, self.cap = anchor, c, cap
        self.tau_row, self.tau_col = tau_of(d1, skin), tau_of(d2, skin)
        self.rows, self.cols = [], []
        for i in range(anchor.shape[0]):
            k = np.flatnonzero(D[i] < self.tau_row[i])
            self.rows.append(k if 1 <= len(k) <= cap else None)
        for k in range(c.shape[0]):
            i = np.flatnonzero(D[:, k] < self.tau_col[k])
            self.cols.append(i if 1 <= len(i) <= cap else None)


def _lexmin(d, idx):
    """lowest index among the smallest distances"""
    best = d.min()
    return best, int(idx[d == best].min())


def query(L, moved):
    """-> dist1, idx1, dist2, idx2 of nn_distance(moved, L.c) and a dict: cert_row / cert_col (bool: answered from the list),
    unlisted_row / unlisted_col, flagged (a block of 256 queries refused more than 64)."""
    moved = np.asarray(moved, F)
    n, m = moved.shape[0], L.c.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        D = dist32(moved, L.c)
        dv = moved - L.anchor
        disp2 = ((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]).astype(F)
        disp = np.sqrt(disp2)
        dmax = F(np.nan) if np.isnan(disp2).any() else np.sqrt(disp2.max())
    d1, i1 = np.empty(n, F), np.empty(n, np.int32)
    d2, i2 = np.empty(m, F), np.empty(m, np.int32)
    cert_r, cert_c = np.zeros(n, bool), np.zeros(m, bool)

    def one(dist_line, lst, tau, move):
        if lst is not None:
            with np.errstate(invalid="ignore"):
                best, bi = _lexmin(dist_line[lst], lst) if not np.isnan(dist_line[lst]).all() else (F(np.inf), -1)
                st = np.sqrt(F(tau))
                ok = bi >= 0 and tau >= TAU_MIN and F(F(np.sqrt(F(best)) + F(move)) + F(MARGIN * st)) < st
            if ok:
                return best, bi, True
        return None

    for i in range(n):
        r = one(D[i], L.rows[i], L.tau_row[i], disp[i])
        cert_r[i] = r is not None
        d1[i], i1[i] = r[:2] if r else _brute(D[i])
    for k in range(m):
        r = one(D[:, k], L.cols[k], L.tau_col[k], dmax)
        cert_c[k] = r is not None
        d2[k], i2[k] = r[:2] if r else _brute(D[:, k])
    flagged = any((~cert_r[s:s + BLOCK]).sum() > BLOCK_CAP for s in range(0, n, BLOCK)) or \
        any((~cert_c[s:s + BLOCK]).sum() > BLOCK_CAP for s in range(0, m, BLOCK))
    info = dict(cert_row=cert_r, cert_col=cert_c, unlisted_row=np.array([x is None for x in L.rows]),
                unlisted_col=np.array([x is None for x in L.cols]), flagged=flagged)
    return d1, i1, d2, i2, info


def _brute(line):
    """strict '<' from index 0: the first minimum; index 0 where nothing is below +inf"""
    with np.errstate(invalid="ignore"):
        best, bi = F(np.inf), 0
        finite = np.flatnonzero(line < np.inf)
        if len(finite):
            bi = int(finite[np.argmin(line[finite])])
            best = line[bi]
    return best, bi


def reference(moved, c):
    d1, i1, d2, i2 = nn_model32(np.asarray(moved, F)[None], np.asarray(c, F)[None])
    return d1[0], i1[0], d2[0], i2[0]


# ---- the cases both test files share ------------------------------------------------------------------------------------------------
def uniform(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3), dtype=np.float32) - F(0.5)).astype(F)


def moved_by(a, seed, step):
    """every point moved by exactly `step` (to rounding) in a random direction"""
    v = np.random.default_rng(seed).standard_normal(a.shape)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return (a.astype(np.float64) + step * v).astype(F)


def duplicated(seed, b, n):
    """rows and columns in which every point occurs twice or more, and rows that sit exactly on columns: exact ties everywhere"""
    rng = np.random.default_rng(seed)
    base = (np.round(rng.random((b, max(2, n // 3), 3)) * 64) / 64 - 0.5).astype(F)          # short dyadic coordinates
    a = np.stack([base[u][rng.integers(0, base.shape[1], n)] for u in range(b)])
    c = np.stack([base[u][rng.integers(0, base.shape[1], n)] for u in range(b)])
    return a, c


def blob_and_far_column(seed, b, n):
    """a dense blob of rows (diameter below 0.007) against columns spread over the cube: at a skin of 0.01 every column farther
    than the skin from the blob has ALL n rows below its threshold"""
    rng = np.random.default_rng(seed)
    a = (0.004 * (rng.random((b, n, 3)) - 0.5)).astype(F)
    return a, uniform(seed + 1, b, n)


def _nudge(moved, row, axis, start, towards, c_in, c_out, which):
    """moves coordinate `axis` of moved[row] from `start` (where the two columns / rows are equidistant) by ulps until the outside
    partner is strictly closer / farther than the inside one ('equal': stays)"""
    x = F(start)
    moved[row, axis] = x
    d = lambda: (c_in(), c_out())
    di, do = d()
    assert di == do, "the meeting point is exact in float32"
    if which == "equal":
        return
    closer = which == "closer"
    for _ in range(64):
        x = np.nextafter(x, F(towards) if closer else F(-towards))
        moved[row, axis] = x
        di, do = d()
        if (do < di) if closer else (do > di):
            return
    raise AssertionError("no float32 step separates the two distances")


def boundary_case(seed, n, which, low_index):
    """One cloud pair with two gadgets, everything else far away.
    ROW gadget (at the origin): column `inside` is row 0's nearest at the anchor (1/16 away on +x); column `outside` lies at
    1/16 + 1/64 on -x, beyond tau = (1/16 + skin)^2 with skin = 1/128, so it is NOT in row 0's list.  Row 0 then moves along -x to
    where `outside` is one step closer than ('closer'), exactly as far as ('equal') or one step farther than ('farther') `inside`.
    COLUMN gadget (at y = 1): column 7 has row r_in 1/16 above it as its nearest and row r_out 1/16 + 1/64 below it, outside column
    7's list; r_out moves up to meet r_in's distance in the same three ways.
    low_index: the outside partner carries the lower index of the two (it must win the exact tie).  The certificates must refuse
    (the displacement eats the skin's slack) and the answers must be the brute-force ones.
    -> anchor (n, 3), c (n, 3), moved (n, 3), skin, dict(row=(0, inside, outside), col=(7, r_in, r_out))"""
    skin = 2.0 ** -7
    a = uniform(seed, 1, n)[0] * F(0.25) + F(3.0)             # everything else far away from both gadgets
    c = uniform(seed + 1, 1, n)[0] * F(0.25) - F(3.0)
    inside, outside = (5, 3) if low_index else (3, 5)
    r_in, r_out = (9, 4) if low_index else (4, 9)
    a[0] = (0, 0, 0)
    c[inside] = (2.0 ** -4, 0, 0)
    c[outside] = (-(2.0 ** -4 + 2.0 ** -6), 0, 0)
    c[7] = (0, 1, 0)
    a[r_in] = (0, 1 + 2.0 ** -4, 0)
    a[r_out] = (0, 1 - (2.0 ** -4 + 2.0 ** -6), 0)
    moved = a.copy()
    _nudge(moved, 0, 0, -(2.0 ** -7), -1.0, lambda: dist32(moved[:1], c[[inside]])[0, 0], lambda: dist32(moved[:1], c[[outside]])[0, 0], which)
    _nudge(moved, r_out, 1, 1 - 2.0 ** -4, 2.0, lambda: dist32(moved[[r_in]], c[[7]])[0, 0], lambda: dist32(moved[[r_out]], c[[7]])[0, 0], which)
    return a, c, moved, skin, dict(row=(0, inside, outside), col=(7, r_in, r_out))
