"""Hard inputs for the matrix-pipe-screened symmetric Chamfer scan (csrc/chamfer_mx.h), numpy only, no GPU: a float32 model of
nn_distance, a mirror of the kernel's chunk layout, and cloud generators that place exact ties, near ties, list loads, gaps and
scales ON CHOSEN BOUNDARIES of that layout (tests/test_chamfer_hard_clouds_host.py holds them to their claims on the CPU,
tests/test_gpu_chamfer_mx_hard.py runs the kernel on them).

THE LAYOUT MIRROR MUST MOVE WITH THE KERNEL'S.  `layout()` and `predict_lists()` restate compile-time facts of chamfer_mx.h:
    MX_WROWS = 256, MX_ROWS = 2048 (lines 56-57)        a wave owns 256 rows, a workgroup one row super-tile of 2048
    MX_ICAP = 160, MX_CCAP = 32 (lines 73-74)           rows / columns a wave can list before it redoes all of its own
    MX_ROW_IDMASK = 31, MX_COL_IDMASK = 127 (62-63)     32 row-direction chunks, 8 x 8 x 2 column-direction chunks
    accumulator register r of a lane = row 8 (r / 4) + 4 (lane / 32) + r % 4 of a 32-row tile (lines 34-36, 435), so a
        column-direction chunk is the 16 rows of (wave, row tile, lane half (row % 8) / 4) -- the key's id, line 341
    a row-direction chunk is "the columns 32 ct + lane % 32" of a stage, ct = 0 .. 7 (lines 36, 381-394): 8 columns, evaluated by
        a lane pair, the even column tiles by one lane and the odd ones by the other
    the column phase serves column c of a stage by thread 2 c: wave c / 32 (line 421), which is also whose list it joins
    eps, the bias and the candidate threshold (lines 207-227, 281-288)
and of the plan (chamfer_sym.hip: sym_shape): C columns a stage, S stages a workgroup, cslices column slices, rtiles row
super-tiles, all TAKEN from geoadv_debug_chamfer_sym_plan, never recomputed.  If the kernel's layout changes and this file does
not, the host test's class checks fail -- they do not go quietly vacuous.

The deterministic family (`constellations`).  Sites are distinct points of a lattice of spacing h = 1/16 in [-0.5, 0.5)^3; a
site hosts a few rows and columns at offsets 0, +-d e_x, +-d e_y, +-d e_z, 2 d e_y with d = 2^-10.  Every coordinate is a short
dyadic number, so equal distances are equal in float32 EXACTLY.  Columns [256 p, 256 p + 256) -- one stage of one workgroup -- live
in the lattice plane z = p % 16, plain columns at +d e_x of their site with their row at the site itself; a row that looks at
another stage's plane from outside sees the column straight below it first, and the next one 2 h d = 2^-13 or more later (more
than twice the kernel's reach of about 5e-5 there), so it is certified.  A tie is a site with several columns (row-direction
classes) or several rows (column-direction classes) at +-d e_z / +d e_y around the query; WHICH indices they carry decides the
class:
    rows:     a   two columns of one 8-column chunk and stage, column tiles of equal parity (one lane's descending select)
              a'  ... of different parity (the lane pair's exchange)
              b   different chunks of one stage (the row is listed)
              c   different stages of one workgroup (the 64-bit LDS minimum); needs S >= 2
              d   different column slices (the merge / the loss launch); needs cslices >= 2
              e   three columns: two as b, the third as c; needs S >= 2
    columns:  f   two rows of one 16-row chunk
              g   two chunks of one wave (the wave's SECOND candidate: sets `defer`)
              h   three chunks of one wave (the third is what the per-wave pair cannot hold)
              i   different waves
              j   different row super-tiles (the merge); needs rtiles >= 2
The candidates' positions rotate from instance to instance, so the lowest index takes each in turn.  `near=True` moves the
HIGHEST-index candidate of every tie nearer by 2^-24 along its axis -- the smallest step every site coordinate can take (one ulp
at 0.5; the next float below d itself is not representable once added to a site coordinate) -- which changes its squared
distance by 2^-33, five orders below eps: the reference then answers the highest index, and a kernel that trusts its
approximation answers another.

List loads (`capacity=True`, 2048 x 2048 only).  In wave w exactly k rows are class-b ties whose columns all lie in stage-plane
w, k = 152 ... 168 over the waves and clouds (MX_ICAP = 160 in the middle); with S >= 2, exactly k' = 28 ... 36 class g / h columns
fall among the 32 S columns one wave serves in a workgroup (MX_CCAP = 32).  The kernel reports no counts: the straddle rests on
construction.  `predict_lists()` backs it on the CPU: from the float32 distances and the kernel's own eps formula it counts, per
wave and workgroup, the queries that MUST be listed (an exact tie between chunks: the approximations differ by 2 eps at most) and
those that MAY be (second chunk not provably outside the reach); on these clouds the two counts agree, and the host test
asserts that they are the k and k' asked for.

The other families: `shell_and_cluster` (a cube of edge rho against a sphere shell around it: every gap scales with rho),
`scaled` (the data-derived scale at the edges of the kernel's sane range [2^-40, 2^40]) and `with_outlier` (one far point owns
the scale of the workgroups that see it).  All emit finite data only, so `nn_model32` needs no NaN rule."""

import numpy as np

from test_chamfer_sym_plan_host import _plan as _sym_plan

F = np.float32
H = 2.0 ** -4
D = 2.0 ** -10
STEP = 2.0 ** -24
MX_WROWS, MX_ROWS, MX_ICAP, MX_CCAP = 256, 2048, 160, 32
ROW_CLASSES = ("a", "a'", "b", "c", "d", "e")
COL_CLASSES = ("f", "g", "h", "i", "j")
EX, EY, EZ = np.eye(3)
TIE_OFFSETS = (D * EZ, -D * EZ, D * EY)


def plan_of(b, n, m):
    """The operator's plan for (b, n, m), read through geoadv_debug_chamfer_sym_plan (host only)."""
    from geometric_adv_amd import _lib
    return _sym_plan(_lib.lib(), np=1, b=b, n=n, m=m)          # (the package's own handle: it binds to the HIP runtime torch ships)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's arithmetic in float32
# ------------------------------------------------------------------------------------------------------------------------------
def dist32(a, c):
    """(n, 3), (m, 3) float32 -> (n, m) float32: d = ((dx*dx)+(dy*dy))+(dz*dz), every operation rounded to float32."""
    a, c = np.asarray(a, F), np.asarray(c, F)
    dx = a[:, None, 0] - c[None, :, 0]
    d = dx * dx
    dy = a[:, None, 1] - c[None, :, 1]
    d = d + dy * dy
    dz = a[:, None, 2] - c[None, :, 2]
    return d + dz * dz


def nn_model32(a, c):
    """(b, n, 3), (b, m, 3) -> dist1 (b, n), idx1, dist2 (b, m), idx2 as tf_nndistance.cpp:21-43 gives them: strict '<', so the first
    minimum wins (argmin).  Finite inputs only."""
    a, c = np.asarray(a, F), np.asarray(c, F)
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    d1, i1 = np.empty((b, n), F), np.empty((b, n), np.int32)
    d2, i2 = np.empty((b, m), F), np.empty((b, m), np.int32)
    for u in range(b):
        d = dist32(a[u], c[u])
        i1[u] = d.argmin(1); d1[u] = d[np.arange(n), i1[u]]
        i2[u] = d.argmin(0); d2[u] = d[i2[u], np.arange(m)]
    return d1, i1, d2, i2


# ------------------------------------------------------------------------------------------------------------------------------
# the layout
# ------------------------------------------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, plan, n, m):
        assert plan["screened"] == 1
        self.n, self.m = n, m
        self.C, self.S, self.rtiles, self.cslices = plan["C"], plan["S"], plan["rtiles"], plan["cslices"]
        self.SC = self.S * self.C

    def row(self, j):
        """-> dict of arrays: rt (row super-tile), wave, rtile (row tile of 32 in the wave), half (lane half), chunk (id of the
        16-row column-direction chunk inside the super-tile: wave << 4 | rtile << 1 | half, the kernel's key id)."""
        j = np.asarray(j)
        w, r, h = (j % MX_ROWS) // MX_WROWS, (j % MX_WROWS) // 32, ((j % 32) % 8) // 4
        return dict(rt=j // MX_ROWS, wave=w, rtile=r, half=h, chunk=(w << 4) | (r << 1) | h)

    def col(self, k):
        """-> dict of arrays: slice (workgroup), stage, chunk (the 8-column row-direction chunk k % 32), ctile (column tile of the
        stage; its parity is the lane of the pair that evaluates it), wave (which serves the column in the column phase)."""
        k = np.asarray(k)
        ct = (k % self.C) // 32
        return dict(slice=k // self.SC, stage=(k % self.SC) // self.C, chunk=k % 32, ctile=ct, wave=ct)

    def col_at(self, sl, st, ct, ch):
        return sl * self.SC + st * self.C + ct * 32 + ch

    def row_at(self, rt, w, r, h, a, b):
        return rt * MX_ROWS + w * MX_WROWS + r * 32 + 8 * a + 4 * h + b

    def row_class(self, cols):
        """The class of a row whose equidistant columns are `cols` (2 or 3 indices)."""
        c = self.col(np.sort(np.asarray(cols)))
        key = list(zip(c["slice"], c["stage"]))
        if len(cols) == 3:
            same = [key[0] == key[1], key[0] == key[2], key[1] == key[2]]
            ok = sum(same) == 1 and len(set(c["slice"])) == 1
            u, v = [(0, 1), (0, 2), (1, 2)][same.index(True)] if ok else (0, 0)
            return "e" if ok and c["chunk"][u] != c["chunk"][v] else None
        if c["slice"][0] != c["slice"][1]:
            return "d"
        if c["stage"][0] != c["stage"][1]:
            return "c"
        if c["chunk"][0] != c["chunk"][1]:
            return "b"
        return "a" if (c["ctile"][0] - c["ctile"][1]) % 2 == 0 else "a'"

    def col_class(self, rows):
        """The class of a column whose equidistant rows are `rows` (2 or 3 indices)."""
        r = self.row(np.sort(np.asarray(rows)))
        if len(rows) == 3:
            ok = len(set(r["rt"])) == 1 and len(set(r["wave"])) == 1 and len(set(r["chunk"])) == 3
            return "h" if ok else None
        if r["rt"][0] != r["rt"][1]:
            return "j"
        if r["wave"][0] != r["wave"][1]:
            return "i"
        return "g" if r["chunk"][0] != r["chunk"][1] else "f"


def layout(plan, n, m):
    return Layout(plan, n, m)


# ------------------------------------------------------------------------------------------------------------------------------
# which queries the kernel lists: must (exact tie between chunks) and may (second chunk not provably out of reach)
# ------------------------------------------------------------------------------------------------------------------------------
def _two_smallest(v, axis):
    p = np.partition(v, 1, axis=axis)
    return np.take(p, 0, axis=axis), np.take(p, 1, axis=axis)


def predict_lists(plan, a, c):
    """For one cloud pair: rows[lo|hi][rt, slice, wave] = listed (row, stage) items of the wave in that workgroup, and
    cols[lo|hi][rt, slice, wave] = deferred columns among those the wave serves.  lo counts what MUST be listed under the kernel's
    error bound (an exact float32 tie between the two best chunks: their approximations are within 2 eps), hi what MAY be (the
    second chunk is not provably outside the threshold 2 eps + 2^-15 v1, approximation errors and the keys' truncation included).
    Padding rows of a ragged last wave count into hi (their operands are neutralised, their keys nearly equal)."""
    L = Layout(plan, a.shape[0], c.shape[0])
    n, m = L.n, L.m
    a64, c64 = a.astype(np.float64), c.astype(np.float64)
    out = {k: np.zeros((L.rtiles, L.cslices, 8), np.int64) for k in ("rows_lo", "rows_hi", "cols_lo", "cols_hi")}
    d_all = dist32(a, c).astype(np.float64)
    for rt in range(L.rtiles):
        r0, r1 = rt * MX_ROWS, min(n, (rt + 1) * MX_ROWS)
        P = a64[r0:r1]
        lo, hi = P.min(0), P.max(0)
        cen = 0.5 * lo + 0.5 * hi
        for sl in range(L.cslices):
            c0, c1 = sl * L.SC, min(m, (sl + 1) * L.SC)
            Q = c64[c0:c1]
            re = np.maximum(hi - cen, cen - lo)
            ce = np.maximum(Q.max(0) - cen, cen - Q.min(0))
            big = max(re.max(), ce.max())
            assert 2.0 ** -40 <= big <= 2.0 ** 40
            s2 = (2.0 ** (13 - int(np.floor(np.log2(big))))) ** 2
            eps_box = 2.0 * float((re * re + ce * ce).sum()) * s2 * 1.0001 * 2.0 ** -18 + 32.0
            bias = 2.0 ** np.ceil(np.log2(2.0 * eps_box))
            rn2, cn2 = ((P - cen) ** 2).sum(1).max(), ((Q - cen) ** 2).sum(1).max()
            eps = 2.0 * (rn2 + cn2) * s2 * 1.0001 * 2.0 ** -18 + 32.0

            def reach(dmin):               # scaled units: the threshold + both approximation errors + the keys' truncation
                return 4.0 * eps + (s2 * dmin + bias + eps) * 2.0 ** -14

            for st in range(L.S):
                k0, k1 = c0 + st * L.C, min(c1, c0 + (st + 1) * L.C)
                if k0 >= k1:
                    break
                d = np.full((MX_ROWS, L.C), np.inf)
                d[:r1 - r0, :k1 - k0] = d_all[r0:r1, k0:k1]
                # rows: 32 chunks of the columns 32 ct + ch
                m1, m2 = _two_smallest(d.reshape(MX_ROWS, L.C // 32, 32).min(1), 1)
                real = np.arange(MX_ROWS) < r1 - r0
                must = real & (m2 == m1)
                may = ~real | ~(s2 * (m2 - m1) > reach(m1))
                out["rows_lo"][rt, sl] += must.reshape(8, MX_WROWS).sum(1)
                out["rows_hi"][rt, sl] += may.reshape(8, MX_WROWS).sum(1)
                # columns: 128 chunks of 16 rows (wave, row tile, lane half); deferred = some wave has TWO chunks in reach
                ch = d.reshape(8, 8, 4, 2, 4, L.C).min((2, 4)).reshape(8, 16, L.C)         # [wave, (rtile, half), column]
                best = ch.min((0, 1))
                w1, w2 = _two_smallest(ch, 1)                                               # per wave
                live = np.arange(L.C) < k1 - k0
                must_c = live & ((w2 == best[None]).any(0))
                may_c = live & (~(s2 * (w2 - best[None]) > reach(best)[None])).any(0)
                out["cols_lo"][rt, sl] += must_c.reshape(8, 32).sum(1)
                out["cols_hi"][rt, sl] += may_c.reshape(8, 32).sum(1)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the deterministic family
# ------------------------------------------------------------------------------------------------------------------------------
class Constellations:
    """a (clouds, n, 3), c (clouds, m, 3); classes[name] = [(cloud, 'row' | 'col', query, candidates), ...]; plain_rows /
    plain_cols = [(cloud, index array)]: queries with one neighbour at their site and the next one a lattice step away;
    capacity = {(cloud, 'row', wave, slice): k} and {(cloud, 'col', wave, slice): k'} for the list-load clouds; near = the ties are
    broken in favour of the highest index."""

    def __init__(self):
        self.a, self.c, self.classes, self.plain_rows, self.plain_cols, self.capacity, self.near = None, None, {}, [], [], {}, False


def _one_cloud(L, rng, near, capacity, ci, rep, out):
    n, m = L.n, L.m
    assert n <= 4096 and m <= 8192
    free_r, free_c = np.ones(n, bool), np.ones(m, bool)
    occ = None                       # (list-load clouds: the one set of sites every plane uses)
    gadgets = []                     # dict(dir, cls, rows=[...] / None, cols=[...] / None, roff, coff, query)

    def tie(direction, cls, members, others, inst, double_row=None):
        k = len(members)
        order = np.argsort(members)
        offs = [None] * k
        for pos, u in enumerate(order):                    # the candidates' positions rotate: the lowest index takes each in turn
            offs[u] = np.array(TIE_OFFSETS[(pos + inst) % k if k == 3 else (pos + inst) % 2], np.float64)
        if near:
            u = int(np.argmax(members))
            offs[u] = offs[u] * (1.0 - STEP / D)
        gadgets.append(dict(dir=direction, cls=cls, members=list(members), offs=offs, others=others, double_row=double_row))
        (free_c if direction == "row" else free_r)[list(members)] = False
        for o in ([] if others is None else others):
            (free_r if direction == "row" else free_c)[o] = False

    def draw_cols(cls):
        sl, st, ch, ct = rng.integers(L.cslices), rng.integers(L.S), rng.integers(32), rng.integers(8)
        if cls == "a":
            return [L.col_at(sl, st, ct, ch), L.col_at(sl, st, (ct + 2 * rng.integers(1, 4)) % 8, ch)]
        if cls == "a'":
            return [L.col_at(sl, st, ct, ch), L.col_at(sl, st, (ct + 1 + 2 * rng.integers(0, 4)) % 8, ch)]
        ch2 = (ch + rng.integers(1, 32)) % 32
        if cls == "b":
            return [L.col_at(sl, st, ct, ch), L.col_at(sl, st, rng.integers(8), ch2)]
        st2 = (st + rng.integers(1, max(2, L.S))) % L.S
        if cls == "c":
            return [L.col_at(sl, st, ct, ch), L.col_at(sl, st2, rng.integers(8), rng.integers(32))]
        if cls == "d":
            sl2 = (sl + rng.integers(1, max(2, L.cslices))) % L.cslices
            return [L.col_at(sl, st, ct, ch), L.col_at(sl2, rng.integers(L.S), rng.integers(8), rng.integers(32))]
        return [L.col_at(sl, st, ct, ch), L.col_at(sl, st, rng.integers(8), ch2), L.col_at(sl, st2, rng.integers(8), rng.integers(32))]

    def draw_rows(cls):
        rt, w, r, h = rng.integers(L.rtiles), rng.integers(8), rng.integers(8), rng.integers(2)
        a, b = rng.integers(4), rng.integers(4)
        any_ab = lambda: (rng.integers(4), rng.integers(4))
        if cls == "f":
            q = (4 * a + b + rng.integers(1, 16)) % 16
            return [L.row_at(rt, w, r, h, a, b), L.row_at(rt, w, r, h, q // 4, q % 4)]
        other = lambda: divmod((2 * r + h + rng.integers(1, 16)) % 16, 2)
        if cls == "g":
            (r2, h2) = other()
            return [L.row_at(rt, w, r, h, a, b), L.row_at(rt, w, r2, h2, *any_ab())]
        if cls == "h":
            c2 = rng.choice(16, 3, replace=False)
            return [L.row_at(rt, w, int(u) // 2, int(u) % 2, *any_ab()) for u in c2]
        if cls == "i":
            return [L.row_at(rt, w, r, h, a, b), L.row_at(rt, (w + rng.integers(1, 8)) % 8, rng.integers(8), rng.integers(2), *any_ab())]
        rt2 = (rt + rng.integers(1, max(2, L.rtiles))) % L.rtiles
        return [L.row_at(rt, w, r, h, a, b), L.row_at(rt2, rng.integers(8), rng.integers(8), rng.integers(2), *any_ab())]

    if capacity:
        assert n == 2048 and m == 2048
        # columns first (they take rows of the wave whose stage-plane they live in): k' of the 32 S columns one wave serves
        if L.S >= 2:
            for t in range(2):
                sl, v = (ci + t) % L.cslices, (ci + 4 * t) % 8
                kk = 28 + (2 * ci + t) % 9
                cand = [L.col_at(sl, st, v, ch) for ch in range(32) for st in range(L.S)]       # the stages alternate
                cols = [cand[u] for u in rng.permutation(len(cand))[:kk]] if L.S > 2 else cand[:kk]
                for u, k in enumerate(cols):
                    w = k // 256
                    cls = "h" if u % 4 == 3 else "g"
                    for _ in range(1000):
                        c2 = rng.choice(16, 3 if cls == "h" else 2, replace=False)
                        rows = [L.row_at(0, w, int(x) // 2, int(x) % 2, rng.integers(4), rng.integers(4)) for x in c2]
                        if free_r[rows].all():
                            break
                    else:
                        raise AssertionError("no free rows")
                    tie("col", cls, rows, [k], u)
                out.capacity[(ci, "col", v, sl)] = kk
        extra = sum(len(g["members"]) - 1 for g in gadgets)            # rows the column ties took beyond one a column
        ks = [152 + (ci * 8 + w) % 17 for w in range(8)]
        # A tie site holds two columns, so a plane of 256 columns leaves lattice sites empty -- and a row that looks at the plane over
        # an empty site has its four neighbours to choose from, often tied.  So every plane gets the SAME number n2 of two-column
        # sites (class-b ties, filled up with class-a ties, which are not listed: one chunk) and all planes use ONE set of 256 - n2
        # sites: no row ever stands over an empty one.  Rows: a site has one, a class-b site mostly two (j, j + 1 of one 4-row
        # group: the same 16-row chunk, so their columns stay certified); the rows left over look down from the planes above.
        doubles = [k // 2 for k in ks]
        n2 = max(max(k - y for k, y in zip(ks, doubles)), -(-(sum(doubles) + extra) // 8))
        assert n2 <= 100
        occ = [int(u) for u in rng.permutation(256)[:256 - n2]]
        for w in range(8):
            k, y = ks[w], doubles[w]
            x = k - 2 * y
            plane = np.arange(256 * w, 256 * w + 256)
            for u in range(n2 - x - y):                                # the class-a fillers first: they need two columns of one chunk
                ch = next(q for q in rng.permutation(32) if free_c[plane[plane % 32 == q]].sum() >= 2)
                k1, k2 = [int(q) for q in rng.choice(plane[(plane % 32 == ch) & free_c[plane]], 2, replace=False)]
                tie("row", L.row_class([k1, k2]), [k1, k2], None, u)
            pcols = [int(u) for u in rng.permutation(plane) if free_c[u]]
            pairs = [(j, j + 1) for j in range(256 * w, 256 * w + 256, 2) if free_r[j] and free_r[j + 1]]
            pairs = [pairs[u] for u in rng.permutation(len(pairs))]
            take = [pairs.pop() for _ in range(y)]
            lone = [j for j in range(256 * w, 256 * w + 256) if free_r[j] and not free_r[j ^ 1]] + [p_[0] for p_ in pairs]
            take += [(lone[u],) for u in range(x)]
            assert sum(len(t_) for t_ in take) == k
            for u, rows in enumerate(take):
                k1 = pcols.pop()
                k2 = next(q for q in pcols if q % 32 != k1 % 32)
                pcols.remove(k2)
                tie("row", "b", [k1, k2], [rows[0]], u, double_row=rows[1] if len(rows) == 2 else None)
                if len(rows) == 2:
                    free_r[rows[1]] = False
            out.capacity[(ci, "row", w, (256 * w) // L.SC)] = k
    else:
        hosts = dict(c=L.S >= 2, e=L.S >= 2, d=L.cslices >= 2, j=L.rtiles >= 2)
        for cls in ROW_CLASSES + COL_CLASSES:
            if not hosts.get(cls, True):
                continue
            is_row = cls in ROW_CLASSES
            limit, pool = (min(m, 4096), free_c) if is_row else (n, free_r)
            made = 0
            for _ in range(200 * rep):
                if made == rep:
                    break
                mem = [int(x) for x in (draw_cols(cls) if is_row else draw_rows(cls))]
                if len(set(mem)) < len(mem) or max(mem) >= limit or not pool[mem].all():
                    continue
                if (L.row_class(mem) if is_row else L.col_class(mem)) != cls:
                    continue
                tie("row" if is_row else "col", cls, mem, None, made)
                made += 1

    # the members a class does not name: any free index
    for g in gadgets:
        if g["others"] is None:
            pool = free_r if g["dir"] == "row" else free_c
            lim = np.flatnonzero(pool[:4096])
            if len(lim) == 0:
                g["others"] = []
                continue
            o = int(rng.choice(lim))
            pool[o] = False
            g["others"] = [o]
    # plain pairs: a row with a column of its own plane 256 p (the column then has its row inside every row super-tile that holds
    # the plane); what is left over, columns in plane order so that the rows go to the lowest planes
    fc, fr = np.flatnonzero(free_c), np.flatnonzero(free_r)
    fold = fc[fc >= 4096]
    fc = fc[fc < 4096]
    pairs, rest_r, rest_c = [], [], []
    for p in range(16):
        pr, pc = rng.permutation(fr[fr // 256 == p]), rng.permutation(fc[fc // 256 == p])
        k = min(len(pr), len(pc))
        pairs += list(zip(pr[:k].tolist(), pc[:k].tolist()))
        rest_r += pr[k:].tolist(); rest_c += pc[k:].tolist()
    fr, fc = rng.permutation(np.array(rest_r, np.int64)), np.array(rest_c, np.int64)
    npair = min(len(fc), len(fr))
    pairs += list(zip(fr[:npair].tolist(), fc[:npair].tolist()))
    lone_cols, lone_rows = fc[npair:].tolist(), fr[npair:].tolist()

    a, c = np.zeros((n, 3)), np.zeros((m, 3))
    xyz = lambda x, y, z: np.array([(x - 8) * H, (y - 8) * H, (z - 8) * H])
    # sites per lattice plane: everything anchored at a column of stage-plane p lives in z = p
    per = {}
    for g in gadgets:
        anchor = min(g["members"]) if g["dir"] == "row" else (g["others"][0] if g["others"] else None)
        per.setdefault(None if anchor is None else anchor // 256, []).append(("tie", g))
    for j, k in pairs:
        per.setdefault(k // 256, []).append(("pair", (j, k)))
    for k in lone_cols:
        per.setdefault(k // 256, []).append(("col", k))
    assert None not in per, "a column tie found no column"
    plain_r, plain_c, plain_sites = [], [], {}
    for p, items in per.items():
        assert len(items) <= 256
        holes = 256 - len(items)
        odd = [s for s in range(256) if s % 2 == 1]                # a hole's left neighbour (x - 1) is never a hole
        even = [s for s in range(256) if s % 2 == 0]
        odd = [odd[u] for u in rng.permutation(128)]
        used = even + odd[min(holes, 128):]
        used = [used[u] for u in rng.permutation(len(used))][:len(items)]
        if occ is not None:
            assert len(items) == len(occ), (p, len(items), len(occ))
            used = [occ[u] for u in rng.permutation(len(occ))]
        for s, (kind, it) in zip(used, items):
            o = xyz(s % 16, s // 16, p)
            if kind == "pair":
                a[it[0]] = o
                c[it[1]] = o + D * EX
                plain_r.append(it[0]); plain_c.append(it[1])
                plain_sites.setdefault(p, []).append((s, it[0]))
            elif kind == "col":
                c[it] = o + D * EX
            else:
                g = it
                tgt, oth = (c, a) if g["dir"] == "row" else (a, c)
                for u, off in zip(g["members"], g["offs"]):
                    tgt[u] = o + off
                for u in g["others"]:
                    oth[u] = o
                if g["double_row"] is not None:
                    a[g["double_row"]] = o + D * EX
                cand = tuple(sorted(g["members"]))
                if g["others"]:
                    out.classes.setdefault(g["cls"], []).append((ci, g["dir"], g["others"][0], cand))
                    if g["dir"] == "col":
                        plain_r.extend(g["members"])               # a tied row itself sees one column at its site
                    elif g["double_row"] is None:
                        plain_c.extend(g["members"])
                if g["double_row"] is not None:
                    out.classes.setdefault(g["cls"], []).append((ci, "row", g["double_row"], cand))
    # columns beyond the 16 planes: spares at 2 d e_y of a plain site (always another slice than the site's own column)
    for k in fold.tolist():
        sites = next((v for z, v in sorted(plain_sites.items()) if v), None)
        assert sites, "no plain site left for a spare column"
        s, j = sites.pop()
        c[k] = a[j] + 2 * D * EY
        plain_c.append(k)
        plain_r.remove(j)                                          # (its own column at d, the spare at 2 d: certified apart only by the slices)
    # rows without a column: at the sites of the planes no column uses, looking straight down
    if lone_rows:
        levels = [z for z in range(16) if z not in per]
        sites = list(range(256)) if occ is None else occ
        assert len(lone_rows) <= len(sites) * len(levels)
        for u, j in enumerate(lone_rows):
            s = sites[u % len(sites)]
            a[j] = xyz(s % 16, s // 16, levels[u // len(sites)])
    a32, c32 = a.astype(F), c.astype(F)
    assert np.array_equal(a32.astype(np.float64), a) and np.array_equal(c32.astype(np.float64), c), "a coordinate is not a float32"
    out.plain_rows.append((ci, np.array(sorted(plain_r), np.int64)))
    out.plain_cols.append((ci, np.array(sorted(plain_c), np.int64)))
    return a32, c32


def constellations(plan, n, m, seed, clouds=8, rep=12, near=False, capacity=False):
    """`clouds` distinct cloud pairs for one launch shape; rep instances of every class the shape can host per cloud (a class it
    cannot host is absent from .classes), or, with capacity=True, the list loads."""
    L = Layout(plan, n, m)
    out = Constellations()
    out.near = near
    A, Cc = [], []
    for ci in range(clouds):
        rng = np.random.default_rng([seed, ci, int(near), int(capacity)])
        a, c = _one_cloud(L, rng, near, capacity, ci, rep, out)
        A.append(a); Cc.append(c)
    out.a, out.c = np.stack(A), np.stack(Cc)
    return out


def hosted_classes(plan):
    no = set()
    if plan["S"] < 2:
        no |= {"c", "e"}
    if plan["cslices"] < 2:
        no.add("d")
    if plan["rtiles"] < 2:
        no.add("j")
    return [k for k in ROW_CLASSES + COL_CLASSES if k not in no]


# ------------------------------------------------------------------------------------------------------------------------------
# the gap sweep, the scale's edges, the outlier
# ------------------------------------------------------------------------------------------------------------------------------
C0 = np.array([0.3, -0.2, 0.25])


def shell_and_cluster(b, n, m, seed, log2_rho, swapped=False):
    """Rows in a cube of edge rho = 2^log2_rho around C0, columns on the sphere of radius 0.4 around C0 (swapped: rows on the shell,
    columns in the cube): every query sees the whole other cloud at nearly one distance, the best-to-second gap scales with rho."""
    rng = np.random.default_rng([seed, -log2_rho, int(swapped)])

    def cube(k):
        return C0 + (2.0 ** log2_rho) * (rng.random((b, k, 3)) - 0.5)

    def shell(k):
        v = rng.standard_normal((b, k, 3))
        return C0 + 0.4 * v / np.linalg.norm(v, axis=2, keepdims=True)

    a, c = (shell(n), cube(m)) if swapped else (cube(n), shell(m))
    return a.astype(F), c.astype(F)


def _unit_pair(kind, b, n, m, seed):
    rng = np.random.default_rng([seed, 7])
    if kind == "uniform":
        return (rng.random((b, n, 3)) - 0.5).astype(F), (rng.random((b, m, 3)) - 0.5).astype(F)
    assert kind == "sphere"
    v, w = rng.standard_normal((b, n, 3)), rng.standard_normal((b, m, 3))
    return ((0.5 * v / np.linalg.norm(v, axis=2, keepdims=True)).astype(F),
            (0.5 * w / np.linalg.norm(w, axis=2, keepdims=True)).astype(F))


def centred_big(a, c):
    """The kernel's `big` for a whole cloud pair (one workgroup sees all rows and a slice of the columns: its own value is this or
    slightly less): the largest |coordinate| after centring on the rows' bounding box."""
    lo, hi = a.min(0).astype(np.float64), a.max(0).astype(np.float64)
    cen = 0.5 * lo + 0.5 * hi
    return float(max(np.abs(a - cen).max(), np.abs(c - cen).max()))


def scaled(kind, log2_big, b, n, m, seed):
    """A uniform or sphere pair times a power of two such that every cloud's `big` is f * 2^log2_big with f in [1, 2)."""
    a, c = _unit_pair(kind, b, n, m, seed)
    for u in range(b):
        e = int(np.floor(np.log2(centred_big(a[u], c[u]))))
        a[u] *= F(2.0 ** (log2_big - e)); c[u] *= F(2.0 ** (log2_big - e))
        assert 2.0 ** log2_big <= centred_big(a[u], c[u]) < 2.0 ** (log2_big + 1)
    return a, c


def with_outlier(where, log2_far, b, n, m, seed):
    """A unit pair with ONE far point at distance 2^log2_far, in the rows, in the columns or in both (where = 'rows' | 'cols' |
    'both'), at an index drawn per cloud."""
    a, c = _unit_pair("uniform", b, n, m, seed)
    rng = np.random.default_rng([seed, 11, log2_far])
    far = F(2.0 ** log2_far)
    for u in range(b):
        d = rng.standard_normal(3)
        d = (d / np.linalg.norm(d)).astype(F)
        if where in ("rows", "both"):
            a[u, rng.integers(n)] = far * d
        if where in ("cols", "both"):
            c[u, rng.integers(m)] = -far * d if where == "both" else far * d
    return a, c
