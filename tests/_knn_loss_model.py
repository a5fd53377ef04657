"""The rule of geoadv_knn_outlier_loss (include/geoadv.h) restated in numpy, bit for bit, on top of the SOR rule's model
(tests/_stat_defense_model.py: fixed_order_sum, sor_scores, sor_stats): from a batch of clouds x [b,n,3] float32 and the
neighbour indices idx [b,n,k] (the search's, first column already dropped) the squared distances, the float64 scores and
statistics, the mask, the loss and the gradient in the rule's summation order.  Also the clouds the tests share."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stat_defense_model as S  # noqa: E402


def knn_vals(x, idx):
    """val [b,n,k] float32: ((dx*dx + dy*dy) + dz*dz) of x_p - x_idx[p][c], every product and sum rounded to fp32."""
    x = np.asarray(x, np.float32)
    b = x.shape[0]
    nb = x[np.arange(b)[:, None, None], np.asarray(idx, np.int64)]                 # [b,n,k,3]
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[:, :, None, :] - nb
        sq = d * d
        return ((sq[..., 0] + sq[..., 1]) + sq[..., 2]).astype(np.float32)


def mask_of(score, alpha):
    """-> (w [b,n] bool, (mu, var, m)): s finite and s > mu and (s - mu)(s - mu) > (alpha alpha) var."""
    score = np.asarray(score, np.float64)
    mu, var, m = S.sor_stats(score)
    alpha = np.float64(alpha)
    bound = (alpha * alpha) * var
    with np.errstate(invalid="ignore", over="ignore"):
        d = score - mu[:, None]
        w = np.isfinite(score) & (score > mu[:, None]) & (d * d > bound[:, None])
    return w, (mu, var, m)


def masked_edges(idx, w):
    """The edges (source p, target idx[p][c]) of one cloud's masked points in the rule's order: p ascending, within p c
    ascending -> (src, dst) int64."""
    k = idx.shape[1]
    src = np.repeat(np.flatnonzero(w), k)
    dst = np.asarray(idx, np.int64)[w].reshape(-1)
    return src, dst


def in_degree(idx, w):
    """[b,n] int64: how many masked edges end at each point."""
    b, n = w.shape
    return np.stack([np.bincount(masked_edges(idx[c], w[c])[1], minlength=n) for c in range(b)])


def gradient(x, idx, w):
    """grad [b,n,3] float32 of the rule: float64 accumulation, the gather term in column order, then the scatter term in the
    order of masked_edges, one rounding to fp32."""
    x = np.asarray(x, np.float32)
    b, n, _ = x.shape
    k = idx.shape[2]
    out = np.zeros((b, n, 3), np.float32)
    scale = np.float64(2.0) / (np.float64(n) * np.float64(k))
    with np.errstate(invalid="ignore", over="ignore"):
        for cl in range(b):
            x64 = x[cl].astype(np.float64)
            G = np.zeros((n, 3), np.float64)
            own = np.flatnonzero(w[cl])
            for c in range(k):
                G[own] = G[own] + (x64[own] - x64[np.asarray(idx[cl], np.int64)[own, c]])
            src, dst = masked_edges(idx[cl], w[cl])
            order = np.argsort(dst, kind="stable")                                 # per target, the rule's order kept
            src, dst = src[order], dst[order]
            first = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]]) if len(dst) else np.zeros(0, np.int64)
            rank = np.arange(len(dst)) - np.repeat(first, np.diff(np.r_[first, len(dst)]))
            for r in range(int(rank.max()) + 1 if len(dst) else 0):                # the r-th source of every target at once
                e = rank == r
                G[dst[e]] = G[dst[e]] + (x64[dst[e]] - x64[src[e]])
            out[cl] = (G * scale).astype(np.float32)
    return out


def knn_outlier_loss(x, idx, k, alpha):
    """-> dict(val [b,n,k] f32, score [b,n] f64, stats [b,4] f64 = mu, var, m, number masked, mask [b,n] bool, loss [b] f64,
    grad [b,n,3] f32)."""
    x = np.asarray(x, np.float32)
    idx = np.asarray(idx)
    assert idx.shape == x.shape[:2] + (k,)
    n = x.shape[1]
    val = knn_vals(x, idx)
    score = S.sor_scores(val, k)
    w, (mu, var, m) = mask_of(score, alpha)
    loss = S.fixed_order_sum(np.where(w, score, 0.0)) / np.float64(n)
    stats = np.stack([mu, var, m.astype(np.float64), w.sum(axis=1).astype(np.float64)], axis=1)
    return dict(val=val, score=score, stats=stats, mask=w, loss=loss, grad=gradient(x, idx, w))


def brute_idx(x, k):
    """The neighbours of a brute-force fp32 search on a batch: the k + 1 smallest squared distances of every row in a stable
    order, the first column dropped -> [b,n,k] int32."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[:, :, None, :] - x[:, None, :, :]
        sq = d * d
        d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    return np.argsort(d2, axis=2, kind="stable")[:, :, 1:k + 1].astype(np.int32)


# ---- the clouds of the tests --------------------------------------------------------------------------------------------------
def icosahedron():
    """The 12 unit vertices."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = []
    for a in (-1.0, 1.0):
        for c in (-g, g):
            v += [(0.0, a, c), (a, c, 0.0), (c, 0.0, a)]
    v = np.array(v)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def hub_cloud():
    """Five points at the origin, then the 12 icosahedron vertices: at k = 5 every vertex (1.05 from its nearest vertex, 1 from
    the origin) lists the five origin points."""
    return np.concatenate([np.zeros((5, 3), np.float32), icosahedron()])


def cloud_of_kind(kind, n, seed):
    """One cloud [n,3] float32 of a kind of tests/test_gpu_knn_loss.py."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (rng.random((n, 3), dtype=np.float32) - 0.5).astype(np.float32)
    if kind == "lattice":                                   # a 12^3 lattice (as much of it as fits) plus 10 planted far points:
        # a centre and nine satellites that each have the centre as their nearest neighbour (six along the axes at 0.50 .. 0.55,
        # three on diagonals at 0.3; any two satellites are farther apart than either is from the centre)
        g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32) / 16.0
        dirs = np.concatenate([np.eye(3), -np.eye(3), np.array([[-1, -1, -1], [1, 1, -1], [1, -1, 1]]) / np.sqrt(3.0)])
        radius = np.r_[0.50, 0.51, 0.52, 0.53, 0.54, 0.55, 0.3, 0.3, 0.3][:, None]
        far = (3.0 + np.concatenate([np.zeros((1, 3)), dirs * radius])).astype(np.float32)
        m = n - 10
        body = g[:m] if m <= len(g) else np.concatenate([g, (rng.random((m - len(g), 3), dtype=np.float32) * 0.6875).astype(np.float32)])
        return np.concatenate([body, far])[rng.permutation(n)].astype(np.float32)
    if kind == "hub":                                       # the hub case first, then a tight filler cluster far from it
        filler = (rng.random((n - 17, 3), dtype=np.float32) * 0.05 + 10.0).astype(np.float32)
        return np.concatenate([hub_cloud(), filler]).astype(np.float32)
    if kind == "equal":
        return np.full((n, 3), 0.375, np.float32)
    if kind == "pairs":                                     # the first half of the cloud holds every point twice (zero distances
        # and ties), the second half single points (so that the scores differ even at k = 1)
        q = n // 4
        half = (rng.random((q, 3), dtype=np.float32) - 0.5).astype(np.float32)
        rest = (rng.random((n - 2 * q, 3), dtype=np.float32) - 0.5).astype(np.float32)
        return np.concatenate([half, half, rest]).astype(np.float32)
    raise ValueError(kind)
