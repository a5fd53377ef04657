"""The SURFACE rule of geoadv_knn_outlier_loss (GEOADV_KNN_LOSS_SURFACE, include/geoadv.h) restated in numpy, bit for bit, beside
the SOR rule's model (tests/_knn_loss_model.py: knn_vals, masked_edges; tests/_stat_defense_model.py: fixed_order_sum): from a
batch of clouds x [b,n,3] float32, the neighbour indices idx [b,n,k] (the search's, first column already dropped) and the
threshold the fp32 distances, the fp32 score of geoadv_outlier_filter, its mask, the float64 hinge and the gradient in the
rule's summation order.  Also the hub cloud of the tests."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_loss_model as M  # noqa: E402
import _stat_defense_model as S  # noqa: E402

MAX_K = 7
SEGMENT_CAP = 16                      # KL_SEGMENT_CAP of csrc/knn_loss.hip: in-degrees above it go through the hub queue


def dists(x, idx):
    """d [b,n,k] float32 = sqrtf(val), val the fp32 squared distance of tests/_knn_loss_model.knn_vals."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(M.knn_vals(x, idx)).astype(np.float32)


def scores(d, k):
    """s_p [b,n] float32: ((d0 + d1) + ...) / float32(k), left to right in fp32; no division for k = 1 (knn_score of
    csrc/defense.hip)."""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = d[:, :, 0].copy()
        for c in range(1, k):
            s = (s + d[:, :, c]).astype(np.float32)
        return (s / np.float32(k)).astype(np.float32) if k > 1 else s


def mask_of(score, thr):
    """w [b,n] bool: s_p > thr in fp32 (NaN: no; +inf: yes)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(score, np.float32) > np.float32(thr)


def gradient(x, idx, w, exact=False):
    """-> (grad [b,n,3] float32, G * scale [b,n,3] float64 before the rounding) of the rule: float64 accumulation of
    ((double)x_i - (double)x_other) / (double)d per edge, the gather term in column order, then the scatter term in the order of
    masked_edges; d = sqrtf of the fp32 squared distance
    recomputed from the edge's endpoint i; an edge with d == 0 adds nothing; one rounding to fp32.  exact=True (no part of the
    rule; for the comparison with float64 autograd): d is the float64 norm of the float64 difference instead."""
    x = np.asarray(x, np.float32)
    b, n, _ = x.shape
    k = idx.shape[2]
    out = np.zeros((b, n, 3), np.float32)
    out64 = np.zeros((b, n, 3), np.float64)
    scale = np.float64(1.0) / (np.float64(n) * np.float64(k))

    def unit(cloud, i, other):
        """the edges' contributions to endpoint i [e,3] float64 (zero rows where d == 0)"""
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            df = cloud[i] - cloud[other]                                           # fp32, from i's end
            sq = df * df
            d = np.sqrt(((sq[:, 0] + sq[:, 1]) + sq[:, 2]).astype(np.float32)).astype(np.float32)
            diff = cloud[i].astype(np.float64) - cloud[other].astype(np.float64)
            if exact:
                d = np.sqrt((diff * diff).sum(axis=1))
            u = diff / d.astype(np.float64)[:, None]
        u[d == 0] = 0.0
        return u

    with np.errstate(invalid="ignore", over="ignore"):
        for cl in range(b):
            nb = np.asarray(idx[cl], np.int64)
            G = np.zeros((n, 3), np.float64)
            own = np.flatnonzero(w[cl])
            for c in range(k):
                G[own] = G[own] + unit(x[cl], own, nb[own, c])
            src, dst = M.masked_edges(idx[cl], w[cl])
            order = np.argsort(dst, kind="stable")                                 # per target, the rule's order kept
            src, dst = src[order], dst[order]
            first = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]]) if len(dst) else np.zeros(0, np.int64)
            rank = np.arange(len(dst)) - np.repeat(first, np.diff(np.r_[first, len(dst)]))
            for r in range(int(rank.max()) + 1 if len(dst) else 0):                # the r-th source of every target at once
                e = rank == r
                G[dst[e]] = G[dst[e]] + unit(x[cl], dst[e], src[e])
            out64[cl] = G * scale
            out[cl] = out64[cl].astype(np.float32)
    return out, out64


def surface_loss(x, idx, k, thr):
    """-> dict(dist [b,n,k] f32, score32 [b,n] f32, score [b,n] f64 (the op's output), stats [b,4] f64 = thr, +0.0, the number of
    scores that are not NaN, the number masked, mask [b,n] bool, loss [b] f64, grad [b,n,3] f32, grad64 [b,n,3] f64: grad before its
    rounding).  thr is used as float32(thr)."""
    x = np.asarray(x, np.float32)
    idx = np.asarray(idx)
    assert idx.shape == x.shape[:2] + (k,) and 1 <= k <= MAX_K
    n = x.shape[1]
    thr = np.float32(thr)
    d = dists(x, idx)
    s32 = scores(d, k)
    s64 = s32.astype(np.float64)
    w = mask_of(s32, thr)
    with np.errstate(invalid="ignore", over="ignore"):
        loss = S.fixed_order_sum(np.where(w, s64 - np.float64(thr), 0.0)) / np.float64(n)
    b = x.shape[0]
    stats = np.stack([np.full(b, np.float64(thr)), np.zeros(b), (~np.isnan(s32)).sum(axis=1).astype(np.float64),
                      w.sum(axis=1).astype(np.float64)], axis=1)
    grad, grad64 = gradient(x, idx, w)
    return dict(dist=d, score32=s32, score=s64, stats=stats, mask=w, loss=loss, grad=grad, grad64=grad64)


# ---- the clouds of the tests --------------------------------------------------------------------------------------------------
def dodecahedron():
    """The 20 unit vertices (edge 0.714: at most three other vertices closer than the centre to any one)."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(a, b, c) for a in (-1.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)]
    for a in (-1.0 / g, 1.0 / g):
        for c in (-g, g):
            v += [(0.0, a, c), (a, c, 0.0), (c, 0.0, a)]
    v = np.array(v)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def hub_cloud(n, seed):
    """Four points at the origin, the 20 dodecahedron vertices, then a tight filler cluster at 10.  At k = 7 every vertex lists
    its three edge neighbours (0.714) and the four origin points (1.0), so with thr = 0.5 the 24 points are masked and the
    origin points have in-degrees above SEGMENT_CAP."""
    rng = np.random.default_rng(seed)
    filler = (rng.random((n - 24, 3), dtype=np.float32) * 0.05 + 10.0).astype(np.float32)
    return np.concatenate([np.zeros((4, 3), np.float32), dodecahedron(), filler]).astype(np.float32)


def cloud_of_kind(kind, n, seed):
    return hub_cloud(n, seed) if kind == "dodecahedron" else M.cloud_of_kind(kind, n, seed)
