"""The rules of geoadv_sor_filter and geoadv_random_drop (include/geoadv.h) restated in numpy, bit for bit: the float64
statistics of SOR in the kernel's fixed summation order, the packing, and the counter-based draws of SRS in the uint64 style of
tests/_batch_noise64.py.  Every function works on a batch of clouds at once (the leading axis), cloud by cloud the same
arithmetic."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _batch_noise64 import G, mix  # noqa: E402

T = 1024                  # threads of the workgroup that sums a cloud (include/geoadv.h)
WAVE = 64
SRS_STREAM = 48


def fixed_order_sum(terms):
    """SUM of the rule over float64 terms [b, n] -> [b]: partial sums by p mod T added sequentially from +0.0, the xor
    butterfly within every wave of 64, the waves in ascending order."""
    terms = np.asarray(terms, np.float64)
    b, n = terms.shape
    rows = -(-n // T)
    # a thread without a point keeps its +0.0, and so does a wave of such threads: x + 0.0 has x's bits (x is never -0.0 here:
    # every partial sum starts at +0.0), so for n < T only the waves that hold points are formed
    threads = T if n >= T else -(-n // WAVE) * WAVE
    padded = np.zeros((b, rows * threads), np.float64)
    padded[:, :n] = terms
    padded = padded.reshape(b, rows, threads)
    acc = np.zeros((b, threads), np.float64)
    for row in range(rows):
        acc = acc + padded[:, row]
    v = acc.reshape(b, threads // WAVE, WAVE)
    lane = np.arange(WAVE)
    for m in (1, 2, 4, 8, 16, 32):
        v = v + v[:, :, lane ^ m]
    total = v[:, 0, 0]
    for w in range(1, threads // WAVE):
        total = total + v[:, w, 0]
    return total


def sor_scores(knn, k):
    """s_p of the rule from knn [b, n, stride] float32: a left-to-right float64 sum of the first k columns, over k."""
    knn = np.asarray(knn, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = knn[:, :, 0].astype(np.float64)
        for j in range(1, k):
            s = s + knn[:, :, j].astype(np.float64)
        return s / np.float64(k)


def dyadic_scores(n, seed):
    """n scores that are multiples of 2^-10 in [0, 32) whose mean is a multiple of 2^-10 too, with (n >= 3) one point exactly at
    the mean: every partial sum of the scores and of the squared deviations (multiples of 2^-20 below 2^10, at most 2^15 of
    them) is exact in float64 in any order, so mu is exact and var the correctly rounded quotient."""
    u = np.random.default_rng(seed).integers(0, 4096, size=n)
    u[-1] = (-int(u[:-1].sum())) % n                      # sum = 0 mod n: an integer mean (in units of 2^-10)
    if n >= 3:
        mean = int(u.sum()) // n
        i, j = np.argsort(u[:-1], kind="stable")[-2:]     # the two largest: u[i] + u[j] >= mean unless the last point is huge
        if u[i] + u[j] >= mean:
            u[i], u[j] = mean, u[i] + u[j] - mean         # same sum, one point at the mean
    return u.astype(np.float64) / 1024.0


def sor_stats(scores):
    """(mu [b], var [b], m [b] int64) of the rule from float64 scores [b, n]."""
    scores = np.asarray(scores, np.float64)
    fin = np.isfinite(scores)
    m = fin.sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mu = np.where(m > 0, fixed_order_sum(np.where(fin, scores, 0.0)) / m.astype(np.float64), 0.0)
        d = scores - mu[:, None]
        sq = np.where(fin, d * d, 0.0)
        var = np.where(m >= 2, fixed_order_sum(sq) / (m.astype(np.float64) - 1.0), 0.0)
    return mu, var, m


def sor_inliers(scores, alpha):
    """-> (inlier mask [b, n], (mu, var, m))."""
    scores = np.asarray(scores, np.float64)
    mu, var, m = sor_stats(scores)
    alpha = np.float64(alpha)
    bound = (alpha * alpha) * var
    with np.errstate(invalid="ignore", over="ignore"):
        d = scores - mu[:, None]
        inl = np.isfinite(scores) & ((scores <= mu[:, None]) | (d * d <= bound[:, None]))
    return inl, (mu, var, m)


def pack(pc, mask):
    """The points of pc [b,n,3] with mask [b,n], per cloud in point order and padded with the last of them (zeros if none)
    -> (packed [b,n,3], idx [b,n] int64 zero-padded, count [b])."""
    b, n, _ = pc.shape
    order = np.argsort(~mask, axis=1, kind="stable")      # the masked points first, both halves in point order
    count = mask.sum(axis=1)
    slot = np.arange(n)[None, :]
    src = np.where(slot < count[:, None], order, np.take_along_axis(order, np.maximum(count - 1, 0)[:, None], axis=1))
    out = np.take_along_axis(pc, src[:, :, None], axis=1)
    out[count == 0] = 0
    return out, np.where(slot < count[:, None], order, 0), count


def sor_filter(pc, knn, k, alpha):
    """geoadv_sor_filter on pc [b,n,3], knn [b,n,stride] -> (outlier_pc, outlier_idx int16, outlier_num int16, inlier_pc,
    stats [b,3] float64)."""
    pc = np.asarray(pc, np.float32)
    inl, (mu, var, m) = sor_inliers(sor_scores(knn, k), alpha)
    o_pc, o_idx, o_num = pack(pc, ~inl)
    i_pc = pack(pc, inl)[0]
    return o_pc, o_idx.astype(np.int16), o_num.astype(np.int16), i_pc, np.stack([mu, var, m.astype(np.float64)], axis=1)


def srs_draws(seed, counter, slots, n):
    """r(p) of the rule, uint64 [len(slots), n]."""
    with np.errstate(over="ignore"):
        s = np.asarray(slots, dtype=np.uint64)[:, None]
        p = np.arange(n, dtype=np.uint64)[None, :]
        key0 = mix(mix(np.uint64(seed) + G) ^ np.uint64(counter))
        return mix(mix(key0 ^ ((s << np.uint64(32)) | p)) + np.uint64(SRS_STREAM) * G)


def srs_dropped(seed, counter, slots, n, drop):
    """The dropped points of every slot, ascending: int32 [len(slots), drop] -- the drop smallest (r(p), p)."""
    r = srs_draws(seed, counter, slots, n)
    order = np.argsort(r, axis=1, kind="stable")           # stable: equal draws (there are none) in ascending p
    return np.sort(order[:, :drop], axis=1).astype(np.int32)


def random_drop(pc, drop, seed, counter=0, slot_offset=0):
    """geoadv_random_drop on pc [b,n,3] -> (kept [b,n,3], dropped_idx int32 [b,drop])."""
    pc = np.asarray(pc, np.float32)
    b, n, _ = pc.shape
    dropped = srs_dropped(seed, counter, np.arange(b, dtype=np.uint64) + np.uint64(slot_offset), n, drop)
    mask = np.ones((b, n), bool)
    np.put_along_axis(mask, dropped.astype(np.int64), False, axis=1)
    return pack(pc, mask)[0], dropped
