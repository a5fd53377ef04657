"""The numpy model of farthest point sampling that csrc/sampling.hip is pinned to bit for bit (the rule of include/geoadv.h):
fp32 throughout, every product and sum rounded on its own, the largest distance wins and the LOWEST index among equals."""
import numpy as np


def fps(x, m, start=0):
    """x float32 (n,3), m picks, start index -> (idx (m,) int32, t (n,) float32 = the final squared distance to the chosen set)."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    start = int(start)
    if not 0 <= start < n:
        start = 0
    finite = np.isfinite(x).all(1)
    t = np.where(finite, np.float32(np.inf), np.float32(-1)).astype(np.float32)
    idx = np.empty(m, np.int32)
    cur = start
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(m):
            idx[s] = cur
            d = x - x[cur]
            d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            t = np.where((d < t) & finite, d, t)        # a NaN d never replaces t
            cur = int(np.argmax(t))                     # largest t, lowest index among equals
    return idx, t


def fps_batch(x, m, start=None):
    """fps over a batch (b,n,3) -> (idx (b,m) int32, sampled (b,m,3), t (b,n)); start None, an int or (b,) integers.
    The same arithmetic as fps, element for element, with the batch as one more array axis (tests/test_fps_host.py holds the two
    against each other)."""
    x = np.asarray(x, dtype=np.float32)
    b, n, _ = x.shape
    cur = np.zeros(b, np.int64) if start is None else np.broadcast_to(np.asarray(start, dtype=np.int64), (b,)).copy()
    cur[(cur < 0) | (cur >= n)] = 0
    finite = np.isfinite(x).all(2)
    t = np.where(finite, np.float32(np.inf), np.float32(-1)).astype(np.float32)
    idx = np.empty((b, m), np.int32)
    rows = np.arange(b)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(m):
            idx[:, s] = cur
            d = x - x[rows, cur][:, None, :]
            d = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
            t = np.where((d < t) & finite, d, t)
            cur = np.argmax(t, axis=1)
    return idx, x[rows[:, None], idx], t
