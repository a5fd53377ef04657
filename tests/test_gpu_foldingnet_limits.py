"""GPU: the FoldingNet graph build and forward (csrc/foldingnet.hip) across their chunk boundaries (min(1024, 2^17 / n)
clouds per chunk: 64 at n = 2048, 16 at 8192, 8 at 16384), at the ends of the accepted sizes (n 17 ... 16384) and on the
padded and degenerate clouds the defenses hand on, against the float64 model of tests/_fold_model64.py on the GPU's own
kNN.  Tolerance, error metric, weights and helpers are those of test_gpu_foldingnet.py.

Every call here goes through the C ABI with caller-made outputs: one guard cloud before and one after the range the call
may write, filled with a sentinel bit pattern (a NaN as float, no valid index as an integer).  After the call the guards
still hold the sentinel and no element in range does.

The float64 graph of the large clouds is _graph64 below (the covariances and the symmetric adjacency vectorised, the kNN in
row blocks); test_graph64_is_the_model_s pins it to _fold_model64's on a small cloud.  k = 17 sets: on the CPU, the float64
search with its distances formed in float32 (dx * dx + dy * dy + dz * dz) selects the float64 one's set at every
point of every cloud used here (n = 17 ... 16384), inside the existing 99.9 % cap.

Worst errors measured on the MI355X against float64 (the tests print each): across the chunk boundaries code 4.4e-7,
p1 2.8e-6, recon 3.7e-6; n 17 ... 16384 code 6.5e-7, p1 2.1e-6, recon 3.6e-6, the GPU's k = 17 sets equal to float64's
at every point; the padded cloud 4.2e-6; coincident points 2.8e-6.
"""
import ctypes

import numpy as np
import pytest

import _fold_model64 as M
from test_gpu_foldingnet import TOL, _ae, _clouds, _err, _state

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5A5A5               # int32; as a float a NaN, as an index or degree outside every valid range
PIECE = 7                           # split-invariance: pieces of 7 clouds (no chunk size is a multiple of 7)
OFFSET = 1000003                    # cloud_offset of the device-sampling runs


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _chunk(n):
    return min(1024, (1 << 17) // n)    # foldingnet.hip: fold_chunk, for a batch above it


def _guarded(planes, tail):
    import torch
    return torch.full((planes + 2,) + tuple(tail), SENTINEL, dtype=torch.int32, device="cuda:0")


def _unguard(bufs, floats):
    import torch
    torch.cuda.synchronize()
    out = {}
    for k, buf in bufs.items():
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "%s: a guard cloud was written" % k
        assert not bool((buf[1:-1] == SENTINEL).any()), "%s: an element in range was never written" % k
        out[k] = buf[1:-1].view(torch.float32) if k in floats else buf[1:-1]
    return out


def _workspace(ae, b, n):
    import torch
    from geometric_adv_amd import _lib
    return torch.empty(int(_lib.lib().geoadv_fold_workspace_bytes(ae.handle, b, n)), dtype=torch.uint8, device="cuda:0")


def _graph(ae, x):
    """geoadv_fold_graph into guarded outputs: degree (b, n), knn (b, n, 16) int32 and cov (b, n, 9) float32."""
    from geometric_adv_amd import _lib
    b, n = int(x.shape[0]), int(x.shape[1])
    bufs = {"degree": _guarded(b, (n,)), "knn": _guarded(b, (n, 16)), "cov": _guarded(b, (n, 9))}
    st = _lib.lib().geoadv_fold_graph(ae.handle, b, n, _lib.ptr(x), _lib.ptr(bufs["degree"][1:]), _lib.ptr(bufs["knn"][1:]),
                                      _lib.ptr(bufs["cov"][1:]), _lib.ptr(_workspace(ae, b, n)), _lib.stream_handle())
    _lib.check(st, "fold_graph")
    return _unguard(bufs, ("cov",))


def _forward(ae, x, picks=None, cloud_offset=0):
    """geoadv_fold_forward into guarded outputs: code (b, 512), p1, recon (b, 2025, 3) float32, picks and cols
    (2, b, n, 16) int32.  With `picks` (a (2, b, n, 16) int32 device tensor) in given mode, else device sampling with the
    object's seed and the ordinals cloud_offset + k."""
    from geometric_adv_amd import _lib
    b, n = int(x.shape[0]), int(x.shape[1])
    bufs = {"code": _guarded(b, (512,)), "p1": _guarded(b, (2025, 3)), "recon": _guarded(b, (2025, 3)),
            "cols": _guarded(2 * b, (n, 16))}
    if picks is None:
        bufs["picks"] = _guarded(2 * b, (n, 16))
        pk = bufs["picks"][1:]
    else:
        assert tuple(picks.shape) == (2, b, n, 16) and picks.is_contiguous()
        pk = picks
    st = _lib.lib().geoadv_fold_forward(ae.handle, b, n, _lib.ptr(x), 0 if picks is not None else 1,
                                        ctypes.c_ulonglong(ae.seed), ctypes.c_longlong(cloud_offset), _lib.ptr(pk),
                                        _lib.ptr(bufs["cols"][1:]), _lib.ptr(bufs["code"][1:]), _lib.ptr(bufs["p1"][1:]),
                                        _lib.ptr(bufs["recon"][1:]), _lib.ptr(_workspace(ae, b, n)), _lib.stream_handle())
    _lib.check(st, "fold_forward")
    out = _unguard(bufs, ("code", "p1", "recon"))
    for k in ("cols", "picks"):
        if k in out:
            out[k] = out[k].view(2, b, n, 16)
    return out


def _clouds_of(out, s, e):
    """The clouds [s, e) of every output of _forward / _graph (picks and cols are pool-layer major)."""
    return {k: (v[:, s:e] if k in ("picks", "cols") else v[s:e]) for k, v in out.items()}


def _sample(b, chunk, seed):
    """Clouds to compare with float64: the first, those around every chunk boundary, the first and last of the last chunk,
    a dozen random ones -- and, for each of these, the clouds a whole number of chunks before it, which a launcher that
    dropped or misapplied a chunk offset would have read or written instead."""
    s = {0, b - 1, (b - 1) // chunk * chunk}
    for k in range(chunk, b + chunk, chunk):
        s.update((k - 1, k, k + 1))
    s.update(int(v) for v in np.random.default_rng(seed).integers(0, b, 12))
    s = {c for c in s if 0 <= c < b}
    for c in list(s):
        s.update(range(c % chunk, c, chunk))
    return np.array(sorted(s))


def _separation(ref):
    """Smallest distance, in the tests' error metric, between the float64 outputs of two distinct sampled clouds."""
    flat = ref.reshape(len(ref), -1)
    d = np.array([[np.abs(p - q).max() for q in flat] for p in flat])
    d[np.diag_indices(len(d))] = np.inf
    return d.min() / max(1.0, np.abs(ref).max())


def _boxed_clouds(seed, b, n):
    """b clouds of n points, each uniform in a box of its own (centre within 0.3 of the origin, half sides 0.05 ... 0.2
    per axis) inside the unit cube: clouds that differ far more than two draws from the same cube do."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.3, 0.3, (b, 1, 3))
    half = rng.uniform(0.05, 0.2, (b, 1, 3))
    return (centre + half * (2 * rng.random((b, n, 3)) - 1)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ float64 graph, vectorised
def _knn64(x, dtype=np.float64):
    """(n, 17) the 17 nearest of every point of one cloud by squared distance formed in `dtype` as dx dx + dy dy + dz dz,
    ties by index: candidates from the expanded form in float64 (row blocks), then the exact differences."""
    x64 = np.asarray(x, np.float64)
    xt = np.asarray(x, dtype)
    n = len(x64)
    sq = (x64 ** 2).sum(1)
    out = np.empty((n, 17), np.int64)
    for r0 in range(0, n, 1024):
        blk = slice(r0, min(n, r0 + 1024))
        if n > 48:
            d = sq[blk, None] + sq[None, :] - 2.0 * (x64[blk] @ x64.T)
            cand = np.sort(np.argpartition(d, 47, axis=1)[:, :48], axis=1)
        else:
            cand = np.broadcast_to(np.arange(n), (blk.stop - blk.start, n))
        diff = xt[blk, None, :] - xt[cand]
        exact = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
        order = np.argsort(exact, axis=1, kind="stable")[:, :17]
        out[blk] = np.take_along_axis(cand, order, axis=1)
    return out


def _knn_agreement(x, knn):
    """Fraction of the points of cloud x whose 17-set (the point and the GPU's 16) is the float64 search's."""
    n = len(x)
    got = np.sort(np.concatenate([np.arange(n)[:, None], np.asarray(knn, np.int64)], axis=1), axis=1)
    return (got == np.sort(_knn64(x), axis=1)).all(axis=1).mean()


def _graph64(x, knn):
    """One cloud: (cov (n, 9) float32, deg (n,), starts (n + 1,), columns) -- np.cov(ddof=1) of the 16 neighbours and the
    sorted rows of the symmetric adjacency in CSR form, in float64 / exact integers."""
    x = np.asarray(x, np.float64)
    L = np.asarray(knn, np.int64)
    n = len(x)
    d = x[L] - x[L].mean(axis=1, keepdims=True)
    cov = (np.einsum("nka,nkb->nab", d, d) / 15.0).reshape(n, 9).astype(np.float32)
    src = np.concatenate([np.repeat(np.arange(n), 16), L.reshape(-1)])
    dst = np.concatenate([L.reshape(-1), np.repeat(np.arange(n), 16)])
    key = np.unique(src * n + dst)
    starts = np.searchsorted(key // n, np.arange(n + 1))
    return cov, np.diff(starts), starts, key % n


def _check_against_float64(x, idx, ordinals, g, out, tag):
    """Clouds idx of the host batch x against float64: g and out are the device outputs of _graph and _forward (device
    sampling at `ordinals`) for exactly these clouds.  Returns the float64 (code, recon)."""
    ae_seed = _ae().seed
    g = {k: v.cpu().numpy() for k, v in g.items()}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    codes, recs, worst = [], [], np.zeros(3)
    for j, c in enumerate(idx):
        cov, deg, starts, col = _graph64(x[c], g["knn"][j])
        assert np.array_equal(deg, g["degree"][j]), "%s: degrees of cloud %d" % (tag, c)
        scale = np.abs(cov).max(axis=1, keepdims=True)
        assert (np.abs(g["cov"][j] - cov) <= 1e-5 * scale).all(), "%s: covariances of cloud %d" % (tag, c)
        picks = M.device_picks(ae_seed, [ordinals[j]], deg[None])
        assert np.array_equal(out["picks"][:, j], picks[:, 0]), "%s: picks of cloud %d" % (tag, c)
        cols = col[starts[None, :-1, None] + picks[:, 0]]
        assert np.array_equal(out["cols"][:, j], cols), "%s: cols of cloud %d" % (tag, c)
        code, p1, rec = M.model(_state(), x[c:c + 1], cov[None], cols[:, None])
        worst = np.maximum(worst, (_err(out["code"][j:j + 1], code), _err(out["p1"][j:j + 1], p1),
                                   _err(out["recon"][j:j + 1], rec)))
        codes.append(code[0])
        recs.append(rec[0])
    print("%s: relative errors code %.2e p1 %.2e recon %.2e" % ((tag,) + tuple(worst)))
    assert worst.max() <= TOL
    return np.stack(codes), np.stack(recs)


def test_graph64_is_the_model_s():
    x = _clouds(1, 1, 300)
    knn = M.knn(x)
    assert np.array_equal(np.sort(_knn64(x[0])[:, 1:], axis=1), np.sort(knn[0], axis=1))
    cov, deg, starts, col = _graph64(x[0], knn[0])
    cov_m, rows = M.graph_from_knn(x, knn)
    assert np.allclose(cov, cov_m[0], rtol=1e-6, atol=1e-12) and np.array_equal(deg, M.degrees(rows)[0])
    picks = M.device_picks(3, [5], deg[None])
    assert np.array_equal(col[starts[None, :-1, None] + picks[:, 0]], M.resolve(rows, picks)[:, 0])


# ------------------------------------------------------------------------------------------------ chunk boundaries
@pytest.mark.parametrize("n,b", [(2048, 63), (2048, 64), (2048, 67), (2048, 131), (8192, 32), (8192, 35), (16384, 9)])
def test_chunk_boundary(n, b):
    """One graph call, one device-sampling forward at cloud_offset 1 000 003 and one given-picks forward over b clouds:
    no second chunk, a full chunk, a short second chunk, three chunks with a short last one at n = 2048 (chunk 64); the
    two and three chunks get_reconstructions' default batch makes at n = 8192 (chunk 16); two chunks at 16384 (chunk 8).

    1. every output of graph and forward equals, bit for bit, the same clouds run 7 at a time at the matching
       cloud_offset (a short piece launches other column slices: the launch shape must not show); the given-picks
       forward, fed the positions the device drew, returns the device run's cols, code, p1 and recon;
    2. the sampled clouds (_sample) against float64 on the GPU's own kNN: degrees, the device sampler's exact draws at
       the clouds' ordinals, the resolved columns, and code / p1 / recon within TOL;
    3. in float64 any two sampled clouds -- each boundary cloud and its counterparts one and two chunks earlier among
       them -- differ by more than 100 x TOL in the code and in the reconstruction (_boxed_clouds), so a neighbour's or
       another chunk's result cannot pass 2; their degrees and draws differ as well;
    4. the guards (_graph, _forward)."""
    import torch
    ae = _ae()
    chunk = _chunk(n)
    x = _boxed_clouds(n + b, b, n)
    xd = _dev(x)
    g = _graph(ae, xd)
    out = _forward(ae, xd, cloud_offset=OFFSET)
    for s in range(0, b, PIECE):
        e = min(b, s + PIECE)
        for name, whole, piece in (("graph", g, _graph(ae, xd[s:e])),
                                   ("forward", out, _forward(ae, xd[s:e], cloud_offset=OFFSET + s))):
            for k, v in _clouds_of(whole, s, e).items():
                assert torch.equal(piece[k], v), "%s %s differs from the run in pieces at clouds %d..." % (name, k, s)
    given_in = out["picks"].clone()
    given = _forward(ae, xd, picks=given_in)
    assert torch.equal(given_in, out["picks"])
    for k in ("cols", "code", "p1", "recon"):
        assert torch.equal(given[k], out[k]), "given picks: %s" % k
    idx = _sample(b, chunk, b)
    sel = torch.from_numpy(idx).to("cuda:0")
    pick = lambda d: {k: (v[:, sel] if k in ("picks", "cols") else v[sel]) for k, v in d.items()}
    code, rec = _check_against_float64(x, idx, idx + OFFSET, pick(g), pick(out), "n %d b %d" % (n, b))
    sep = (_separation(code), _separation(rec))
    print("n %d b %d: %d sampled clouds, separation code %.2e recon %.2e" % ((n, b, len(idx)) + sep))
    assert min(sep) > 100 * TOL


@pytest.mark.parametrize("n,total", [(8192, 35), (16384, 33)])
def test_get_reconstructions_does_not_depend_on_batch_size(n, total):
    """The default batch_size (32) makes two chunks per call at n = 8192 and four at 16384; batch_size 4 stays inside one."""
    x = _boxed_clouds(9 * n, total, n)
    r32 = _ae().get_reconstructions(x)
    ae4 = _ae(batch_size=4)
    r4 = np.concatenate([ae4.get_reconstructions(x[:5]), ae4.get_reconstructions(x[5:])])
    assert r32.shape == (total, 2025, 3) and np.isfinite(r32).all()
    assert np.array_equal(r32, r4)
    assert len(np.unique(r32.reshape(total, -1), axis=0)) == total


# ------------------------------------------------------------------------------------------------ size limits
@pytest.mark.parametrize("n", [17, 18, 63, 64, 65, 8192, 16384])
def test_point_count_limits_vs_float64(n):
    ae = _ae()
    b = 2
    x = _clouds(5000 + n, b, n)
    xd = _dev(x)
    g = _graph(ae, xd)
    knn = g["knn"].cpu().numpy()
    agree = np.mean([_knn_agreement(x[c], knn[c]) for c in range(b)])
    print("n %d: k = 17 sets equal to float64's on %.4f %% of the points" % (n, 100 * agree))
    assert agree > 0.999
    if n <= 65:                                   # the model's own graph as well
        _, rows = M.graph_from_knn(x, knn)
        assert np.array_equal(M.degrees(rows), g["degree"].cpu().numpy())
    out = _forward(ae, xd, cloud_offset=11)
    _check_against_float64(x, np.arange(b), np.arange(b) + 11, g, out, "n %d" % n)


# ------------------------------------------------------------------------------------------------ padded, degenerate
def test_padded_cloud_with_real_ties(oracle):
    """1900 distinct points padded to 2048 by repeating the last one (149 coincident points: hundreds of zero distances).
    Degrees, picks and cols equal the model built on the GPU's own kNN; the 16 neighbours' squared distances, recomputed
    in the oracle's arithmetic and sorted, are oracle.knn_point's k = 17 values with one zero removed (the point or a
    copy of it), bit for bit; the covariance of 16 identical neighbours is exactly zero."""
    ae = _ae()
    n0, n = 1900, 2048
    x = _clouds(77, 2, n0)
    x = np.concatenate([x, np.repeat(x[:, -1:], n - n0, axis=1)], axis=1)
    xd = _dev(x)
    g = _graph(ae, xd)
    knn, cov = g["knn"].cpu().numpy(), g["cov"].cpu().numpy()
    _, rows = M.graph_from_knn(x, knn)
    assert np.array_equal(M.degrees(rows), g["degree"].cpu().numpy())
    out = _forward(ae, xd, cloud_offset=3)
    assert np.array_equal(out["cols"].cpu().numpy(), M.resolve(rows, out["picks"].cpu().numpy()))
    _check_against_float64(x, np.arange(2), np.arange(2) + 3, g, out, "padded")
    val, _ = oracle.knn_point(17, x, x)
    assert not val[:, :, 0].any()
    d = np.stack([x[c][knn[c]] for c in range(2)]) - x[:, :, None, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    assert np.array_equal(np.sort(d2, axis=2), val[:, :, 1:])
    copies = np.arange(n0 - 1, n)
    assert (knn[:, copies] >= n0 - 1).all()
    assert not cov[:, copies].any()
    assert np.isfinite(out["recon"].cpu().numpy()).all()


@pytest.mark.parametrize("n", [17, 64, 2048])
def test_coincident_points_vs_float64(n):
    """Every distance is zero: any 16 neighbours are right; the graph is the model's on the GPU's kNN, the covariance
    exactly zero, the outputs finite and float64's within TOL."""
    ae = _ae()
    x = np.repeat(_clouds(8000, 2, 1), n, axis=1)
    xd = _dev(x)
    g = _graph(ae, xd)
    knn = g["knn"].cpu().numpy()
    assert (knn >= 0).all() and (knn < n).all() and not g["cov"].cpu().numpy().any()
    out = _forward(ae, xd, cloud_offset=5)
    assert all(np.isfinite(out[k].cpu().numpy()).all() for k in ("code", "p1", "recon"))
    _check_against_float64(x, np.arange(2), np.arange(2) + 5, g, out, "coincident n %d" % n)
