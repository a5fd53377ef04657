"""GPU: the PointNet classifier forward (csrc/classifier.hip) across its chunk boundary (65 535 clouds per chunk), at the
ends of its accepted sizes (n 1 ... 16384, 1 ... 1024 classes) and on the padded and degenerate clouds the defenses hand
on, against the float64 model of tests/_cls_model64.py.  Tolerance, error metric, weights and helpers are those of
test_gpu_classifier.py.

Every call here goes through the C ABI with caller-made outputs: one guard cloud before and one after the range the call
may write, all filled with a sentinel bit pattern (a NaN as float, far outside [0, 1024) as a label).  After the call the
guards still hold the sentinel and no element in range does.

MEMORY of the largest case (131 073 one-point clouds, both transforms): geoadv_cls_workspace_bytes is that of a full
chunk of 65 535 clouds, 3 005 435 392 bytes (pooled 3 x 65 535 x 4 KiB, T2 and the folded conv3 65 535 x 16 KiB each, the
folded conv1 and T1), the T2 output of 131 075 clouds 2 147 532 800 bytes, logits, T1 and labels 12 MB: 5.2 GB.  The
65 538 clouds of a second chunk of three need 4.1 GB.  (A byte count above 2^31 is also why the binding must declare the
workspace query as size_t: test_wrapper_sizes_a_workspace_above_2_GiB.)

Worst errors measured on the MI355X against float64 (the tests print each): across the chunk boundary (n = 1) logits
1.5e-6, T1 6.6e-7, T2 1.5e-6; n 1 ... 16384 logits 5.2e-5 (n = 65, b = 1), T1 5.0e-6, T2 5.5e-6; 1 ... 1024 classes
logits 4.3e-5, and 9.2e-5 with one class (a single logit of magnitude below 1: the metric is then absolute);
coincident points 2.7e-6.
"""
import functools

import numpy as np
import pytest

import _cls_model64 as M
from test_gpu_classifier import TOL, _clf, _clouds, _dev, _err, _weights

pytestmark = pytest.mark.gpu

CHUNK = 65535                       # classifier.hip: chunk_of
SENTINEL = 0x7FA5A5A5               # int32; as a float a NaN, as a label outside [0, 1024)
PIECE = 9973                        # split-invariance: pieces of this many clouds (a prime: never on the chunk grid)


def _guarded(b, tail):
    import torch
    return torch.full((b + 2,) + tuple(tail), SENTINEL, dtype=torch.int32, device="cuda:0")


def _check_guards(name, buf):
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "%s: a guard cloud was written" % name
    assert not bool((buf[1:-1] == SENTINEL).any()), "%s: an element in range was never written" % name


_WS = {}


def _workspace(need):
    import torch
    if "ws" not in _WS or _WS["ws"].numel() < need:
        _WS.pop("ws", None)
        _WS["ws"] = torch.empty(int(need), dtype=torch.uint8, device="cuda:0")
    return _WS["ws"]


def _forward(clf, x, logits=True, transforms=True):
    """geoadv_cls_forward on the device tensor x (b, n, 3) into guarded outputs; returns {name: device tensor} of the
    in-range parts (floats viewed as float32), after the guard checks."""
    import torch
    from geometric_adv_amd import _lib
    lib = _lib.lib()
    b, n = int(x.shape[0]), int(x.shape[1])
    bufs = {"labels": _guarded(b, ())}
    if logits:
        bufs["logits"] = _guarded(b, (clf.num_classes,))
    if transforms:
        bufs["t1"] = _guarded(b, (3, 3))
        bufs["t2"] = _guarded(b, (64, 64))
    p = lambda k: _lib.ptr(bufs[k][1:]) if k in bufs else None
    need = lib.geoadv_cls_workspace_bytes(clf.handle, b, n)
    assert need >= 3 * 4096 * min(b, CHUNK)
    st = lib.geoadv_cls_forward(clf.handle, b, n, _lib.ptr(x), p("logits"), p("labels"), p("t1"), p("t2"),
                                _lib.ptr(_workspace(need)), _lib.stream_handle())
    _lib.check(st, "cls_forward")
    torch.cuda.synchronize()
    out = {}
    for k, buf in bufs.items():
        _check_guards(k, buf)
        out[k] = buf[1:-1] if k == "labels" else buf[1:-1].view(torch.float32)
    return out


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
    d = np.abs(flat[:, None, :] - flat[None, :, :]).max(axis=2)
    d[np.diag_indices(len(d))] = np.inf
    return d.min() / max(1.0, np.abs(ref).max())


def _one_point_clouds(b):
    """b clouds of one point each, spread over the unit cube centred at the origin."""
    return (np.random.default_rng(2024).random((b, 1, 3)) - 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _boundary_run(b):
    """(host clouds, device clouds, outputs of one call) for b one-point clouds; the largest b's run is reused by the
    labels-only test."""
    x = _one_point_clouds(b)
    xd = _dev(x)
    return x, xd, _forward(_clf(13), xd)


@pytest.mark.parametrize("b", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_chunk_boundary(b):
    """One call over b one-point clouds (no second chunk, a full chunk, a second chunk of one cloud, three chunks with a
    short last one), both transforms asked for.

    1. every output equals, bit for bit, the same clouds run PIECE at a time;
    2. the sampled clouds (_sample) equal the float64 model within TOL, labels where its top-2 gap allows;
    3. in float64 any two sampled clouds -- each boundary cloud and its counterparts one and two chunks earlier among
       them -- differ by more than 100 x TOL in the logits, in T1 and in T2, so a neighbour's or another chunk's result
       cannot pass 2.  One-point clouds drawn over the cube separate by that much (no need to raise n): in float64 the
       smallest distances are 1.3e-2 (logits), 8.1e-2 (T1), 4.8e-2 (T2), asserted below.
    4. the guards (_forward)."""
    import torch
    clf = _clf(13)
    x, xd, out = _boundary_run(b)
    for s in range(0, b, PIECE):
        piece = _forward(clf, xd[s:s + PIECE])
        for k, v in piece.items():
            assert torch.equal(v, out[k][s:s + PIECE]), "%s differs from the run in pieces at clouds %d..." % (k, s)
    idx = _sample(b, CHUNK, b)
    ref, t1, t2 = M.numpy_model(_weights(13), x[idx])
    sep = (_separation(ref), _separation(t1), _separation(t2))
    print("b %d: %d sampled clouds, separation logits %.2e T1 %.2e T2 %.2e" % ((b, len(idx)) + sep))
    assert min(sep) > 100 * TOL
    sel = torch.from_numpy(idx).to("cuda:0")
    got = {k: v[sel].cpu().numpy() for k, v in out.items()}
    e = (_err(got["logits"], ref), _err(got["t1"], t1), _err(got["t2"], t2))
    print("b %d: relative errors logits %.2e T1 %.2e T2 %.2e" % ((b,) + e))
    assert max(e) <= TOL
    top2 = np.sort(ref, axis=1)[:, -2:]
    ok = (top2[:, 1] - top2[:, 0]) > 10 * TOL * max(1.0, np.abs(ref).max())
    assert np.array_equal(got["labels"][ok], np.argmax(ref, axis=1)[ok])
    # the labels are the first maxima of the logits the same call wrote, for every cloud
    assert torch.equal(out["labels"].long(), out["logits"].argmax(dim=1))


def test_chunk_boundary_labels_only():
    """Without logits and transforms the launcher writes the logits to its T2 scratch and T1 / T2 nowhere else: the labels
    of a three-chunk call are those of the full call."""
    import torch
    b = 2 * CHUNK + 3
    _, xd, full = _boundary_run(b)
    out = _forward(_clf(13), xd, logits=False, transforms=False)
    assert sorted(out) == ["labels"]
    assert torch.equal(out["labels"], full["labels"])


def test_wrapper_sizes_a_workspace_above_2_GiB():
    """PointNetClassifier.forward on more than one chunk: the workspace of a full chunk is 3.0e9 bytes, more than an int
    holds.  A fresh object, so that the workspace is the one this call sizes."""
    import torch
    from geometric_adv_amd import _lib
    from geometric_adv_amd.classifier import PointNetClassifier
    b = CHUNK + 1
    need = _lib.lib().geoadv_cls_workspace_bytes(_clf(13).handle, b, 1)
    assert need == 3005435392
    _, xd, want = _boundary_run(b)
    clf = PointNetClassifier(None, num_classes=13, weights=_weights(13))
    logits, labels, t1, t2 = clf.forward(xd, transforms=True)
    assert clf._ws.numel() >= need
    assert torch.equal(logits, want["logits"]) and torch.equal(labels, want["labels"])
    assert torch.equal(t1, want["t1"]) and torch.equal(t2, want["t2"])
    del clf
    _boundary_run.cache_clear()
    _WS.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ size limits
def _labels_ok(got, ref):
    top2 = np.sort(ref, axis=1)[:, -2:] if ref.shape[1] > 1 else None
    if top2 is None:
        assert (got == 0).all()
        return
    ok = (top2[:, 1] - top2[:, 0]) > 10 * TOL * max(1.0, np.abs(ref).max())
    assert np.array_equal(got[ok], np.argmax(ref, axis=1)[ok])


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 16383, 16384])
def test_point_count_limits_vs_float64(n, b):
    x = _clouds(5000 + n, b, n)
    out = {k: v.cpu().numpy() for k, v in _forward(_clf(13), _dev(x)).items()}
    ref, t1, t2 = M.numpy_model(_weights(13), x)
    e = (_err(out["logits"], ref), _err(out["t1"], t1), _err(out["t2"], t2))
    print("n %d b %d: relative errors logits %.2e T1 %.2e T2 %.2e" % ((n, b) + e))
    assert max(e) <= TOL
    _labels_ok(out["labels"], ref)


@pytest.mark.parametrize("num_classes", [1, 2, 511, 512, 513, 1024])
def test_class_count_limits_vs_float64(num_classes):
    """One class, two, and counts around the head kernel's 512 threads (its fc3 loop strides by 512) up to the 1024 cap."""
    x = _clouds(6000 + num_classes, 5, 300)
    out = {k: v.cpu().numpy() for k, v in _forward(_clf(num_classes), _dev(x), transforms=False).items()}
    ref = M.numpy_model(_weights(num_classes), x)[0]
    assert out["logits"].shape == (5, num_classes)
    e = _err(out["logits"], ref)
    print("%d classes: relative error logits %.2e" % (num_classes, e))
    assert e <= TOL
    _labels_ok(out["labels"], ref)
    assert np.array_equal(out["labels"], np.argmax(out["logits"], axis=1))
    if num_classes == 1:
        assert (out["labels"] == 0).all()


@pytest.mark.parametrize("num_classes,first,second", [(13, 4, 9), (600, 77, 590), (600, 511, 512)])
def test_exact_tie_takes_the_first_maximum(num_classes, first, second):
    """Two identical fc3 columns and biases, raised above every other class: the logits tie exactly and the label is the
    first of the two, as np.argmax."""
    from geometric_adv_amd.classifier import PointNetClassifier
    w = dict(_weights(num_classes))
    W = np.array(w["fc3/weights"], copy=True)
    bias = np.array(w["fc3/biases"], copy=True)
    W[:, second] = W[:, first]
    bias[first] = bias[second] = np.abs(bias).max() + 100.0
    w["fc3/weights"], w["fc3/biases"] = W, bias
    x = _clouds(77, 6, 200)
    ref = M.numpy_model(w, x)[0]
    assert np.allclose(ref[:, first], ref[:, second], rtol=1e-12, atol=0)
    assert (np.delete(ref, [first, second], axis=1).max(axis=1) < ref[:, first] - 50).all()
    out = {k: v.cpu().numpy() for k, v in _forward(PointNetClassifier(None, num_classes=num_classes, weights=w), _dev(x),
                                                   transforms=False).items()}
    assert np.array_equal(out["logits"][:, first], out["logits"][:, second])
    assert _err(out["logits"], ref) <= TOL
    assert (out["labels"] == first).all()


# ------------------------------------------------------------------------------------------------ padded, degenerate
@pytest.mark.parametrize("n0,n", [(2011, 2048), (64, 2048), (1, 2048), (63, 64)])
def test_padding_with_the_last_point_changes_no_bit(n0, n):
    """What defend_surface / defend_critical hand on: n0 distinct points padded to n by repeating the last one (inside a
    tile, across a tile edge, across many tiles) give the bits of the n0-point cloud alone, transforms included."""
    import torch
    clf = _clf(13)
    x = _clouds(7000 + n0, 3, n0)
    padded = np.concatenate([x, np.repeat(x[:, -1:], n - n0, axis=1)], axis=1)
    assert padded.shape == (3, n, 3)
    a = _forward(clf, _dev(x))
    b = _forward(clf, _dev(padded))
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n", [1, 100, 2048])
def test_coincident_points_vs_float64(n):
    x = np.repeat(_clouds(8000, 4, 1), n, axis=1)
    out = {k: v.cpu().numpy() for k, v in _forward(_clf(13), _dev(x)).items()}
    ref, t1, t2 = M.numpy_model(_weights(13), x)
    assert all(np.isfinite(out[k]).all() for k in ("logits", "t1", "t2"))
    e = (_err(out["logits"], ref), _err(out["t1"], t1), _err(out["t2"], t2))
    print("coincident n %d: relative errors logits %.2e T1 %.2e T2 %.2e" % ((n,) + e))
    assert max(e) <= TOL
    _labels_ok(out["labels"], ref)
