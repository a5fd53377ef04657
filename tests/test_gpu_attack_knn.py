"""GPU: the kNN outlier term of the auto-encoder attack (geoadv_attack_config.knn_weight; csrc/knn_loss.hip's second instance
called from do_step in csrc/attack.hip) against the public op ops.knn_outlier_loss, which tests/test_gpu_knn_loss.py pins to the
numpy model.

What is held: with init_pert = 0 the cached forward's adv is the source x bit for bit, so the gradient Adam consumed after ONE
iteration differs between a knn_weight = W handle and a knn_weight = 0 handle by dist_weight[b] * W * dK(x), dK the op's gradient:
  |grad_W - grad_0 - w_b W dK|  <=  4 * 2^-24 * (|grad_0| + |grad_W| + |w_b W dK|)        elementwise, subtraction in float64
The bound is derived, not measured: the two totals differ by the term's products and one sum inside g_dist (each rounded to fp32,
2^-24 relative) and by the one fp32 sum g_enc + g_dist that forms the total in each handle.

The reference is the op at alpha = 1.05 (a double); the handle takes knn_alpha as a float, so its alpha is float32(1.05) widened,
4.8e-8 below.  A point whose (s - mu)^2 lies within 1e-7 of alpha^2 var would change sides and fail the bound by orders of
magnitude: none of these clouds has one.

Shapes: the smallest that reach each path of do_step and of the kernel (asserted through AdvAE._test_plan() where the plan says it):
  3 x 256           two-scan kernel (batch * n < 4096), masked backward; at this size the forward's fused loss launch forms g_dist
  16 x 256          symmetric scan, fused loss launch, Adam in the next forward's loaders
  16 x 256          separate_adam=True: Adam as its own launch
  16 x 256          loss_adv_type='latent'
  16 x 256          max_point_dist_weight=2.0: the step forms g_dist itself (max-point branch), the term is added after it
  2 x 1025          a second point per thread of the 1024-thread workgroup, ragged tile
Victims: weights.randomized_weights(n); clouds: tests/_knn_loss_model.cloud_of_kind, kinds `random` and `hub` in every batch.
(The stream test of the term is tests/test_gpu_stream_order_attack_knn.py: it has to run after tests/test_gpu_stream_order.py.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _knn_loss_model import cloud_of_kind  # noqa: E402

pytestmark = pytest.mark.gpu

W_TERM, K, ALPHA = 3.0, 5, 1.05
EPS = 2.0 ** -24

CASES = {      # b, n, Configuration arguments, what _test_plan() must report
    "two_scan_3x256": dict(b=3, n=256, conf={}, plan=dict(symmetric=False, loss="fused")),
    "symmetric_16x256": dict(b=16, n=256, conf={}, plan=dict(symmetric=True, loss="fused", grad="fused_1pass")),
    "separate_adam_16x256": dict(b=16, n=256, conf={"separate_adam": True}, plan=dict(symmetric=True, loss="fused", grad="fused_1pass")),
    "latent_16x256": dict(b=16, n=256, conf={"loss_adv_type": "latent"}, plan=dict(symmetric=True, grad="fused_1pass")),
    "max_point_16x256": dict(b=16, n=256, conf={"max_point_dist_weight": 2.0}, plan=dict(symmetric=True, loss="metrics", grad="step_fx_1pass")),
    "ragged_2x1025": dict(b=2, n=1025, conf={}, plan=dict(symmetric=False)),
}

_AE = {}
_REF = {}


def _ae(n):
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    if n not in _AE:
        _AE[n] = PointNetAE(W.randomized_weights(n), n, encoder_arith="bf16x3")     # (the hub clouds' filler sits at 10: fp32 range)
    return _AE[n]


def _handle(b, n, knn_weight=None, lr=0.01, **conf):
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    kw = {} if knn_weight is None else dict(knn_weight=knn_weight, knn_k=K, knn_alpha=ALPHA)
    kw.update(conf)
    c = Configuration(batch_size=b, n_points=n, weights=None, num_iterations=2, num_iterations_thresh=1, learning_rate=lr, **kw)
    return AdvAE("knn-term", c, ae=_ae(n))


def _inputs(b, n):
    """Sources of kinds random / hub alternating, random targets, per-cloud weights that differ, computed once per shape."""
    import torch
    if (b, n) not in _REF:
        from geometric_adv_amd import ops
        x = np.stack([cloud_of_kind(("random", "hub")[c % 2], n, 700 + c) for c in range(b)])
        gt = np.stack([cloud_of_kind("random", n, 800 + c) for c in range(b)])
        w = np.resize(np.array([0.5, 1.0, 2.0, 0.25, 1.5], np.float32), b)
        tz = _ae(n).transform(gt).astype(np.float32)
        dK = ops.knn_outlier_loss(torch.as_tensor(x, device="cuda:0"), K, ALPHA)[1].cpu().numpy()
        _REF[(b, n)] = dict(x=x, gt=gt, w=w, tz=tz, dK=dK)
    return _REF[(b, n)]


def _start(at, inp, sel=None):
    s = slice(None) if sel is None else sel
    x = inp["x"][s]
    at.set_inputs(x, inp["gt"][s], inp["tz"][s], inp["w"][s])
    at.init_pert(np.zeros_like(x), reset_optimizer=True)


def _peek(at):
    import torch
    p = at.peek()
    torch.cuda.synchronize()
    return p


def _equal_peeks(a, b):
    import torch
    return [k for k in sorted(a) if not torch.equal(a[k], b[k])]


def _same_bytes(a, b):
    import torch
    return [k for k in sorted(a) if not torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8))]


def _term_error(g0, gw, term):
    """(worst ratio of |grad_W - grad_0 - term| to the bound's sum, in units of 2^-24; must be <= 4)"""
    g0, gw, term = (np.asarray(a, np.float64) for a in (g0, gw, term))
    err = np.abs(gw - g0 - term)
    scale = np.abs(g0) + np.abs(gw) + np.abs(term)
    assert np.isfinite(err).all() and np.isfinite(scale).all()
    bad = err > 4.0 * EPS * scale
    ratio = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0)) / EPS
    return float(ratio.max()), int(bad.sum())


@pytest.mark.parametrize("name", list(CASES))
def test_the_term_is_the_ops_gradient_weighted(name):
    """Measured on an MI355X (worst |grad_W - grad_0 - w W dK| in units of 2^-24 of |grad_0| + |grad_W| + |w W dK|; bound 4;
    printed per case under -s): two_scan_3x256 0.857, symmetric_16x256 0.934, separate_adam_16x256 0.934, latent_16x256 0.900,
    max_point_16x256 0.934, ragged_2x1025 0.688; no element beyond the bound in any case."""
    case = CASES[name]
    b, n = case["b"], case["n"]
    inp = _inputs(b, n)
    dK = inp["dK"]
    assert (np.abs(dK).reshape(b, -1).max(axis=1) > 0).all(), "dK must be non-zero on at least one point of every cloud"
    term = inp["w"].astype(np.float64)[:, None, None] * W_TERM * dK.astype(np.float64)

    h0, hw = _handle(b, n, 0.0, **case["conf"]), _handle(b, n, W_TERM, **case["conf"])
    peeks = {}
    for key, at in (("0", h0), ("w", hw)):
        _start(at, inp)
        at.run(0, 1, 1)
        plan = at._test_plan()
        got = {k: plan[k] for k in case["plan"]}
        assert got == case["plan"], "%s runs another form than the one it was written for: %s" % (name, got)
        peeks[key] = _peek(at)
    worst, nbad = _term_error(peeks["0"]["grad"].cpu().numpy(), peeks["w"]["grad"].cpu().numpy(), term)
    print("%s: worst %.3f x 2^-24 of the bound's sum (bound 4), %d elements beyond it" % (name, worst, nbad))
    assert nbad == 0 and worst <= 4.0

    # knn_weight = 0 is a handle without the members: every peeked tensor equals that of a default-configuration handle
    hd = _handle(b, n, None, **case["conf"])
    _start(hd, inp)
    hd.run(0, 1, 1)
    assert _equal_peeks(_peek(hd), peeks["0"]) == []

    # nothing process-wide: a second iteration of each alone, then a fresh pair used alternately on the one stream
    for at in (h0, hw):
        at.run(1, 1, 1)
    solo = {"0": _peek(h0), "w": _peek(hw)}
    a0, aw = _handle(b, n, 0.0, **case["conf"]), _handle(b, n, W_TERM, **case["conf"])
    _start(aw, inp); _start(a0, inp)
    aw.run(0, 1, 1); a0.run(0, 1, 1)
    first = {"0": _peek(a0), "w": _peek(aw)}
    aw.run(1, 1, 1); a0.run(1, 1, 1)
    second = {"0": _peek(a0), "w": _peek(aw)}
    for key in ("0", "w"):
        assert _same_bytes(first[key], peeks[key]) == [], "alternating handles changed the first iteration of handle %s" % key
        assert _same_bytes(second[key], solo[key]) == [], "alternating handles changed the second iteration of handle %s" % key


def test_an_empty_mask_changes_nothing():
    """knn_alpha = 1e6 masks no point: dK = +0.0 everywhere, and after two iterations grad, pert, adv and the six history rows
    equal those of the knn_weight = 0 handle as values."""
    import torch
    b, n = 16, 256
    inp = _inputs(b, n)
    out = {}
    for key, weight, kw in (("0", 0.0, {}), ("w", W_TERM, dict(knn_alpha=1e6))):
        at = _handle(b, n, weight, **kw)
        _start(at, inp)
        hist = torch.zeros((2, 6, b), dtype=torch.float32, device="cuda:0")
        at.run(0, 2, 1, hist)
        out[key] = (_peek(at), hist.clone())
    for k in ("grad", "pert", "adv"):
        assert torch.equal(out["0"][0][k], out["w"][0][k]), k
    assert torch.equal(out["0"][1], out["w"][1])
    assert torch.isfinite(out["0"][1]).all()


def test_a_cloud_alone_and_in_a_batch():
    """Cloud 0 of the 16 x 256 case attacked alone (B = 1: another scan, another backward) and inside the batch: its kNN
    contribution grad_W - grad_0 is w_0 W dK[0] within the bound of the first test either way, so the two differ by at most the
    two bounds together; two handles of one configuration give identical bits."""
    b, n = 16, 256
    inp = _inputs(b, n)
    term = float(inp["w"][0]) * W_TERM * inp["dK"][0].astype(np.float64)
    diff, bound = {}, {}
    for key, bb, sel in (("alone", 1, slice(0, 1)), ("batch", b, None)):
        g = {}
        for wkey, wt in (("0", 0.0), ("w", W_TERM), ("w2", W_TERM)):
            at = _handle(bb, n, wt)
            _start(at, inp, sel)
            at.run(0, 1, 1)
            g[wkey] = _peek(at)["grad"][0].cpu().numpy()
        assert g["w"].tobytes() == g["w2"].tobytes(), "two runs of one configuration differ (%s)" % key
        worst, nbad = _term_error(g["0"], g["w"], term)
        print("cloud 0 %s: worst %.3f x 2^-24 (bound 4)" % (key, worst))
        assert nbad == 0
        diff[key] = g["w"].astype(np.float64) - g["0"].astype(np.float64)
        bound[key] = 4.0 * EPS * (np.abs(g["0"]) + np.abs(g["w"]) + np.abs(term))
    assert (np.abs(diff["alone"] - diff["batch"]) <= bound["alone"] + bound["batch"]).all()


def test_it_does_what_it_is_for():
    """4 x 256 random clouds with 12 points displaced by 0.2 along a fixed direction (K(x) > 0), learning rate 0.01, 60
    iterations, dist_weight 1: the sum over the batch of K(adv) is strictly smaller with knn_weight = 20 than without.
    MI355X run (printed under -s): sum of K over the sources 0.0234182926, over adv without the term 0.0182916106, over adv with
    knn_weight = 20 0.00262816411."""
    import torch
    from geometric_adv_amd import ops
    b, n = 4, 256
    rng = np.random.default_rng(900)
    x = np.stack([cloud_of_kind("random", n, 910 + c) for c in range(b)])
    direction = np.array([0.6, 0.0, 0.8], np.float32)
    for c in range(b):
        x[c, rng.permutation(n)[:12]] += np.float32(0.2) * direction
    gt = np.stack([cloud_of_kind("random", n, 920 + c) for c in range(b)])
    tz = _ae(n).transform(gt).astype(np.float32)
    kx = float(ops.knn_outlier_loss(torch.as_tensor(x, device="cuda:0"))[0].sum())
    assert kx > 0.0
    sums = {}
    for wt in (0.0, 20.0):
        at = _handle(b, n, wt, lr=0.01)
        at.set_inputs(x, gt, tz, 1.0)
        at.init_pert(np.zeros_like(x), reset_optimizer=True)
        at.run(0, 60, 60)
        sums[wt] = float(ops.knn_outlier_loss(_peek(at)["adv"])[0].sum())
    print("sum of K over the batch: sources %.9g, adv without the term %.9g, adv with knn_weight = 20 %.9g" % (kx, sums[0.0], sums[20.0]))
    assert sums[20.0] < sums[0.0]


def _config(b, **kw):
    from geometric_adv_amd import _abi
    c = _abi.AttackConfig(batch=b, loss_adv_type=_abi.GEOADV_LOSS_ADV_CHAMFER, loss_dist_type=_abi.GEOADV_LOSS_DIST_CHAMFER,
                          learning_rate=0.01, knn_weight=W_TERM, knn_k=K, knn_alpha=ALPHA)          # every other member zero
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _create(ae, cfg):
    from geometric_adv_amd import _lib
    import torch
    h = C.c_void_p()
    with torch.cuda.device("cuda:0"):
        rc = _lib.lib().geoadv_attack_create(C.byref(h), ae.handle, C.byref(cfg))
    return rc, h, _lib.lib().geoadv_last_error().decode("utf-8", "replace")


BAD = {       # n_points of the victim, the bad field(s), a word of the message
    "knn_weight nan": (256, dict(knn_weight=float("nan")), "knn_weight"),
    "knn_weight inf": (256, dict(knn_weight=float("inf")), "knn_weight"),
    "loss_dist_type pert": (256, dict(loss_dist_type=1), "pert"),
    "knn_k 0": (256, dict(knn_k=0), "knn_k"),
    "knn_k 16": (256, dict(knn_k=16), "knn_k"),
    "knn_alpha -1": (256, dict(knn_alpha=-1.0), "knn_alpha"),
    "knn_alpha nan": (256, dict(knn_alpha=float("nan")), "knn_alpha"),
    "knn_alpha inf": (256, dict(knn_alpha=float("inf")), "knn_alpha"),
    "n = knn_k + 1": (16, dict(knn_k=15), "points"),
    "n 16385": (16385, dict(), "points"),
    "batch 65536": (256, dict(batch=65536), "batch"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_create_refuses(name):
    from geometric_adv_amd import _abi
    n, fields, word = BAD[name]
    rc, h, msg = _create(_ae(n), _config(2, **fields))
    if n != 256:
        _AE.pop(n)                  # (victims of other sizes serve this case alone)
    assert rc == _abi.GEOADV_EINVAL and not h.value
    assert word in msg, msg


def test_create_ignores_the_other_members_while_the_term_is_off():
    from geometric_adv_amd import _lib
    for n, fields in ((256, dict(knn_k=-7, knn_alpha=float("nan"))), (256, dict(knn_k=1 << 30, knn_alpha=-1.0)),
                      (256, dict(loss_dist_type=1, knn_k=99))):
        rc, h, msg = _create(_ae(n), _config(2, knn_weight=0.0, **fields))
        assert rc == 0 and h.value, msg
        _lib.lib().geoadv_attack_destroy(h)
