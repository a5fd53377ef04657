"""GPU: the kNN term of the auto-encoder attack under the SURFACE rule (geoadv_attack_config.knn_rule = 1, knn_thresh; the
surface instances of csrc/knn_loss.hip's launch called from do_step in csrc/attack.hip) against the public op
ops.knn_outlier_loss(..., rule="surface"), which tests/test_gpu_surface_loss.py pins to the numpy model.  The mirror of
tests/test_gpu_attack_knn.py, same six loop forms, asserted through AdvAE._test_plan().

What is held: with init_pert = 0 the cached forward's adv is the source x bit for bit, so the gradient Adam consumed after ONE
iteration differs between a knn_weight = W handle and a knn_weight = 0 handle by dist_weight[b] * W * dK(x), dK the op's gradient
under the surface rule at k = 2:
  |grad_W - grad_0 - w_b W dK|  <=  4 * 2^-24 * (|grad_0| + |grad_W| + |w_b W dK|)        elementwise, subtraction in float64
The bound is the one derived in tests/test_gpu_attack_knn.py: the two totals differ by the term's two products and one sum inside
g_dist (each rounded to fp32, 2^-24 relative) and by the one fp32 sum g_enc + g_dist that forms the total in each handle.  The
arithmetic that applies the term is the same kernel epilogue under either rule, so the derivation carries over unchanged.

The threshold of a shape is the median model score (tests/_surface_loss_model.py, brute-force neighbours) of its first source
cloud: a float32, so the handle (knn_thresh is a float) and the op (thr = (float)alpha) see the same value, and about half of
that cloud's points are masked.

A cloud alone and in a batch: the issue asks for the same bytes.  A handle of B = 1 runs another loop form than one of B = 16
(two-scan kernel, another backward), and the TOTAL gradient is all the handle shows, so across batch SIZES the two are held to
the bound above (as tests/test_gpu_attack_knn.py holds the SOR term); bytes are asserted where the form is the same: the cloud
at another slot among other batch mates, and two handles of one configuration.  The term's own launch is held to bytes alone and
in a batch by tests/test_gpu_surface_loss.py.

Victims: weights.randomized_weights(n); clouds: kinds `random` and `dodecahedron` (tests/_surface_loss_model.py) alternating."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_loss_model as M  # noqa: E402
import _surface_loss_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu

W_TERM, K = 3.0, 2
EPS = 2.0 ** -24

CASES = {      # b, n, Configuration arguments, what _test_plan() must report (those of tests/test_gpu_attack_knn.py)
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


def _handle(b, n, knn_weight=None, thr=None, lr=0.01, **conf):
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    kw = {} if knn_weight is None else dict(knn_weight=knn_weight, knn_k=K, knn_rule="surface", knn_thresh=float(thr))
    kw.update(conf)
    c = Configuration(batch_size=b, n_points=n, weights=None, num_iterations=2, num_iterations_thresh=1, learning_rate=lr, **kw)
    return AdvAE("surface-term", c, ae=_ae(n))


def _median_score(cloud):
    x = cloud[None]
    return np.float32(np.median(SM.scores(SM.dists(x, M.brute_idx(x, K)), K)[0]))


def _inputs(b, n):
    """Sources of kinds random / dodecahedron alternating, random targets, per-cloud weights that differ, the shape's threshold
    and the op's gradient under the surface rule, computed once per shape."""
    import torch
    if (b, n) not in _REF:
        from geometric_adv_amd import ops
        x = np.stack([SM.cloud_of_kind(("random", "dodecahedron")[c % 2], n, 700 + c) for c in range(b)])
        gt = np.stack([SM.cloud_of_kind("random", n, 800 + c) for c in range(b)])
        w = np.resize(np.array([0.5, 1.0, 2.0, 0.25, 1.5], np.float32), b)
        tz = _ae(n).transform(gt).astype(np.float32)
        thr = _median_score(x[0])
        dK = ops.knn_outlier_loss(torch.as_tensor(x, device="cuda:0"), K, rule="surface", thresh=float(thr))[1].cpu().numpy()
        _REF[(b, n)] = dict(x=x, gt=gt, w=w, tz=tz, dK=dK, thr=thr)
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
    printed per case under -s): two_scan_3x256 0.821, symmetric_16x256 1.071, separate_adam_16x256 1.071, latent_16x256 1.035,
    max_point_16x256 1.071, ragged_2x1025 0.906; no element beyond the bound in any case."""
    case = CASES[name]
    b, n = case["b"], case["n"]
    inp = _inputs(b, n)
    dK, thr = inp["dK"], inp["thr"]
    assert (np.abs(dK).reshape(b, -1).max(axis=1) > 0).all(), "dK must be non-zero on at least one point of every cloud"
    term = inp["w"].astype(np.float64)[:, None, None] * W_TERM * dK.astype(np.float64)

    h0, hw = _handle(b, n, 0.0, thr, **case["conf"]), _handle(b, n, W_TERM, thr, **case["conf"])
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

    # two handles of one configuration, used alternately on the one stream, give the bits each gives alone
    a0, aw = _handle(b, n, 0.0, thr, **case["conf"]), _handle(b, n, W_TERM, thr, **case["conf"])
    _start(aw, inp); _start(a0, inp)
    aw.run(0, 1, 1); a0.run(0, 1, 1)
    for key, at in (("0", a0), ("w", aw)):
        assert _same_bytes(_peek(at), peeks[key]) == [], "alternating handles changed the first iteration of handle %s" % key


def test_a_threshold_nothing_exceeds_changes_nothing():
    """knn_thresh = 1e6 masks no point: dK = +0.0 everywhere, and after two iterations grad, pert, adv and the six history rows
    equal those of the knn_weight = 0 handle as values."""
    import torch
    b, n = 16, 256
    inp = _inputs(b, n)
    out = {}
    for key, weight, thr in (("0", 0.0, inp["thr"]), ("w", W_TERM, 1e6)):
        at = _handle(b, n, weight, thr)
        _start(at, inp)
        hist = torch.zeros((2, 6, b), dtype=torch.float32, device="cuda:0")
        at.run(0, 2, 1, hist)
        out[key] = (_peek(at), hist.clone())
    for k in ("grad", "pert", "adv"):
        assert torch.equal(out["0"][0][k], out["w"][0][k]), k
    assert torch.equal(out["0"][1], out["w"][1])
    assert torch.isfinite(out["0"][1]).all()


def test_rule_sor_is_the_handle_without_the_two_members():
    """knn_rule = 'sor' with any knn_thresh: the bytes of a handle whose Configuration never named the two members, term on
    (knn_k = 5, knn_alpha = 1.05) and off, after two iterations."""
    import torch
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    b, n = 16, 256
    inp = _inputs(b, n)
    for weight in (0.0, W_TERM):
        peeks = []
        for extra in ({}, dict(knn_rule="sor", knn_thresh=-7.0)):
            c = Configuration(batch_size=b, n_points=n, weights=None, num_iterations=2, num_iterations_thresh=1, learning_rate=0.01,
                              knn_weight=weight, knn_k=5, knn_alpha=1.05, **extra)
            at = AdvAE("surface-term", c, ae=_ae(n))
            _start(at, inp)
            hist = torch.zeros((2, 6, b), dtype=torch.float32, device="cuda:0")
            at.run(0, 2, 1, hist)
            p = _peek(at)
            p["hist"] = hist.clone()
            peeks.append(p)
        assert _same_bytes(peeks[0], peeks[1]) == [], "knn_weight = %g" % weight


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
            at = _handle(bb, n, wt, inp["thr"])
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


def test_a_cloud_has_the_same_bytes_among_other_clouds():
    """Bytes where bytes are possible: the loop form depends on the batch size (B = 1 runs the two-scan kernel and another
    backward, so its total gradient differs from the batch's in the last bits whatever the term does -- the test above), but not
    on a cloud's slot or on its batch mates.  Cloud 0 of the 16 x 256 case at slot 5 of a batch of 15 OTHER source clouds (its own
    target and weight with it): after one iteration with the term its gradient, perturbation and adversarial cloud have the bytes
    they have at slot 0 of the original batch."""
    b, n, slot = 16, 256, 5
    inp = _inputs(b, n)
    other = dict(inp)
    other["x"] = np.stack([SM.cloud_of_kind("random", n, 1700 + c) for c in range(b)])
    other["x"][slot] = inp["x"][0]
    for key in ("gt", "tz", "w"):
        other[key] = np.roll(inp[key], slot, axis=0)
    assert np.array_equal(other["gt"][slot], inp["gt"][0]) and other["w"][slot] == inp["w"][0]
    peeks = []
    for data in (inp, other):
        at = _handle(b, n, W_TERM, inp["thr"])
        _start(at, data)
        at.run(0, 1, 1)
        peeks.append(_peek(at))
    for k in ("grad", "pert", "adv"):
        assert peeks[0][k][0].cpu().numpy().tobytes() == peeks[1][k][slot].cpu().numpy().tobytes(), k
    assert peeks[0]["grad"][1].cpu().numpy().tobytes() != peeks[1]["grad"][1].cpu().numpy().tobytes()      # (the mates did change)


def test_it_does_what_it_is_for():
    """16 x 256 random clouds, threshold the median score of the first, learning rate 0.01, 60 iterations, dist_weight 1: the
    off-surface defense's filter (ops.outlier_filter on ops.knn_dists, k = 2) finds strictly fewer outliers over the batch in the
    best clouds of the knn_weight = 5 attack than in those of the attack without the term.  MI355X run (printed under -s), at
    thr = 0.105279133: 2121 outliers in the sources, 2164 in the best clouds without the term, 69 with knn_weight = 5."""
    import torch
    from geometric_adv_amd import ops
    b, n = 16, 256
    x = np.stack([SM.cloud_of_kind("random", n, 910 + c) for c in range(b)])
    gt = np.stack([SM.cloud_of_kind("random", n, 920 + c) for c in range(b)])
    tz = _ae(n).transform(gt).astype(np.float32)
    thr = _median_score(x[0])

    def outliers(clouds):
        dev = torch.as_tensor(clouds, dtype=torch.float32, device="cuda:0")
        return int(ops.outlier_filter(dev, ops.knn_dists(dev, K), float(thr), top_k=K)[2].to(torch.int64).sum())

    ref = _ae(n).get_loss_per_pc(gt).astype(np.float32)
    totals = {}
    for wt in (0.0, 5.0):
        from geometric_adv_amd.adv_ae import AdvAE, Configuration
        c = Configuration(batch_size=b, n_points=n, weights=None, num_iterations=60, num_iterations_thresh=40, learning_rate=0.01,
                          dist_weight_list=[1.0], knn_weight=wt, knn_k=K, knn_rule="surface", knn_thresh=float(thr))
        at = AdvAE("surface-term", c, ae=_ae(n))
        at.set_inputs(x, gt, tz, 1.0)
        at.init_pert(np.zeros_like(x), reset_optimizer=True)
        at.run(0, 60, 40)
        totals[wt] = outliers(at.get_best(ref)[1])
    print("outliers over the batch at thr = %.9g: sources %d, best clouds without the term %d, with knn_weight = 5 %d"
          % (thr, outliers(x), totals[0.0], totals[5.0]))
    assert totals[5.0] < totals[0.0]


def _config(b, **kw):
    from geometric_adv_amd import _abi
    c = _abi.AttackConfig(batch=b, loss_adv_type=_abi.GEOADV_LOSS_ADV_CHAMFER, loss_dist_type=_abi.GEOADV_LOSS_DIST_CHAMFER,
                          learning_rate=0.01, knn_weight=W_TERM, knn_k=K, knn_rule=1, knn_thresh=0.04)          # every other member zero
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


BAD = {       # the bad field(s), a word of the message
    "knn_rule 2": (dict(knn_rule=2), "knn_rule"),
    "knn_rule -1": (dict(knn_rule=-1), "knn_rule"),
    "knn_k 8 under rule 1": (dict(knn_k=8), "knn_k"),
    "knn_thresh -1": (dict(knn_thresh=-1.0), "knn_thresh"),
    "knn_thresh nan": (dict(knn_thresh=float("nan")), "knn_thresh"),
    "knn_thresh inf": (dict(knn_thresh=float("inf")), "knn_thresh"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_create_refuses(name):
    from geometric_adv_amd import _abi
    fields, word = BAD[name]
    rc, h, msg = _create(_ae(256), _config(2, **fields))
    assert rc == _abi.GEOADV_EINVAL and not h.value
    assert word in msg, msg


def test_create_reads_only_what_the_rule_reads():
    """Rule 1 does not read knn_alpha; rule 0 does not read knn_thresh and takes knn_k = 8; knn_weight = 0 reads neither member."""
    from geometric_adv_amd import _lib
    for fields in (dict(knn_alpha=float("nan")), dict(knn_alpha=-1.0, knn_k=7),
                   dict(knn_rule=0, knn_alpha=1.05, knn_k=8, knn_thresh=float("nan")),
                   dict(knn_weight=0.0, knn_rule=99, knn_thresh=float("nan"), knn_k=-3)):
        rc, h, msg = _create(_ae(256), _config(2, **fields))
        assert rc == 0 and h.value, msg
        _lib.lib().geoadv_attack_destroy(h)
