"""GPU: the classifier's input gradient (csrc/cls_grad.hip through geoadv_cls_input_grad and
PointNetClassifier.input_gradient) against the float64 model of tests/_cls_grad_model64.py, its tie and sparsity rules, its
bit-exact invariances, isolation and refusals.  Every test calls the new entry point."""
import ctypes
import functools

import numpy as np
import pytest

import _cls_grad_model64 as G
import _cls_model64 as M

pytestmark = pytest.mark.gpu

# TOLERANCE -- a measurement, not a choice.  tools/cls_grad_tolerance.py runs the SAME torch graph in float32 on the CPU
# (winners handed in from the float64 run) and compares with float64:
#   gradient, max-abs over the cloud / the cloud's max-abs gradient, worst cloud of this file's 90 (case, cloud) pairs:
#                                                                  F32_GRAD_ERR = 2.41e-5
#   pre-activations per layer, max |pre32 - pre64| / max |pre64| over a cloud, worst of 120 clouds of this file's generator
#   (seeds 0 .. 3 of every (classes, n)):                          F32_PRE_ERR[layer] = 2.3e-7 (tconv1) ... 3.7e-5 (fc2)
#   logits, max-abs / max |Z|, same sample:                        F32_LOGIT_ERR = 3.42e-5
# The GPU gets 4 x torch's gradient error (an fp32 chain summed in another order, with the head kernels' sequential
# 1024-term chains, earned the forward about 4 x torch's error in test_gpu_classifier.py):  TOL_GRAD = 4 * 2.41e-5 = 9.64e-5.
# MARGIN.  A ReLU whose float64 pre-activation lies within the forward's error of zero may be masked the other way on the
# GPU, which moves a whole path's gradient, not a rounding (seen on the MI355X on unselected clouds: 4e-4 ... 3e-1 of the
# cloud's largest gradient, at units within 2e-6 of zero; 1e-6 ... 2e-5 on clouds without such a unit).  A cloud is compared
# only if every unit on a winner row's path keeps |pre| / max |pre of its layer| >= F32_PRE_ERR[layer] for the per-point
# layers -- the WORST float32 error among the layer's ~10^6 sampled units, several times a typical unit's; their fan-in is
# <= 128 on the MFMA, like torch's blocked sums -- and >= 4 * F32_PRE_ERR[layer] for the fc1 / fc2 units of the three heads,
# whose sequential 1024-term chains are where the GPU earned its factor 4; the CW maximum and clamp keep 4 * F32_LOGIT_ERR.
# The pools' own near ties need no margin: the op's winners are validated against float64 and then handed to the model.
# SEEDS.  A random cloud keeps these margins with probability 0.05 ... 0.15 (n >= 63), so CASE_SEED[(classes, n)] lists, per
# cloud, the first seeds whose cloud keeps 1.25 x the margins for all three losses (searched on the CPU with the float64
# model alone, same tool): the float64 model leaves out none of the 120 comparisons, and the GPU's own winners can move a
# margin only by a near tie's width.  The cap asserted below: at most a quarter left out over the whole parametrised set,
# at least one cloud kept per case.
# Loss and logits: the forward's tolerance (test_gpu_classifier.py: 1e-4 of max(1, max |Z|)); a loss is a difference of
# two logits or a log-sum-exp minus one, hence twice that.
F32_GRAD_ERR = 2.41e-05
F32_LOGIT_ERR = 3.42e-05
F32_PRE_ERR = {"transform_net1/tconv1": 2.26e-07, "transform_net1/tconv2": 7.23e-07, "conv1": 4.68e-06, "conv2": 7.63e-06,
               "transform_net2/tconv1": 8.15e-06, "transform_net2/tconv2": 1.17e-05, "conv3": 1.33e-05, "conv4": 1.52e-05,
               "transform_net1/tfc1": 5.14e-06, "transform_net1/tfc2": 6.70e-06, "transform_net2/tfc1": 1.66e-05,
               "transform_net2/tfc2": 2.13e-05, "fc1": 2.95e-05, "fc2": 3.69e-05}
TOL_GRAD = 4 * F32_GRAD_ERR
TOL_FWD = 1e-4
CASE_SEED = {(13, 1): (0, 1, 2), (13, 63): (7, 42, 49), (13, 64): (12, 23, 49), (13, 65): (12, 20, 27), (13, 130): (42, 71, 155),
             (40, 1): (0, 3, 5), (40, 63): (5, 26, 32), (40, 64): (2, 19, 25), (40, 65): (8, 14, 81), (40, 130): (182, 237, 258)}
KAPPA = 0.5
CLOUDS = 3
NS = (1, 63, 64, 65, 130)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _weights(num_classes):
    from geometric_adv_amd import cls_weights as CW
    return CW.synthetic_weights(num_classes, seed=num_classes)


@functools.lru_cache(maxsize=None)
def _clf(num_classes):
    from geometric_adv_amd.classifier import PointNetClassifier
    return PointNetClassifier(None, num_classes=num_classes, weights=_weights(num_classes))


def make_case(seed, num_classes, n, loss, clouds=CLOUDS):
    """Clouds in the unit cube's centre and labels that keep every loss informative: the cross entropy and the targeted CW
    loss aim at a class the float64 model does NOT predict (a saturated softmax has a gradient of rounding noise), the
    untargeted CW loss starts from the predicted class (otherwise it sits on its clamp)."""
    if isinstance(seed, tuple):                                          # one seed per cloud (CASE_SEED)
        parts = [make_case(s, num_classes, n, loss, clouds=1) for s in seed]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    rng = np.random.default_rng(seed)
    x = (rng.random((clouds, n, 3)) - 0.5).astype(np.float32)
    top = np.argmax(M.numpy_model(_weights(num_classes), x)[0], axis=1)
    shift = 1 + rng.integers(0, num_classes - 1, clouds)
    y = top if loss == "cw_untargeted" else (top + shift) % num_classes
    return x, y.astype(np.int32)


def keep_mask(ref, factor=1.0):
    """Which clouds of a float64 result keep the margins above (times `factor`)."""
    keep = np.ones(len(ref["loss"]), bool)
    for s, m in ref["margin_layers"].items():
        keep &= m >= factor * (4 if "fc" in s else 1) * F32_PRE_ERR[s]
    return keep & (ref["margin_loss"] >= factor * 4 * F32_LOGIT_ERR)


def _grad_err(got, ref):
    b = len(ref)
    scale = np.abs(ref).reshape(b, -1).max(1)
    return np.abs(np.asarray(got, np.float64) - ref).reshape(b, -1).max(1) / np.where(scale > 0, scale, 1.0)


def _validate_winners(win, ref):
    """Each row the op chose holds, in float64, a value within the forward's tolerance of the float64 maximum."""
    for p in range(3):
        col = ref["columns"][p]                                         # (b, n, 1024)
        top = col.max(1)
        chosen = np.take_along_axis(col, win[:, p][:, None, :].astype(np.int64), axis=1)[:, 0]
        assert (win[:, p] >= 0).all() and (win[:, p] < col.shape[1]).all()
        assert (top - chosen <= TOL_FWD * max(1.0, col.max())).all(), "pool %d: a winner is not a maximum" % p


@functools.lru_cache(maxsize=None)
def _compare(b, num_classes, n, loss):
    """One call of the op on a case and its comparison with the float64 model: (kept (b,) bool, gradient errors (b,),
    max |grad| (b,), logits error, loss error, max(1, max |Z|))."""
    x, y = make_case(CASE_SEED[(num_classes, n)], num_classes, n, loss)
    x, y = x[:b], y[:b]
    L, g, logits, win = _clf(num_classes).input_gradient(_dev(x), _dev(y), loss, KAPPA, return_logits=True, return_winners=True)
    win = win.cpu().numpy()
    w = _weights(num_classes)
    _validate_winners(win, G.grad_model(w, x, y, loss, KAPPA))
    ref = G.grad_model(w, x, y, loss, KAPPA, winners=win)               # a near tie cannot move the gradient to another point
    return (keep_mask(ref), _grad_err(g.cpu().numpy(), ref["grad"]), np.abs(ref["grad"]).reshape(b, -1).max(1),
            np.abs(logits.cpu().numpy() - ref["logits"]).max(), np.abs(L.cpu().numpy() - ref["loss"]).max(),
            max(1.0, np.abs(ref["logits"]).max()))


@pytest.mark.parametrize("loss", G.LOSSES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("num_classes", [13, 40])
@pytest.mark.parametrize("b", [1, 3])
def test_gradient_loss_and_logits_vs_float64(b, num_classes, n, loss):
    keep, err, gmax, logit_err, loss_err, zmax = _compare(b, num_classes, n, loss)
    print("b %d classes %d n %d %s: kept %s gradient errors %s (TOL %.2e) max |grad| %s logits %.2e loss %.2e" %
          (b, num_classes, n, loss, keep, err, TOL_GRAD, gmax, logit_err, loss_err))
    assert logit_err <= TOL_FWD * zmax
    assert loss_err <= 2 * TOL_FWD * zmax
    assert keep.any(), "every cloud of the case is below the decision margin"
    assert (gmax[keep] > 0).all()
    assert (err[keep] <= TOL_GRAD).all()


def test_left_out_clouds_stay_under_the_cap():
    """At most a quarter of the clouds of the whole parametrised set are below the margin (its cases are computed once)."""
    out = total = 0
    for b in (1, 3):
        for num_classes in (13, 40):
            for n in NS:
                for loss in G.LOSSES:
                    keep = _compare(b, num_classes, n, loss)[0]
                    out += int((~keep).sum())
                    total += b
    assert total == 120 and 4 * out <= total, "%d of %d clouds left out" % (out, total)


def test_detached_transforms_are_told_apart():
    """The float64 gradient with T1 and T2 held constant differs from the full one by far more than the tolerance
    (> 100 x TOL_GRAD) on the test weights, and the op agrees with the full one."""
    x, y = make_case(CASE_SEED[(13, 130)], 13, 130, "xent")
    L, g, win = _clf(13).input_gradient(_dev(x), _dev(y), "xent", return_winners=True)
    win = win.cpu().numpy()
    ref = G.grad_model(_weights(13), x, y, "xent", winners=win)
    cut = G.grad_model(_weights(13), x, y, "xent", winners=win, detach_transforms=True)
    assert (_grad_err(cut["grad"], ref["grad"]) > 100 * TOL_GRAD).all()
    keep = keep_mask(ref)
    assert keep.any() and (_grad_err(g.cpu().numpy(), ref["grad"])[keep] <= TOL_GRAD).all()


def test_ties_go_to_the_lowest_row():
    import torch
    clf = _clf(13)
    x = make_case(5, 13, 65, "xent")[0][:2]
    first = clf.input_gradient(_dev(x), _dev(np.array([2, 7], np.int32)), "xent", return_winners=True)[2].cpu().numpy()[0]
    rows, counts = np.unique(first[~np.isin(first, (3, 40, 64))], return_counts=True)
    r = rows[np.argmax(counts)]                                         # a point that wins many columns moves to row 3
    x[0, [3, r]] = x[0, [r, 3]]
    x[0, 40] = x[0, 3]
    x[0, 64] = x[0, 3]
    x[1, :] = x[1, 0]                                                   # a cloud of identical points
    y = np.array([2, 7], np.int32)
    for loss in G.LOSSES:
        L, g, win = clf.input_gradient(_dev(x), _dev(y), loss, KAPPA, return_winners=True)
        win, g = win.cpu().numpy(), g.cpu().numpy()
        assert not np.isin(win[0], (40, 64)).any() and (win[0] == 3).any()
        assert not g[0, 40].any() and not g[0, 64].any()
        assert not win[1].any() and not g[1, 1:].any()
    L, g = clf.input_gradient(_dev(x), _dev(np.array([2, 7], np.int32)), "xent")
    assert g[1, 0].abs().max().item() > 0 and g[0, 3].abs().max().item() > 0
    assert torch.isfinite(g).all()


def test_rows_that_win_nothing_have_zero_gradient():
    clf = _clf(40)
    x, y = make_case(9, 40, 130, "cw_targeted")
    L, g, win = clf.input_gradient(_dev(x), _dev(y), "cw_targeted", KAPPA, return_winners=True)
    win, g = win.cpu().numpy(), g.cpu().numpy()
    some = 0
    for c in range(CLOUDS):
        losers = np.setdiff1d(np.arange(130), np.unique(win[c]))
        some += len(losers)
        assert not g[c, losers].any()
        assert np.abs(g[c]).max() > 0
    assert some > 0


def test_bit_exact_invariances():
    import torch
    clf = _clf(13)
    n = 130
    cloud, y = make_case(31, 13, n, "cw_targeted", clouds=1)
    others, yo = make_case(32, 13, n, "cw_targeted", clouds=70)
    alone = clf.input_gradient(_dev(cloud), _dev(y), "cw_targeted", KAPPA, return_logits=True, return_winners=True)
    again = clf.input_gradient(_dev(cloud), _dev(y), "cw_targeted", KAPPA, return_logits=True, return_winners=True)
    assert all(torch.equal(a, b) for a, b in zip(alone, again))
    fwd_logits, fwd_labels = clf.forward(_dev(cloud))
    assert torch.equal(alone[2], fwd_logits)
    for size, pos in ((3, 1), (33, 0), (33, 32), (70, 65)):              # 70: past the op's chunk of 64 clouds
        batch, yb = others[:size].copy(), yo[:size].copy()
        batch[pos], yb[pos] = cloud[0], y[0]
        got = clf.input_gradient(_dev(batch), _dev(yb), "cw_targeted", KAPPA, return_logits=True, return_winners=True)
        assert all(torch.equal(a[pos], b[0]) for a, b in zip(got, alone)), (size, pos)
    # on a side stream: the delayed-call protocol of tests/_stream_order.py (behind a pending delay, over scratch that holds
    # another cloud's values: the default stream's bits, and the host is not blocked)
    import _stream_order as SO
    SO.check_call("classifier.input_gradient",
                  lambda xd, yd: clf.input_gradient(xd, yd, "cw_targeted", KAPPA, return_logits=True, return_winners=True),
                  [_dev(others[:1]), _dev(((y + 1) % 13).astype(y.dtype))], [_dev(cloud), _dev(y)], keep=clf)


def test_point_permutation_permutes_winners_and_gradient():
    clf = _clf(13)
    n = 130
    x, y = make_case(CASE_SEED[(13, n)][:1], 13, n, "xent")
    perm = np.random.default_rng(4).permutation(n)
    L0, g0, w0 = (t.cpu().numpy() for t in clf.input_gradient(_dev(x), _dev(y), "xent", return_winners=True))
    L1, g1, w1 = (t.cpu().numpy() for t in clf.input_gradient(_dev(x[:, perm]), _dev(y), "xent", return_winners=True))
    ref = G.grad_model(_weights(13), x, y, "xent")
    assert ref["margin_pool"][0] > 0                                    # no tied maxima: the winners are points, not positions
    live = ref["pooled"] > 0
    assert np.array_equal(perm[w1][live], w0[live]) and not w1[~live].any() and not w0[~live].any()
    assert L0[0] == L1[0]                                               # the forward does not depend on the order of points
    assert (_grad_err(g1, g0[:, perm].astype(np.float64)) <= TOL_GRAD).all()


def test_nan_cloud_and_bad_label_are_isolated():
    import torch
    clf = _clf(13)
    x, y = make_case(41, 13, 130, "xent", clouds=4)
    clean = clf.input_gradient(_dev(x), _dev(y), "xent", return_logits=True, return_winners=True)
    bad = x.copy()
    bad[2, 5, 1] = np.nan
    bad[2, 77] = np.inf
    got = clf.input_gradient(_dev(bad), _dev(y), "xent", return_logits=True, return_winners=True)
    for c in (0, 1, 3):
        assert all(torch.equal(a[c], b[c]) for a, b in zip(got, clean))
    for labels in ([0, 13, 0, 0], [0, -1, 0, 0], [0, 2 ** 30, 0, 0]):
        yb = y.copy()
        yb[1] = labels[1]
        for loss in G.LOSSES:
            ok = clf.input_gradient(_dev(x), _dev(y), loss, KAPPA, return_logits=True, return_winners=True)
            got = clf.input_gradient(_dev(x), _dev(yb), loss, KAPPA, return_logits=True, return_winners=True)
            assert torch.isnan(got[0][1]) and torch.isnan(got[1][1]).all()
            assert torch.equal(got[2], ok[2])
            for c in (0, 2, 3):
                assert all(torch.equal(a[c], b[c]) for a, b in zip(got, ok))


def _raw(clf, b, n, x, y, kind, kappa, loss, logits, win, grad, ws):
    import torch
    from geometric_adv_amd import _lib
    with torch.cuda.device(clf.device):
        return _lib.lib().geoadv_cls_input_grad(clf.handle, b, n, _lib.ptr(x), _lib.ptr(y), kind, kappa, _lib.ptr(loss),
                                                _lib.ptr(logits), _lib.ptr(win), _lib.ptr(grad), _lib.ptr(ws), _lib.stream_handle())


def test_refusals_write_nothing():
    import torch
    from geometric_adv_amd import _abi, _lib
    clf = _clf(13)
    x = _dev(make_case(1, 13, 8, "xent", clouds=2)[0])
    y = _dev(np.array([1, 2], np.int32))
    ws = torch.empty(int(_lib.lib().geoadv_cls_input_grad_workspace_bytes(clf.handle, 2, 16385)) + (1 << 20), dtype=torch.uint8, device="cuda:0")
    big = torch.zeros((1, 16385, 3), device="cuda:0")
    cases = [(2, 0, x, 0, 0.0), (1, 16385, big, 0, 0.0), (0, 8, x, 0, 0.0), (2, 8, x, 0, -0.5), (2, 8, x, 0, float("nan")),
             (2, 8, x, 0, float("inf")), (2, 8, x, 3, 0.0), (2, 8, x, -1, 0.0)]
    for b, n, pts, kind, kappa in cases:
        outs = [torch.full((2,), 7.0, device="cuda:0"), torch.full((2, 13), 7.0, device="cuda:0"),
                torch.full((2, 3, 1024), 7, dtype=torch.int32, device="cuda:0"), torch.full((2, 8, 3), 7.0, device="cuda:0")]
        assert _raw(clf, b, n, pts, y, kind, kappa, *outs, ws) == _abi.GEOADV_EINVAL, (b, n, kind, kappa)
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs)
    # the CW kinds need two classes
    from geometric_adv_amd import cls_weights as CW
    from geometric_adv_amd.classifier import PointNetClassifier
    one = PointNetClassifier(None, num_classes=1, weights=CW.synthetic_weights(1, seed=1))
    y0 = _dev(np.zeros(2, np.int32))
    for kind in (_abi.GEOADV_CLS_LOSS_CW_TARGETED, _abi.GEOADV_CLS_LOSS_CW_UNTARGETED):
        outs = [torch.full((2,), 7.0, device="cuda:0"), torch.full((2, 1), 7.0, device="cuda:0"),
                torch.full((2, 3, 1024), 7, dtype=torch.int32, device="cuda:0"), torch.full((2, 8, 3), 7.0, device="cuda:0")]
        assert _raw(one, 2, 8, x, y0, kind, 0.0, *outs, ws) == _abi.GEOADV_EINVAL
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs)
    L, g = one.input_gradient(x, y0, "xent")                            # one class: the cross entropy is 0, its gradient too
    assert not L.any() and not g.any()
    with pytest.raises(ValueError):
        clf.input_gradient(x, y.to(torch.int64))
    with pytest.raises(ValueError):
        clf.input_gradient(x, y, loss="hinge")


def test_the_largest_cloud_runs():
    """n = 16384, b = 1: finite and sparse, its logits the forward's.  (The float64 model holds three [16384 x 1024]
    float64 layers with their autograd copies at this size -- beyond a few seconds -- so it is not compared here.)"""
    clf = _clf(13)
    n = 16384
    x, y = make_case(51, 13, n, "cw_targeted", clouds=1)
    L, g, logits, win = clf.input_gradient(_dev(x), _dev(y), "cw_targeted", KAPPA, return_logits=True, return_winners=True)
    win, g = win.cpu().numpy(), g.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(L.cpu().numpy()).all()
    rows = np.unique(win[0])
    assert len(rows) <= 3 * 1024 and rows.max() < n and rows.max() > 1024        # winners beyond the first 1024 rows
    losers = np.setdiff1d(np.arange(n), rows)
    assert not g[0, losers].any() and np.abs(g[0]).max() > 0
    fwd = clf.forward(_dev(x))[0]
    assert np.array_equal(logits.cpu().numpy(), fwd.cpu().numpy())
