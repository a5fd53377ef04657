"""GPU: the voted evaluation of the classifier (csrc/cls_eval.hip through geoadv_rotate_y, geoadv_cls_evaluate,
ops.rotate_point_cloud_by_angle and PointNetClassifier.evaluate_batch / evaluate): the rotation against the reference's
provider.rotate_point_cloud_by_angle (tests/golden/classifier_eval.npz), the closing kernel's loss against cls_trainer._loss64
on the logits and T2 of the same forward, the votes against separate forward calls, ties, chunking, refusals and streams.

MEASURED on the MI355X: the largest error / bound of the loss over the closing-kernel cases is 0.015 (the logit spread of
200; below 0.01 elsewhere); DESIGN.md, 'Voted evaluation'.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import _cls_model64  # noqa: F401  (the float64 yardstick of the forward; the loss yardstick here is cls_trainer._loss64)
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _clouds(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3)) - 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _weights(num_classes, kind="synthetic"):
    """cls_weights.synthetic_weights, or that set with one layer replaced: 'perm' -- T2 a signed permutation (exactly
    orthogonal), 'half' -- T2 all 0.5, 'spread' -- logits -100 ... 100 whatever the input, 'tie' / 'second' -- two classes
    with equal logits / with class 1 ahead."""
    from geometric_adv_amd import cls_weights as CW
    w = dict(CW.synthetic_weights(num_classes, seed=100 + num_classes))
    if kind in ("perm", "half"):
        w["transform_net2/transform_feat/weights"] = np.zeros((256, 4096), np.float32)
        if kind == "perm":
            rng = np.random.default_rng(3)
            t = np.zeros((64, 64), np.float32)
            t[np.arange(64), rng.permutation(64)] = rng.choice(np.array([-1.0, 1.0], np.float32), 64)
        else:
            t = np.full((64, 64), 0.5, np.float32)
        w["transform_net2/transform_feat/biases"] = (t - np.eye(64, dtype=np.float32)).reshape(-1)     # (the library adds I)
    elif kind in ("spread", "tie", "second"):
        w["fc3/weights"] = np.zeros((256, num_classes), np.float32)
        w["fc3/biases"] = {"spread": np.linspace(-100.0, 100.0, num_classes), "tie": np.full(num_classes, 0.25),
                           "second": np.array([0.25, 0.5])}[kind].astype(np.float32)
    elif kind != "synthetic":
        raise ValueError(kind)
    return w


@functools.lru_cache(maxsize=None)
def _clf(num_classes, kind="synthetic", batch_size=10):
    from geometric_adv_amd.classifier import PointNetClassifier
    return PointNetClassifier(None, num_classes=num_classes, weights=_weights(num_classes, kind), batch_size=batch_size)


def _labels(seed, b, num_classes):
    return np.random.default_rng(seed).integers(0, num_classes, b).astype(np.int32)


# ---- rotation ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "classifier_eval.npz"))


ROT_SHAPES = [(1, 1), (3, 33), (5, 64), (2, 100), (1, 16384)]


def test_rotation_golden_covers_the_cases():
    g = _golden()
    angles = g["rot_angles"]
    assert len(angles) == 5 and angles[0] == 0.0 and angles[3] == np.pi and angles[4] > 2 * np.pi
    assert np.isclose(angles[1], 2 * np.pi / 3) and np.isclose(angles[2], 2 * np.pi * 5 / 12)
    for b, n in ROT_SHAPES:
        assert g["rot_in__%dx%d" % (b, n)].shape == (b, n, 3)


@pytest.mark.parametrize("offset", [4, 5], ids=["aligned16", "unaligned"])
@pytest.mark.parametrize("b,n", ROT_SHAPES)
def test_rotation_vs_reference_inside_guards(b, n, offset):
    """geoadv_rotate_y straight through the C interface: the input inside a NaN-filled buffer, the output inside a
    pattern-filled one, at a 16-byte aligned offset (the four-points-per-thread body and its tail) and at an unaligned one
    (the one-point-per-thread form).  Equal to the reference at angle 0, within one float32 ulp elsewhere."""
    import torch
    from geometric_adv_amd import _lib
    g = _golden()
    x = g["rot_in__%dx%d" % (b, n)]
    count, pad = b * n * 3, 64
    src = torch.full((count + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda:0")
    src[offset:offset + count] = _dev(x.reshape(-1))
    L = _lib.lib()
    for k, angle in enumerate(g["rot_angles"]):
        dst = torch.full((count + 2 * pad,), 12345.0, dtype=torch.float32, device="cuda:0")
        st = L.geoadv_rotate_y(b, n, ctypes.c_void_p(src.data_ptr() + 4 * offset), ctypes.c_double(float(np.cos(angle))),
                               ctypes.c_double(float(np.sin(angle))), ctypes.c_void_p(dst.data_ptr() + 4 * offset),
                               _lib.stream_handle())
        _lib.check(st, "rotate_y")
        out = dst.cpu().numpy()
        assert np.all(out[:offset] == 12345.0) and np.all(out[offset + count:] == 12345.0), "a guard changed"
        got, want = out[offset:offset + count].reshape(b, n, 3), g["rot_out__%dx%d__%d" % (b, n, k)]
        if k == 0:
            assert np.all(got == want)
        else:
            ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
            assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp), "angle %r" % float(angle)
    assert torch.isnan(src[:offset]).all() and torch.isnan(src[offset + count:]).all()


def test_rotation_op_wrapper():
    from geometric_adv_amd import ops
    g = _golden()
    x = g["rot_in__3x33"]
    got = ops.rotate_point_cloud_by_angle(_dev(x), float(g["rot_angles"][0])).cpu().numpy()
    assert got.dtype == np.float32 and np.all(got == g["rot_out__3x33__0"])
    got = ops.rotate_point_cloud_by_angle(_dev(x), float(g["rot_angles"][4])).cpu().numpy()
    want = g["rot_out__3x33__4"]
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want))))
    with pytest.raises(ValueError):
        ops.rotate_point_cloud_by_angle(_dev(np.zeros((2, 5, 2), np.float32)), 0.0)


# ---- the closing kernel, through geoadv_cls_evaluate with one vote -------------------------------------------------------
def _loss_bound(logits, t2):
    """The issue's bound on |loss - _loss64|, in float64 from the operands: per cloud |dCE| <= (C + 8) u max(1, |z|max + log C)
    and, with delta_ij = 66 u sum_k |t_ik||t_jk| and e = T T^T - I, |dreg| <= sum_ij (|e_ij| delta_ij + delta_ij^2 / 2) + 4096 u reg;
    the loss is mean_b(CE) + 0.001 sum_b(reg)."""
    z = np.asarray(logits, np.float64)
    C = z.shape[1]
    d_ce = (C + 8) * U * np.maximum(1.0, np.abs(z).max(axis=1) + np.log(C))
    t = np.asarray(t2, np.float64).reshape(-1, 64, 64)
    e = t @ t.transpose(0, 2, 1) - np.eye(64)
    delta = 66 * U * (np.abs(t) @ np.abs(t).transpose(0, 2, 1))
    reg = 0.5 * (e ** 2).sum(axis=(1, 2))
    d_reg = (np.abs(e) * delta + 0.5 * delta ** 2).sum(axis=(1, 2)) + 4096 * U * reg
    return d_ce.mean() + 0.001 * d_reg.sum()


def _check_one_vote(clf, x, labels, angle=0.0):
    """loss, pred, pred_sum and vote_counts of a one-vote evaluate_batch against forward(transforms=True) on the same rotated
    input; returns the loss's error / bound."""
    from geometric_adv_amd import ops
    from geometric_adv_amd.cls_trainer import _loss64
    assert angle == 0.0
    loss, pred, psum, counts = clf.evaluate_batch(_dev(x), _dev(labels), 1)
    logits, lab, _, t2 = clf.forward(ops.rotate_point_cloud_by_angle(_dev(x), angle), transforms=True)
    logits, lab, t2 = logits.cpu().numpy(), lab.cpu().numpy(), t2.cpu().numpy()
    assert loss.shape == (1,) and loss.dtype.is_floating_point
    want = _loss64(logits, labels, t2)
    bound = _loss_bound(logits, t2)
    got = float(loss.cpu().numpy()[0])
    assert np.isfinite(got) and np.isfinite(want)
    ratio = abs(got - want) / bound
    print("cls_evaluate loss: b=%d C=%d got %.9g want %.9g error %.3g bound %.3g ratio %.3g"
          % (len(x), logits.shape[1], got, want, abs(got - want), bound, ratio))
    assert abs(got - want) <= bound
    assert np.array_equal(psum.cpu().numpy(), logits.astype(np.float64))
    assert np.array_equal(pred.cpu().numpy(), np.argmax(logits, axis=1))
    assert np.array_equal(pred.cpu().numpy(), lab)
    onehot = np.zeros(logits.shape, np.int32)
    onehot[np.arange(len(lab)), lab] = 1
    assert np.array_equal(counts.cpu().numpy(), onehot)
    return ratio


@pytest.mark.parametrize("b,num_classes", [(1, 13), (3, 13), (5, 1), (7, 40), (33, 13), (2, 1024)])
def test_closing_kernel_loss_vs_loss64(b, num_classes):
    _check_one_vote(_clf(num_classes), _clouds(40 + b, b, 100), _labels(b, b, num_classes))


def test_closing_kernel_orthogonal_t2_has_no_regulariser():
    from geometric_adv_amd.cls_trainer import _loss64
    clf = _clf(13, "perm")
    x, labels = _clouds(51, 3, 64), _labels(51, 3, 13)
    _check_one_vote(clf, x, labels)
    logits, _, _, t2 = clf.forward(_dev(x), transforms=True)
    t = t2.cpu().numpy().astype(np.float64)
    assert np.array_equal(t @ t.transpose(0, 2, 1), np.broadcast_to(np.eye(64), (3, 64, 64)))        # exactly orthogonal
    # with the regulariser exactly 0 the loss is the float32 rounding of the float64 mean cross entropy
    loss = clf.evaluate_batch(_dev(x), _dev(labels), 1)[0].cpu().numpy()[0]
    want = _loss64(logits.cpu().numpy(), labels, t2.cpu().numpy())
    assert abs(float(loss) - want) <= 2 * U * abs(want)


def test_closing_kernel_t2_of_halves():
    clf = _clf(13, "half")
    x, labels = _clouds(52, 3, 64), _labels(52, 3, 13)
    _check_one_vote(clf, x, labels)
    t2 = clf.forward(_dev(x), transforms=True)[3].cpu().numpy()
    assert np.all(t2 == 0.5)
    loss = float(clf.evaluate_batch(_dev(x), _dev(labels), 1)[0].cpu().numpy()[0])
    assert loss > 0.001 * 3 * 0.5 * (4032 * 256 + 64 * 225)           # the regulariser is a SUM over the batch


def test_closing_kernel_logit_spread_of_200():
    clf = _clf(13, "spread")
    x = _clouds(53, 4, 64)
    labels = np.array([0, 12, 6, 3], np.int32)
    _check_one_vote(clf, x, labels)
    logits = clf.logits(_dev(x)).cpu().numpy()
    assert logits.max() - logits.min() == 200.0
    loss = float(clf.evaluate_batch(_dev(x), _dev(labels), 1)[0].cpu().numpy()[0])
    assert np.isfinite(loss) and loss > 0.25 * 200.0                   # (the label-0 cloud alone has a CE of 200)


# ---- votes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("votes", [1, 3, 12])
def test_votes_vs_separate_forwards(votes):
    from geometric_adv_amd import ops
    from geometric_adv_amd.cls_trainer import _loss64
    clf = _clf(13)
    b, n = 3, 100
    x, labels = _clouds(60, b, n), _labels(60, b, 13)
    loss, pred, psum, counts = (t.cpu().numpy() for t in clf.evaluate_batch(_dev(x), _dev(labels), votes))
    want_sum, want_counts = np.zeros((b, 13), np.float64), np.zeros((b, 13), np.int32)
    for v, angle in enumerate(clf.vote_angles(votes)):
        assert angle == v / float(votes) * np.pi * 2
        logits, lab, _, t2 = clf.forward(ops.rotate_point_cloud_by_angle(_dev(x), angle), transforms=True)
        logits = logits.cpu().numpy()
        want_sum += logits
        want_counts[np.arange(b), np.argmax(logits, axis=1)] += 1
        want = _loss64(logits, labels, t2.cpu().numpy())
        assert abs(float(loss[v]) - want) <= _loss_bound(logits, t2.cpu().numpy()), "vote %d" % v
    assert psum.dtype == np.float64 and np.array_equal(psum, want_sum)        # float64 sums of the same values in the same order
    assert np.array_equal(counts.sum(axis=1), np.full(b, votes)) and np.array_equal(counts, want_counts)
    assert np.array_equal(pred, np.argmax(psum, axis=1))
    if votes > 1:
        assert len(np.unique(loss)) > 1                                         # the votes do see different inputs


def test_ties_go_to_the_first_maximum():
    x = _clouds(61, 4, 50)
    pred, psum, counts = (t.cpu().numpy() for t in _clf(2, "tie").evaluate_batch(_dev(x), None, 3)[1:])
    assert np.all(psum[:, 0] == psum[:, 1]) and np.all(psum[:, 0] == 0.75)
    assert np.array_equal(pred, np.zeros(4, np.int32)) and np.array_equal(counts, np.tile(np.array([3, 0], np.int32), (4, 1)))
    pred, psum, counts = (t.cpu().numpy() for t in _clf(2, "second").evaluate_batch(_dev(x), None, 3)[1:])
    assert np.array_equal(pred, np.ones(4, np.int32)) and np.array_equal(counts, np.tile(np.array([0, 3], np.int32), (4, 1)))


def test_evaluate_with_a_ragged_last_chunk():
    """7 clouds in chunks of 3: the voted labels and, restated here, the reference's bookkeeping over the per-chunk losses."""
    votes, total, bs = 3, 7, 3
    clf = _clf(13, "synthetic", bs)
    x = _clouds(62, total, 100)
    labels = np.array([0, 5, 5, 12, 3, 0, 5], np.int64)
    res = clf.evaluate(x, labels, num_votes=votes)
    loss_sum, preds, chunk_losses = 0.0, [], []
    for s in range(0, total, bs):
        e = min(s + bs, total)
        loss, pred, _, _ = clf.evaluate_batch(_dev(x[s:e]), _dev(labels[s:e].astype(np.int32)), votes)
        chunk_losses.append(loss.cpu().numpy())
        batch_loss_sum = 0
        for v in range(votes):
            batch_loss_sum += float(chunk_losses[-1][v]) * (e - s) / float(votes)
        loss_sum += batch_loss_sum
        preds.append(pred.cpu().numpy())
    pred = np.concatenate(preds)
    assert res["pred"].dtype == np.int64 and np.array_equal(res["pred"], pred)
    assert np.array_equal(res["vote_loss"], np.stack(chunk_losses))
    assert abs(res["mean_loss"] - loss_sum / float(total)) <= 1e-12 * abs(loss_sum / float(total))
    assert res["accuracy"] == np.sum(pred == labels) / float(total)
    seen = [int(np.sum(labels == c)) for c in range(13)]
    correct = [int(np.sum((labels == c) & (pred == c))) for c in range(13)]
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.array(correct) / np.array(seen, dtype=np.float64)
    assert np.array_equal(res["class_accuracies"], want, equal_nan=True)
    assert np.isnan(res["class_accuracies"][1]) and not np.isnan(res["class_accuracies"][5])
    assert np.isnan(res["avg_class_acc"])                                       # np.mean over a NaN, as in the reference


# ---- labels, refusals, determinism ----------------------------------------------------------------------------------------
def test_no_labels_gives_predictions_without_loss():
    clf = _clf(13)
    x, labels = _clouds(63, 5, 100), _labels(63, 5, 13)
    with_labels = clf.evaluate_batch(_dev(x), _dev(labels), 3)
    without = clf.evaluate_batch(_dev(x), None, 3)
    assert without[0] is None
    for a, b in zip(with_labels[1:], without[1:]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    res = clf.evaluate(x, None, num_votes=3)
    assert np.array_equal(res["pred"], with_labels[1].cpu().numpy()) and res["mean_loss"] is None and res["accuracy"] is None


@pytest.mark.parametrize("bad", [13, -1, 2 ** 30])
def test_out_of_range_label_gives_nan_loss_only(bad):
    clf = _clf(13)
    x, labels = _clouds(64, 4, 100), _labels(64, 4, 13)
    good = [t.cpu().numpy() for t in clf.evaluate_batch(_dev(x), _dev(labels), 3)]
    wrong = labels.copy()
    wrong[2] = bad
    got = [t.cpu().numpy() for t in clf.evaluate_batch(_dev(x), _dev(wrong), 3)]
    assert np.all(np.isnan(got[0])) and np.all(np.isfinite(good[0]))
    for a, b in zip(good[1:], got[1:]):
        assert np.array_equal(a, b)
    again = [t.cpu().numpy() for t in clf.evaluate_batch(_dev(x), _dev(labels), 3)]    # the next call is untouched
    assert np.array_equal(again[0], good[0])
    with pytest.raises(ValueError, match="labels must lie"):                            # the host path refuses before upload
        clf.evaluate(x, wrong, num_votes=1)


@pytest.mark.parametrize("b,n,votes", [(2, 10, 0), (2, 10, 65), (2, 0, 1), (1, 16385, 1), (0, 10, 1)])
def test_refusals(b, n, votes):
    with pytest.raises(ValueError, match="cls_evaluate"):
        _clf(13).evaluate_batch(_dev(np.zeros((b, n, 3), np.float32)), None, votes)


def test_limits_are_accepted():
    clf = _clf(13)
    loss, pred, psum, counts = clf.evaluate_batch(_dev(_clouds(65, 1, 1)), _dev(np.array([4], np.int32)), 64)
    assert loss.shape == (64,) and bool(np.all(np.isfinite(loss.cpu().numpy()))) and int(counts.sum()) == 64
    pred = clf.evaluate_batch(_dev(_clouds(66, 1, 16384)), None, 1)[1]
    assert np.array_equal(pred.cpu().numpy().astype(np.int8), clf.classify(_clouds(66, 1, 16384)))


def test_two_runs_are_bit_equal_also_on_another_stream():
    import torch
    clf = _clf(13)
    x, labels = _dev(_clouds(67, 5, 300)), _dev(_labels(67, 5, 13))
    first = clf.evaluate_batch(x, labels, 4)
    second = clf.evaluate_batch(x, labels, 4)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert torch.equal(first[0].view(torch.int32), second[0].view(torch.int32))
    # on a side stream: the delayed-call protocol of tests/_stream_order.py (behind a pending delay, over scratch that holds
    # another batch's values: the default stream's bits, and the host is not blocked)
    import _stream_order as SO
    SO.check_call("classifier.evaluate_batch", lambda xd, yd: clf.evaluate_batch(xd, yd, 4),
                  [_dev(_clouds(66, 5, 300)), _dev((_labels(67, 5, 13) + 1) % 13)], [x, labels], keep=clf)


def test_vote_zero_is_classify_on_the_unrotated_input():
    clf = _clf(13)
    x = _clouds(68, 6, 257)
    pred = clf.evaluate_batch(_dev(x), None, 1)[1].cpu().numpy()
    assert np.array_equal(pred.astype(np.int8), clf.classify(x))
