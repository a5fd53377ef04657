"""GPU: the PointNet classifier (csrc/classifier.hip through geoadv_cls_* and classifier.PointNetClassifier) against the
float64 models of tests/_cls_model64.py, its invariances, isolation, refusals, streams and the run_classifier CLI."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import _cls_model64 as M

pytestmark = pytest.mark.gpu

# TOLERANCE.  Every layer is an fp32 dot product (fan-in 3 ... 1024) whose rounding is about sqrt(K) * 2^-24 of the
# magnitudes summed (the MFMA's fp32 accumulation, or the head's fmaf chain): 32 * 6e-8 = 2e-6 of the summed magnitudes for
# K = 1024.  The logits sit at the end of the longest chain -- T-Net1 (5 layers) -> T1, folded into conv1, conv2, T-Net2
# (5 layers) -> T2, folded into conv3, conv4, conv5, fc1, fc2, fc3: 17 dot products -- and every batch norm of the
# calibrated synthetic model divides by its layer's standard deviation, which sits well below the summed magnitudes when
# a layer's terms cancel (the fc heads: 1024 / 512 / 256 terms of both signs).  Measured on the MI355X: T1 / T2 within
# 9e-6 of float64 (10 dot products); logits within 2e-5 with 40 classes and within 7.5e-5 with 13 -- about 4 x what a
# torch-eager fp32 forward of the same graph reaches (its blocked GEMMs sum in shorter chains than the head kernel's
# sequential 1024-term fmaf chains; DESIGN.md, classifier row).  The tolerance is therefore the 1e-4 ceiling, not the 1e-5
# first estimated; the transposed-transform guard below still moves the logits by more than 100 x TOL.
TOL = 1e-4
B_ALL = 32


def _clouds(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3)) - 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _weights(num_classes):
    from geometric_adv_amd import cls_weights as CW
    return CW.synthetic_weights(num_classes, seed=num_classes)


@functools.lru_cache(maxsize=None)
def _clf(num_classes):
    from geometric_adv_amd.classifier import PointNetClassifier
    return PointNetClassifier(None, num_classes=num_classes, weights=_weights(num_classes))


@functools.lru_cache(maxsize=None)
def _ref(n, num_classes):
    x = _clouds(1000 + n, B_ALL, n)
    return (x,) + M.numpy_model(_weights(num_classes), x)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _err(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("num_classes", [13, 40])
@pytest.mark.parametrize("n", [2048, 2047, 1000, 100])
@pytest.mark.parametrize("b", [1, 10, 32])
def test_logits_and_transforms_vs_float64(b, n, num_classes):
    x, ref, t1, t2 = _ref(n, num_classes)
    logits, labels, g1, g2 = _clf(num_classes).forward(_dev(x[:b]), transforms=True)
    assert logits.shape == (b, num_classes)
    e = (_err(logits.cpu().numpy(), ref[:b]), _err(g1.cpu().numpy(), t1[:b]), _err(g2.cpu().numpy(), t2[:b]))
    assert max(e) <= TOL, "relative errors logits / T1 / T2: %s" % (e,)


@pytest.mark.parametrize("num_classes", [13, 40])
def test_labels_equal_float64_argmax(num_classes):
    checked = total = 0
    clf = _clf(num_classes)
    for n in (2048, 2047, 1000, 100):
        x, ref, _, _ = _ref(n, num_classes)
        got = clf.classify(x)
        assert got.dtype == np.int8 and got.shape == (B_ALL,)
        top2 = np.sort(ref, axis=1)[:, -2:]
        ok = (top2[:, 1] - top2[:, 0]) > 10 * TOL * max(1.0, np.abs(ref).max())
        assert np.array_equal(got[ok], np.argmax(ref, axis=1)[ok].astype(np.int8))
        checked += int(ok.sum())
        total += B_ALL
    assert checked >= 0.9 * total


def test_transposed_transforms_are_told_apart():
    """On the test weights, using T1^T / T2^T instead of T1 / T2 moves the logits far beyond the tolerance (> 100 x TOL)."""
    w = _weights(13)
    x = _clouds(7, 4, 1000)
    ref = M.numpy_model(w, x)[0]
    tr = M.numpy_model(w, x, transpose=True)[0]
    assert _err(tr, ref) > 100 * TOL
    got = _clf(13).logits(_dev(x)).cpu().numpy()
    assert _err(got, ref) <= TOL


def test_bit_exact_invariances():
    import torch
    clf = _clf(13)
    n = 2048
    x = _clouds(11, B_ALL, n)
    cloud = _clouds(12, 1, n)
    alone = clf.logits(_dev(cloud))
    for pos in (0, 17):
        batch = x.copy()
        batch[pos] = cloud[0]
        assert torch.equal(clf.logits(_dev(batch))[pos], alone[0])
    assert torch.equal(clf.logits(_dev(cloud)), alone)                   # a second run
    perm = np.random.default_rng(3).permutation(n)
    assert torch.equal(clf.logits(_dev(cloud[:, perm])), alone)
    half = _clouds(13, 1, 1024)
    assert torch.equal(clf.logits(_dev(np.concatenate([half, half], axis=1))), clf.logits(_dev(half)))


def test_nonfinite_cloud_is_isolated():
    import torch
    clf = _clf(13)
    x = _clouds(21, 8, 2000)
    clean = clf.logits(_dev(x))
    bad = x.copy()
    bad[3, 5] = np.nan
    bad[3, 100, 1] = np.inf
    bad[3, 1999, 2] = -np.inf
    got = clf.logits(_dev(bad))
    torch.cuda.synchronize()
    keep = [i for i in range(8) if i != 3]
    assert torch.equal(got[keep], clean[keep])


def test_refusals():
    import torch
    from geometric_adv_amd import _lib
    from geometric_adv_amd import cls_weights as CW
    from geometric_adv_amd.classifier import _ClsWeights
    lib = _lib.lib()
    canon = CW.canonical(_weights(13))
    hw = _ClsWeights()
    for f in ("w", "b", "gamma", "beta", "mean", "var"):
        arr = getattr(hw, f)
        for i, a in enumerate(canon[f]):
            arr[i] = a.ctypes.data if a is not None else None
    for nc in (0, 1025):
        hw.num_classes = nc
        h = ctypes.c_void_p()
        assert lib.geoadv_cls_create(ctypes.byref(h), ctypes.byref(hw)) == 1 and not h.value
    clf = _clf(13)
    for n in (0, 16385):
        with pytest.raises(ValueError, match="out of range"):
            clf.forward(torch.zeros((1, n, 3), device="cuda:0"))
        ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        x = torch.zeros((1, max(n, 1), 3), device="cuda:0")
        assert lib.geoadv_cls_forward(clf.handle, 1, n, _lib.ptr(x), None, None, None, None, _lib.ptr(ws), None) == 1
    x = torch.zeros((1, 16, 3), device="cuda:0")
    assert lib.geoadv_cls_forward(clf.handle, 0, 16, _lib.ptr(x), None, None, None, None, _lib.ptr(ws), None) == 1


def test_non_default_stream_same_bits():
    """The delayed-call protocol of tests/_stream_order.py: behind a pending delay on a side stream, over scratch that holds
    another batch's values, the forward gives the default stream's bits and does not block the host."""
    import _stream_order as SO
    clf = _clf(40)
    SO.check_call("classifier.forward", lambda x: clf.forward(x, transforms=True), [_dev(_clouds(30, 10, 1500))],
                  [_dev(_clouds(31, 10, 1500))], keep=clf)


def _eval_folder(root, n, classes, sizes, dist_weights):
    from geometric_adv_amd.attack_data import prepare_data_for_attack
    ev = root / "log" / "ae" / "eval"
    os.makedirs(ev)
    slice_idx = np.concatenate([[0], np.cumsum(sizes)])
    rec = _clouds(41, int(slice_idx[-1]), n)
    rng = np.random.default_rng(0)
    nn_idx = np.zeros((len(rec), len(rec)), np.int16)
    for s in range(len(rec)):
        for t in range(len(sizes)):
            nn_idx[s, slice_idx[t]:slice_idx[t + 1]] = rng.permutation(sizes[t])
    attack_idx = np.stack([rng.permutation(4)[:2] for _ in sizes])
    np.save(ev / "point_clouds_test_set_3l.npy", rec); np.save(ev / "reconstructions_test_set_3l.npy", rec)
    np.save(ev / "pc_classes_3l.npy", np.array(classes)); np.save(ev / "slice_idx_test_set_3l.npy", slice_idx)
    np.save(ev / "chamfer_nn_idx_complete_test_set_3l.npy", nn_idx)
    np.save(ev / "sel_idx.npy", attack_idx)
    att = ev / "attack_res"
    os.makedirs(att)
    with open(att / "attack_configuration.json", "w") as f:
        json.dump({"class_names": ["chair", "car"], "target_pc_idx_type": "chamfer_nn_complete", "num_pc_for_attack": 2,
                   "num_pc_for_target": 1, "correct_pred_only": 0, "dist_weight_list": dist_weights}, f)
    adv = {}
    for k, name in enumerate(("chair", "car")):
        os.makedirs(att / name)
        _, tgt = prepare_data_for_attack(np.array(classes), [name], ["chair", "car"], rec, slice_idx, attack_idx, 1, nn_idx, None)
        adv[name] = _clouds(50 + k, len(dist_weights) * len(tgt), n).reshape(len(dist_weights), len(tgt), n, 3)
        np.save(att / name / "adversarial_pc_recon.npy", adv[name])
    return ev, rec, slice_idx, attack_idx, nn_idx, adv


@pytest.mark.parametrize("store", ["npz", "ckpt"])
def test_run_classifier_cli_end_to_end(tmp_path, store):
    from geometric_adv_amd import cls_weights as CW, run_classifier, tf_checkpoint
    from geometric_adv_amd.attack_data import prepare_data_for_attack
    n, classes, sizes = 256, ["chair", "table", "car"], [4, 5, 4]
    w = _weights(13)
    cdir = tmp_path / "log" / "pointnet"
    os.makedirs(cdir)
    if store == "npz":
        CW.save_npz(str(cdir / "weights.npz"), w)
    else:
        tf_checkpoint.write_checkpoint(CW.checkpoint_prefix(str(cdir), 150), {**w, "batch": np.array(7, np.int64)})
    ev, rec, slice_idx, attack_idx, nn_idx, adv = _eval_folder(tmp_path, n, classes, sizes, [1.0])
    base = ["--top_dir", str(tmp_path), "--ae_folder", "log/ae", "--classifier_folder", "log/pointnet",
            "--attack_pc_idx", "log/ae/eval/sel_idx.npy", "--num_points", str(n)]
    run_classifier.main(base + ["--data_type", "target"])
    run_classifier.main(base + ["--data_type", "adversarial"])
    clf = _clf(13)
    for name in ("chair", "car"):
        _, tgt = prepare_data_for_attack(np.array(classes), [name], ["chair", "car"], rec, slice_idx, attack_idx, 1, nn_idx, None)
        got = np.load(ev / "attack_res" / "classifier_res_orig" / name / "target_pc_recon_pred.npy")
        assert got.dtype == np.int8 and got.shape == (1, len(tgt))
        assert np.array_equal(got[0], clf.classify(tgt))
        got = np.load(ev / "attack_res" / "classifier_res" / name / "adversarial_pc_recon_pred.npy")
        assert got.dtype == np.int8 and got.shape == (1, len(tgt))
        assert np.array_equal(got[0], clf.classify(adv[name][0]))
    assert os.path.exists(ev / "attack_res" / "classifier_res" / "classifier_configuration.json")
    with pytest.raises(SystemExit):
        run_classifier.main(base + ["--data_type", "after_defense"])


def test_run_classifier_selects_the_dist_weight(tmp_path):
    from geometric_adv_amd import cls_weights as CW, run_classifier
    n, classes, sizes = 128, ["chair", "table", "car"], [4, 5, 4]
    cdir = tmp_path / "log" / "pointnet"
    os.makedirs(cdir)
    CW.save_npz(str(cdir / "weights.npz"), _weights(13))
    ev, _, _, _, _, adv = _eval_folder(tmp_path, n, classes, sizes, [0.5, 2.0])
    base = ["--top_dir", str(tmp_path), "--ae_folder", "log/ae", "--classifier_folder", "log/pointnet",
            "--attack_pc_idx", "log/ae/eval/sel_idx.npy", "--num_points", str(n), "--data_type", "adversarial"]
    with pytest.raises(FileNotFoundError, match="source_target_norm_min_idx"):
        run_classifier.main(base)
    for name in ("chair", "car"):
        os.makedirs(ev / "attack_res" / name / "analysis_results")
        sel = np.arange(adv[name].shape[1]) % 2
        np.save(ev / "attack_res" / name / "analysis_results" / "source_target_norm_min_idx.npy", sel)
    run_classifier.main(base)
    clf = _clf(13)
    for name in ("chair", "car"):
        sel = np.arange(adv[name].shape[1]) % 2
        want = clf.classify(adv[name][sel, np.arange(len(sel))])
        assert np.array_equal(np.load(ev / "attack_res" / "classifier_res" / name / "adversarial_pc_recon_pred.npy")[0], want)
