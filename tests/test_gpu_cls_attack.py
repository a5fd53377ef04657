"""GPU: the white-box classifier attacks (geometric_adv_amd/cls_attack.py on PointNetClassifier.input_gradient) and the
run_cls_attack CLI: Adam's first step, the ifgsm box, successes confirmed by classify, keep-best, the CLI's files.

Shapes: 4 clouds of 128 points, 13 classes, at most 60 iterations.  Success on the synthetic weights is not guaranteed: the
sources (seed SEED of the generator below), the targets (the float64 model's prediction + SHIFT) and the parameters were
picked on the CPU, with the float64 model standing in for the classifier (_cls_grad_model64.ModelClassifier) in the same
ClassifierAttack loop, such that every cloud succeeds there with room (the figures are next to each parameter set)."""
import functools
import json
import os

import numpy as np
import pytest

import _cls_model64 as M

pytestmark = pytest.mark.gpu

B, N, C = 4, 128, 13
SEED, SHIFT = 7, 3
# picked on the CPU (see above); the comments are what the float64 stand-in gave for the four clouds
# cw: targeted succeeds at iterations 9 / 14 / 6 / 3 and on 34 / 34 / 30 / 54 of the 60 iterates; untargeted at iteration 1, on 58+
CW_ARGS = dict(method="cw", dist_type="l2", dist_weight=1.0, kappa=0.0, learning_rate=0.01, num_iterations=60)
# ifgsm: targeted succeeds at iterations 2 / 19 / 3 / 4 and on 55 / 10 / 56 / 56 iterates (eps 0.05 left cloud 1 two); untargeted on 59
IFGSM_ARGS = dict(method="ifgsm", eps=0.1, num_iterations=60)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _weights():
    from geometric_adv_amd import cls_weights as CW
    return CW.synthetic_weights(C, seed=C)


@functools.lru_cache(maxsize=None)
def _clf():
    from geometric_adv_amd.classifier import PointNetClassifier
    return PointNetClassifier(None, num_classes=C, weights=_weights(), batch_size=B)


@functools.lru_cache(maxsize=None)
def case():
    """(clouds, the float64 model's labels, targets)."""
    x = (np.random.default_rng(SEED).random((B, N, 3)) - 0.5).astype(np.float32)
    true = np.argmax(M.numpy_model(_weights(), x)[0], axis=1)
    return x, true.astype(np.int32), ((true + SHIFT) % C).astype(np.int32)


def test_first_cw_step_is_adams():
    """One CW iteration from a zero perturbation moves every coordinate by -lr g / (|g| + 1e-8), g from input_gradient.
    TOLERANCE: TF's form places epsilon after the bias correction, -lr g / (|g| + 1e-8 / sqrt(1 - beta2)), which differs
    from the line above by at most lr * 3.2e-7 / |g|; the sum x + pert rounds by half an ulp of a coordinate below 1
    (6e-8), the step itself by a few ulps of lr (4 * 2^-24 lr).  A coordinate without gradient does not move at all."""
    from geometric_adv_amd.cls_attack import ClassifierAttack
    import torch
    x, true, target = case()
    clf = _clf()
    lr = 0.01
    g = clf.input_gradient(_dev(x), _dev(target), "cw_targeted", 0.0)[1].cpu().numpy().astype(np.float64)
    metrics, adv = ClassifierAttack(clf, **dict(CW_ARGS, num_iterations=1, learning_rate=lr)).attack(x, target)
    assert not metrics[:, 0].any() and (metrics[:, 2] == -1).all()
    assert np.abs(g).max() > 0
    moved = adv.astype(np.float64) - x
    want = -lr * g / (np.abs(g) + 1e-8)
    tol = 6e-8 + 4 * 2.0 ** -24 * lr + lr * 3.2e-7 / np.maximum(np.abs(g), 3.2e-7)
    assert (np.abs(moved - want) <= tol).all()
    assert np.array_equal(adv[g == 0], x[g == 0]) and (g == 0).any()


@pytest.mark.parametrize("targeted", [True, False])
def test_ifgsm_never_leaves_the_box(targeted):
    from geometric_adv_amd.cls_attack import ClassifierAttack
    x, true, target = case()
    eps = np.float32(IFGSM_ARGS["eps"])
    seen = []
    atk = ClassifierAttack(_clf(), targeted=targeted, **IFGSM_ARGS, history=lambda it, adv, ok, D, loss: seen.append((adv - _dev(x)).abs().max()))
    metrics, adv = atk.attack(x, target if targeted else true)
    assert np.abs(adv - x).max() <= eps                                    # float32, exact
    assert len(seen) == IFGSM_ARGS["num_iterations"] and max(s.item() for s in seen) <= eps
    assert np.abs(adv - x).max() > 0


@pytest.mark.parametrize("method", ["cw", "ifgsm"])
@pytest.mark.parametrize("targeted", [True, False])
def test_successes_are_confirmed_by_classify(method, targeted):
    from geometric_adv_amd.cls_attack import ClassifierAttack
    x, true, target = case()
    clf = _clf()
    assert np.array_equal(clf.classify(x), true.astype(np.int8))            # the sources are classified as the float64 model does
    args = CW_ARGS if method == "cw" else IFGSM_ARGS
    metrics, adv = ClassifierAttack(clf, targeted=targeted, **args).attack(x, target if targeted else true)
    assert metrics.shape == (B, 4) and metrics.dtype == np.float32 and adv.shape == x.shape and adv.dtype == np.float32
    print(method, targeted, metrics)
    pred = clf.classify(adv)
    won = metrics[:, 0] == 1
    assert won.all(), "chosen on the CPU to succeed on every cloud"
    assert np.array_equal(pred[won], target[won].astype(np.int8)) if targeted else (pred[won] != true[won]).all()
    assert (metrics[won, 2] >= 0).all() and np.isfinite(metrics[won, 1]).all()
    assert ((metrics[~won, 2] == -1) & np.isinf(metrics[~won, 1])).all()


@pytest.mark.parametrize("method", ["cw", "ifgsm"])
def test_keep_best_returns_the_successful_iterate_of_smallest_distance(method):
    from geometric_adv_amd.cls_attack import ClassifierAttack
    x, true, target = case()
    hist = []
    args = CW_ARGS if method == "cw" else IFGSM_ARGS
    atk = ClassifierAttack(_clf(), targeted=True, **args,
                           history=lambda it, adv, ok, D, loss: hist.append((adv.clone(), ok.clone(), D.clone())))
    metrics, adv = atk.attack(x, target)
    assert len(hist) == args["num_iterations"]
    ok = np.stack([h[1].cpu().numpy() for h in hist])                       # (iterations, B)
    D = np.stack([h[2].cpu().numpy() for h in hist])
    assert ok.any(0).all()
    for c in range(B):
        its = np.nonzero(ok[:, c])[0]
        best = its[np.argmin(D[its, c])]                                    # the earliest among equal distances
        assert metrics[c, 0] == 1 and metrics[c, 2] == best and metrics[c, 1] == D[best, c]
        assert np.array_equal(adv[c], hist[best][0][c].cpu().numpy())
        assert ok[:, c].sum() > 1 and len(np.unique(D[its, c])) > 1         # there was something to choose from


def test_chamfer_distance_term_runs_through_nn_distance():
    from geometric_adv_amd.cls_attack import ClassifierAttack
    from geometric_adv_amd import ops
    x, true, target = case()
    metrics, adv = ClassifierAttack(_clf(), targeted=True, **dict(CW_ARGS, dist_type="chamfer", num_iterations=20)).attack(x, target)
    d1, _, d2, _ = ops.nn_distance(_dev(adv), _dev(x))
    D = (d1.mean(1) + d2.mean(1)).cpu().numpy()
    won = metrics[:, 0] == 1
    assert np.isfinite(metrics[:, 3]).all() and (np.abs(adv - x).max((1, 2)) > 0).all()
    assert np.allclose(metrics[won, 1], D[won], rtol=1e-5, atol=1e-9)


def _run_cli(top, out, extra):
    from geometric_adv_amd import run_cls_attack
    run_cls_attack.main(["--classifier_folder", "clf", "--num_classes", str(C), "--input", "clouds.npy", "--labels", "labels.npy",
                         "--batch_size", "3", "--num_iterations", "30", "--output_dir", out, "--top_dir", str(top)] + extra)
    return {f: open(os.path.join(str(top), out, f), "rb").read() for f in sorted(os.listdir(os.path.join(str(top), out)))}


@pytest.mark.parametrize("targeted", [True, False])
def test_cli_end_to_end(tmp_path, targeted):
    from geometric_adv_amd import cls_weights as CW, ops
    x, true, target = case()
    os.makedirs(str(tmp_path / "clf"))
    CW.save_npz(str(tmp_path / "clf" / "weights.npz"), _weights())
    np.save(str(tmp_path / "clouds.npy"), x)
    np.save(str(tmp_path / "labels.npy"), true)
    np.save(str(tmp_path / "targets.npy"), target)
    extra = ["--method", "cw"] + (["--target_labels", "targets.npy"] if targeted else [])
    first = _run_cli(tmp_path, "res", extra)
    assert sorted(first) == ["adversarial_metrics.npy", "adversarial_pc_input.npy", "adversarial_pred_labels.npy",
                             "cls_attack_configuration.json"]
    again = _run_cli(tmp_path, "res2", extra)
    assert {k: v for k, v in first.items() if k.endswith(".npy")} == {k: v for k, v in again.items() if k.endswith(".npy")}
    conf = json.load(open(str(tmp_path / "res" / "cls_attack_configuration.json")))
    assert conf["targeted"] is targeted and conf["method"] == "cw" and conf["num_iterations"] == 30 and conf["num_clouds"] == B
    conf2 = json.load(open(str(tmp_path / "res2" / "cls_attack_configuration.json")))
    assert {k: v for k, v in conf.items() if k != "output_dir"} == {k: v for k, v in conf2.items() if k != "output_dir"}
    adv = np.load(str(tmp_path / "res" / "adversarial_pc_input.npy"))
    metrics = np.load(str(tmp_path / "res" / "adversarial_metrics.npy"))
    pred = np.load(str(tmp_path / "res" / "adversarial_pred_labels.npy"))
    assert adv.shape == (B, N, 3) and adv.dtype == np.float32
    assert metrics.shape == (B, 4) and metrics.dtype == np.float32
    assert pred.shape == (B,) and pred.dtype == np.int8
    assert np.array_equal(pred, _clf().classify(adv))
    won = metrics[:, 0] == 1
    assert np.array_equal(pred[won], target[won].astype(np.int8)) if targeted else (pred[won] != true[won]).all()
    # the written clouds are what the defenses take
    o_pc, o_idx, o_num, inlier = ops.sor_filter(_dev(adv))
    assert tuple(o_pc.shape) == (B, N, 3) and tuple(o_idx.shape) == (B, N) and tuple(o_num.shape) == (B,) and tuple(inlier.shape) == (B, N, 3)
    assert tuple(ops.random_drop(_dev(adv), 16, seed=1).shape) == (B, N, 3)
