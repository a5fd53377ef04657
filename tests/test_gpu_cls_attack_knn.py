"""GPU: the kNN outlier term and clip_linf of the white-box classifier attack (geometric_adv_amd/cls_attack.py on
ops.knn_outlier_loss) and their run_cls_attack flags: the defaults return what they returned, Adam's step with the term, the
box, the refusal, repeatability, the CLI's files.  The classifier, clouds and parameters of tests/test_gpu_cls_attack.py."""
import functools
import json
import os

import numpy as np
import pytest

import _cls_model64 as M

pytestmark = pytest.mark.gpu

B, N, C = 4, 128, 13
SEED, SHIFT = 7, 3
CW_ARGS = dict(method="cw", dist_type="l2", dist_weight=1.0, kappa=0.0, learning_rate=0.01, num_iterations=60)


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


@pytest.mark.parametrize("dist_type", ["l2", "chamfer"])
def test_defaults_return_the_bytes_they_returned(dist_type, monkeypatch):
    from geometric_adv_amd import ops
    from geometric_adv_amd.cls_attack import ClassifierAttack
    x, true, target = case()
    args = dict(CW_ARGS, dist_type=dist_type, num_iterations=20)
    want = ClassifierAttack(_clf(), **args).attack(x, target)

    def never(*a, **kw):
        raise AssertionError("the kNN op was called with knn_weight = 0")
    monkeypatch.setattr(ops, "knn_outlier_loss", never)
    got = ClassifierAttack(_clf(), **args, knn_weight=0.0, clip_linf=None).attack(x, target)
    assert want[0].tobytes() == got[0].tobytes() and want[1].tobytes() == got[1].tobytes()
    # and the loop without the term is x + pert, Adam, nothing else: its first step from input_gradient alone
    g = _clf().input_gradient(_dev(x), _dev(target), "cw_targeted", 0.0)[1]
    one = ClassifierAttack(_clf(), **dict(args, num_iterations=1)).attack(x, target)[1]
    import torch
    alpha_1 = 0.01 * np.sqrt(1.0 - 0.999) / (1.0 - 0.9)
    m, v = g * (1.0 - 0.9), g * g * (1.0 - 0.999)
    assert torch.equal(_dev(one), _dev(x) + (torch.zeros_like(g) - alpha_1 * m / (torch.sqrt(v) + 1e-8)))


@pytest.mark.parametrize("dist_type", ["l2", "chamfer"])
def test_adam_step_with_the_knn_term(dist_type):
    """Iterates 0 and 1 of the history satisfy the Adam update formed here from input_gradient, _distance and
    ops.knn_outlier_loss at iterate 0: the same tensor operations in the same order, so equality is to the bits."""
    import torch
    from geometric_adv_amd import ops
    from geometric_adv_amd.cls_attack import ADAM_BETA1, ADAM_BETA2, ADAM_EPS, ClassifierAttack
    x, true, target = case()
    hist = []
    args = dict(CW_ARGS, dist_type=dist_type, dist_weight=0.5, num_iterations=2)
    atk = ClassifierAttack(_clf(), **args, knn_weight=2.0, knn_k=5, knn_alpha=1.05,
                           history=lambda it, adv, ok, D, loss: hist.append((adv.clone(), D.clone(), loss.clone())))
    atk.attack(x, target)
    assert len(hist) == 2
    xd, lab = _dev(x), _dev(target)
    assert torch.equal(hist[0][0], xd)
    f, g = _clf().input_gradient(xd, lab, loss="cw_targeted", kappa=0.0, return_logits=True)[:2]
    pert = torch.zeros_like(xd)
    D, dD = atk._distance(xd, pert)
    K, dK = ops.knn_outlier_loss(xd, 5, 1.05)
    assert (K > 0).all() and (dK != 0).any(dim=2).any(dim=1).all()            # the term is there, in every cloud
    assert torch.equal(hist[0][2], f + 0.5 * (D + 2.0 * K.to(D.dtype)))
    assert torch.equal(hist[0][1], D)
    total = g + 0.5 * (dD + 2.0 * dK)
    alpha_1 = 0.01 * np.sqrt(1.0 - ADAM_BETA2) / (1.0 - ADAM_BETA1)
    m = torch.zeros_like(xd) + (total - torch.zeros_like(xd)) * (1.0 - ADAM_BETA1)
    v = torch.zeros_like(xd) + (total * total - torch.zeros_like(xd)) * (1.0 - ADAM_BETA2)
    pert = pert - alpha_1 * m / (torch.sqrt(v) + ADAM_EPS)
    assert torch.equal(hist[1][0], xd + pert)
    # the term moved the step: without it the iterate differs
    plain = []
    ClassifierAttack(_clf(), **args, history=lambda it, adv, ok, D, loss: plain.append(adv.clone())).attack(x, target)
    assert not torch.equal(plain[1], hist[1][0])


def test_clip_linf_holds_at_every_iterate():
    import torch
    from geometric_adv_amd.cls_attack import ClassifierAttack
    x, true, target = case()
    clip = np.float32(0.01)
    seen = []
    atk = ClassifierAttack(_clf(), **dict(CW_ARGS, num_iterations=30), knn_weight=2.0, clip_linf=0.01,
                           history=lambda it, adv, ok, D, loss: seen.append((adv - _dev(x)).abs().max()))
    metrics, adv = atk.attack(x, target)
    assert len(seen) == 30 and max(s.item() for s in seen) <= clip
    assert np.abs(adv - x).max() <= clip                                    # float32, exact
    assert max(s.item() for s in seen) > 0.99 * clip                        # the clamp was at work (Adam's steps are 0.01 each)
    free = ClassifierAttack(_clf(), **dict(CW_ARGS, num_iterations=30), knn_weight=2.0).attack(x, target)[1]
    assert np.abs(free - x).max() > clip


def test_ifgsm_refuses_the_knn_term():
    from geometric_adv_amd.cls_attack import ClassifierAttack
    with pytest.raises(ValueError):
        ClassifierAttack(_clf(), method="ifgsm", knn_weight=1.0)
    ClassifierAttack(_clf(), method="ifgsm", knn_weight=0.0)
    for bad in (dict(knn_weight=float("nan")), dict(knn_weight=1.0, knn_k=0), dict(knn_weight=1.0, knn_alpha=-1.0), dict(clip_linf=0.0)):
        with pytest.raises(ValueError):
            ClassifierAttack(_clf(), method="cw", **bad)


def test_two_runs_give_the_same_bytes():
    from geometric_adv_amd.cls_attack import ClassifierAttack
    x, true, target = case()
    args = dict(CW_ARGS, dist_type="chamfer", num_iterations=20)
    a = ClassifierAttack(_clf(), **args, knn_weight=2.0, clip_linf=0.05).attack(x, target)
    b = ClassifierAttack(_clf(), **args, knn_weight=2.0, clip_linf=0.05).attack(x, target)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.isfinite(a[0][:, 3]).all() and np.abs(a[1] - x).max() > 0


def _run_cli(top, out, extra):
    from geometric_adv_amd import run_cls_attack
    run_cls_attack.main(["--classifier_folder", "clf", "--num_classes", str(C), "--input", "clouds.npy", "--labels", "labels.npy",
                         "--batch_size", "3", "--num_iterations", "20", "--output_dir", out, "--top_dir", str(top)] + extra)
    return {f: open(os.path.join(str(top), out, f), "rb").read() for f in sorted(os.listdir(os.path.join(str(top), out)))}


def test_cli_with_the_knn_flags(tmp_path):
    from geometric_adv_amd import cls_weights as CW
    x, true, target = case()
    os.makedirs(str(tmp_path / "clf"))
    CW.save_npz(str(tmp_path / "clf" / "weights.npz"), _weights())
    np.save(str(tmp_path / "clouds.npy"), x)
    np.save(str(tmp_path / "labels.npy"), true)
    np.save(str(tmp_path / "targets.npy"), target)
    extra = ["--method", "cw", "--target_labels", "targets.npy", "--knn_weight", "2", "--knn_k", "5", "--clip_linf", "0.05"]
    first = _run_cli(tmp_path, "res", extra)
    assert sorted(first) == ["adversarial_metrics.npy", "adversarial_pc_input.npy", "adversarial_pred_labels.npy",
                             "cls_attack_configuration.json"]
    again = _run_cli(tmp_path, "res2", extra)
    assert {k: v for k, v in first.items() if k.endswith(".npy")} == {k: v for k, v in again.items() if k.endswith(".npy")}
    conf = json.load(open(str(tmp_path / "res" / "cls_attack_configuration.json")))
    assert conf["knn_weight"] == 2.0 and conf["knn_k"] == 5 and conf["knn_alpha"] == 1.05 and conf["clip_linf"] == 0.05
    adv = np.load(str(tmp_path / "res" / "adversarial_pc_input.npy"))
    assert adv.shape == (B, N, 3) and adv.dtype == np.float32 and np.abs(adv - x).max() <= np.float32(0.05)
    plain = _run_cli(tmp_path, "res3", extra[:4])
    assert plain["adversarial_pc_input.npy"] != first["adversarial_pc_input.npy"]
    conf3 = json.load(open(str(tmp_path / "res3" / "cls_attack_configuration.json")))
    assert conf3["knn_weight"] == 0.0 and conf3["clip_linf"] is None
