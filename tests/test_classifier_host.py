"""CPU: the PointNet classifier's float64 models, weights and checkpoint contract, and the ctypes mirror of
geoadv_cls_weights (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _cls_model64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clouds(seed, b, n):
    return np.random.default_rng(seed).random((b, n, 3)) - 0.5


@pytest.mark.parametrize("num_classes", [13, 40])
def test_two_float64_models_agree(num_classes):
    from geometric_adv_amd import cls_weights as CW
    w = CW.synthetic_weights(num_classes, seed=num_classes)
    x = _clouds(1, 3, 200)
    a, t1a, t2a = M.numpy_model(w, x)
    b, t1b, t2b = M.torch_model(w, x)
    assert a.shape == (3, num_classes)
    scale = max(1.0, np.abs(a).max())
    assert np.abs(a - b).max() <= 1e-10 * scale
    assert np.abs(t1a - t1b).max() <= 1e-10 and np.abs(t2a - t2b).max() <= 1e-10
    # the package's own float64 forward (used to calibrate the synthetic model) is a third opinion
    assert np.abs(CW.forward64(w, x) - a).max() <= 1e-10 * scale


def test_synthetic_model_is_calibrated_and_transforms_are_not_trivial():
    from geometric_adv_amd import cls_weights as CW
    w = CW.synthetic_weights(13, seed=0)
    _, t1, t2 = M.numpy_model(w, _clouds(2, 4, 256))
    for t, k in ((t1, 3), (t2, 64)):
        d = t - np.eye(k)
        assert np.abs(d).max() > 0.02                              # not the identity
        assert np.abs(t - t.transpose(0, 2, 1)).max() > 0.02        # not symmetric
    # calibration: pre-BN outputs of conv1 on the calibration batch are standardised
    x = CW.calibration_batch()
    _, t1c, _ = M.numpy_model(w, x)
    a = M._np_dense(np.matmul(x, t1c), w, "conv1").reshape(-1, 64)
    names = CW.bn_names("conv1")
    z = (a - w[names["mean"]]) / np.sqrt(w[names["var"]] + 1e-3)
    assert np.abs(z.mean(0)).max() < 1e-3 and np.abs(z.std(0) - 1).max() < 0.05      # (eps = 1e-3 against var)


def test_identity_is_added_exactly_once():
    """With zero transform weights and biases both T-Nets are the identity: the model equals the same model without them."""
    from geometric_adv_amd import cls_weights as CW
    w = dict(CW.synthetic_weights(13, seed=3))
    for s in ("transform_net1/transform_XYZ", "transform_net2/transform_feat"):
        w[s + "/weights"] = np.zeros_like(w[s + "/weights"])
        w[s + "/biases"] = np.zeros_like(w[s + "/biases"])
    x = _clouds(4, 2, 128)
    with_t, t1, t2 = M.numpy_model(w, x)
    without, _, _ = M.numpy_model(w, x, with_transforms=False)
    assert np.array_equal(t1, np.broadcast_to(np.eye(3), t1.shape)) and np.array_equal(t2, np.broadcast_to(np.eye(64), t2.shape))
    assert np.array_equal(with_t, without)
    assert np.allclose(M.torch_model(w, x)[0], without, rtol=0, atol=1e-10)


def test_variable_names_follow_the_graph():
    from geometric_adv_amd import cls_weights as CW
    names = set(CW.variable_names())
    for must in ["conv1/weights", "conv1/biases", "conv1/bn/beta", "conv1/bn/gamma",
                 "conv1/bn/conv1/bn/moments/Squeeze/ExponentialMovingAverage",
                 "conv1/bn/conv1/bn/moments/Squeeze_1/ExponentialMovingAverage",
                 "transform_net1/tconv2/weights", "transform_net2/transform_feat/biases", "fc3/weights",
                 "transform_net1/tconv1/bn/transform_net1/tconv1/bn/moments/Squeeze/ExponentialMovingAverage",
                 "fc1/bn/fc1/bn/moments/Squeeze_1/ExponentialMovingAverage",
                 "transform_net2/tfc1/bn/transform_net2/tfc1/bn/moments/Squeeze/ExponentialMovingAverage"]:
        assert must in names
    assert len(names) == 20 * 2 + 17 * 4
    assert "fc3/bn/gamma" not in names and "transform_net1/transform_XYZ/bn/beta" not in names


def test_checkpoint_round_trip(tmp_path):
    from geometric_adv_amd import cls_weights as CW, tf_checkpoint
    w = CW.synthetic_weights(13, seed=5)
    extra = {"batch": np.array(1234, dtype=np.int64), "conv1/weights/Adam": np.ones((1, 3, 1, 64), np.float32),
             "fc3/biases/Adam_1": np.ones(13, np.float32), "beta1_power": np.array(0.9, np.float32)}
    tf_checkpoint.write_checkpoint(CW.checkpoint_prefix(str(tmp_path), 150), {**w, **extra})
    got = CW.load(str(tmp_path), restore_epoch=150)
    assert sorted(got) == sorted(w)
    for k, v in w.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v)
    # the same through the prefix, and through an .npz
    got2 = CW.load(os.path.join(str(tmp_path), "model-150.ckpt"))
    assert all(np.array_equal(got2[k], w[k]) for k in w)
    CW.save_npz(str(tmp_path / "w.npz"), {**w, **{k: v for k, v in extra.items() if k != "batch"}})
    got3 = CW.load(str(tmp_path / "w.npz"))
    assert sorted(got3) == sorted(w) and all(np.array_equal(got3[k], w[k]) for k in w)
    # a missing variable is named
    gone = "transform_net2/tconv3/bn/transform_net2/tconv3/bn/moments/Squeeze_1/ExponentialMovingAverage"
    w2 = {k: v for k, v in w.items() if k not in (gone, "fc2/biases")}
    tf_checkpoint.write_checkpoint(str(tmp_path / "model-005.ckpt"), w2)
    with pytest.raises(KeyError) as e:
        CW.load(str(tmp_path), restore_epoch=5)
    assert gone in str(e.value) and "fc2/biases" in str(e.value)


def test_checkpoint_prefix_formats_the_epoch():
    from geometric_adv_amd import cls_weights as CW
    assert CW.checkpoint_prefix("d", 5) == os.path.join("d", "model-005.ckpt")
    assert CW.checkpoint_prefix("d", 50) == os.path.join("d", "model-050.ckpt")
    assert CW.checkpoint_prefix("d", 150) == os.path.join("d", "model-150.ckpt")


def test_canonical_layout():
    from geometric_adv_amd import cls_weights as CW
    w = CW.synthetic_weights(40, seed=1)
    c = CW.canonical(w)
    assert len(c["w"]) == 20
    assert c["w"][0].shape == (3, 64) and c["w"][5].shape == (256, 9) and c["w"][13].shape == (256, 4096)
    assert c["w"][19].shape == (256, 40) and c["b"][19].shape == (40,)
    for i in (5, 13, 19):
        assert c["gamma"][i] is None and c["var"][i] is None
    assert np.array_equal(c["w"][6], w["conv1/weights"].reshape(3, 64))


def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "geoadv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    defines = dict(re.findall(r"#define\s+(GEOADV_\w+)\s+(\d+)", text))
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+float\s*\*|int)\s*(.*)", decl)
        base = "int" if m.group(1) == "int" else "ptr"
        for item in m.group(2).split(","):
            item = item.strip().lstrip("*").strip()
            mm = re.match(r"(\w+)\s*(?:\[(\w+)\])?$", item)
            count = int(defines.get(mm.group(2), mm.group(2))) if mm.group(2) else 1
            fields.append((mm.group(1), base, count))
    return fields


def test_python_mirror_of_cls_weights_matches_the_header():
    from geometric_adv_amd.classifier import _ClsWeights
    want = _header_struct("geoadv_cls_weights")
    got = []
    for f, t in _ClsWeights._fields_:
        if t is ctypes.c_int:
            got.append((f, "int", 1))
        else:
            assert t._type_ is ctypes.c_void_p
            got.append((f, "ptr", t._length_))
    assert got == want
    assert want[0] == ("num_classes", "int", 1) and len(want) == 7
