"""CPU: the float64 model of the classifier training step (tests/_cls_train_model64.py), the schedules, the initialiser, the
dropout generator and the checkpoint names of the trainer's export."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cls_train_model64 as M  # noqa: E402
from geometric_adv_amd import cls_weights as CW, tf_checkpoint  # noqa: E402


def _tiny(seed=0, B=3, N=8, nc=4):
    rng = np.random.default_rng(seed)
    w = CW.synthetic_weights(nc, seed)
    x = rng.random((B, N, 3)) - 0.5
    y = rng.integers(0, nc, B)
    return w, x, y


def test_model_gradients_match_central_differences():
    """d loss / d variable of the model against central differences on entries of every layer (tiny instance, fixed masks)."""
    w, x, y = _tiny()
    nc = 4
    params = {k: v.clone().requires_grad_(True) for k, v in M.to_params(w, nc).items()}
    masks = [torch.tensor(M.keep_mask(3, 0, 0, 3, 512)), torch.tensor(M.keep_mask(3, 0, 1, 3, 256))]
    xt, yt = torch.tensor(x), torch.tensor(y)
    loss, _ = M.forward(params, xt, yt, masks)
    loss.backward()
    rng = np.random.default_rng(1)
    worst = 0.0
    with torch.no_grad():
        for name, p in params.items():
            for _ in range(2):
                i = int(rng.integers(0, p.numel()))
                h = 1e-6
                old = p.view(-1)[i].item()
                p.view(-1)[i] = old + h
                lp = M.forward(params, xt, yt, masks)[0].item()
                p.view(-1)[i] = old - h
                lm = M.forward(params, xt, yt, masks)[0].item()
                p.view(-1)[i] = old
                fd = (lp - lm) / (2 * h)
                g = p.grad.view(-1)[i].item()
                scale = max(1e-3, float(p.grad.abs().max()))
                worst = max(worst, abs(fd - g) / scale)
    assert worst < 1e-4, worst            # measured 2.6e-5: a central difference of step 1e-6 across BN-coupled ReLUs


def test_model_step_is_deterministic_and_moves_every_variable():
    w, x, y = _tiny(2)
    a = M.step(w, x, y, 4, step_k=3, seed=5)
    b = M.step(w, x, y, 4, step_k=3, seed=5)
    assert a["loss"] == b["loss"]
    for k in a["grads"]:
        assert np.array_equal(a["grads"][k], b["grads"][k])
    # every variable but the conv / fc biases that feed a batch norm (their gradient is zero up to rounding)
    fed = set(s + "/biases" for s, _, _, bn, _ in CW.LAYERS if bn)
    still = [k for k in CW.trainable_names() if k not in fed and np.allclose(a["new_weights"][k], w[k], rtol=0, atol=1e-7)]
    assert not still, still


def _own_pins(ref):
    return {"relu": {k: v.copy() for k, v in ref["relu_mask"].items()}, "dropout": [m.copy() for m in ref["masks"]]}


def test_own_decisions_pinned_reproduce_the_model_bit_for_bit():
    """Pinning fp64's own ReLU masks, pool rows and dropout masks changes nothing and reports no disagreement."""
    w, x, y = _tiny(3, B=3, N=16)
    ref = M.step(w, x, y, 4, seed=2)
    got = M.step(w, x, y, 4, seed=2, pins=_own_pins(ref), force_argmax=ref["argmax"])
    assert got["loss"] == ref["loss"]
    for k in ref["grads"]:
        assert np.array_equal(got["grads"][k], ref["grads"][k]), k
    for k in ("logits", "t1", "t2"):
        assert np.array_equal(got[k], ref[k]), k
    rep = M.pin_disagreements(got)
    assert set(rep) == set(ref["relu_mask"]) | {"pool0", "pool1", "pool2"}
    assert all(v == (0, 0.0) for v in rep.values()), rep


@pytest.mark.parametrize("scope", ["conv4", "transform_net1/tfc1"])
def test_a_flipped_relu_pin_moves_the_gradients_and_is_reported(scope):
    """Flipping the pin of the layer's ReLU input closest to zero: one disagreement, reported at that input's |z|; the
    gradients move (the row's share through the flipped unit).  tfc1 has no dropout that could hide the flip."""
    w, x, y = _tiny(4, B=3, N=16)
    ref = M.step(w, x, y, 4, seed=1)
    pins = _own_pins(ref)
    flat = pins["relu"][scope].reshape(-1)
    i = ref["relu_closest"][scope]
    flat[i] = not flat[i]
    got = M.step(w, x, y, 4, seed=1, pins=pins, force_argmax=ref["argmax"])
    rep = M.pin_disagreements(got)
    assert rep[scope] == (1, ref["relu_margin"][scope]), rep[scope]
    # later layers move by the flipped unit's share: only inputs that close to zero may change side there
    assert all(v[1] < 1e-5 for k, v in rep.items() if k != scope), rep
    moved = max(float(np.abs(got["grads"][k] - g).max()) for k, g in ref["grads"].items())
    assert moved > 1e-9, moved


def test_a_forced_pool_row_is_reported_with_its_gap():
    w, x, y = _tiny(5, B=2, N=16)
    ref = M.step(w, x, y, 4, seed=0)
    arg = [a.copy() for a in ref["argmax"]]
    arg[2][1, 7] = (arg[2][1, 7] + 1) % 16
    got = M.step(w, x, y, 4, seed=0, pins=_own_pins(ref), force_argmax=arg)
    cnt, gap = M.pin_disagreements(got)["pool2"]
    assert cnt == 1 and gap > 0
    assert not np.array_equal(got["grads"]["conv5/weights"], ref["grads"]["conv5/weights"])


@pytest.mark.parametrize("B,decay_step", [(32, 200000), (7, 100)])
def test_schedule_staircase_edges(B, decay_step):
    k_edge = -(-decay_step // B)                  # first step with k * B >= decay_step
    lr0, d0 = M.schedule(k_edge - 1, B, 0.001, decay_step, 0.7)
    lr1, d1 = M.schedule(k_edge, B, 0.001, decay_step, 0.7)
    assert lr0 == 0.001 and d0 == 0.5
    assert np.isclose(lr1, 0.0007) and d1 == 0.75
    assert M.schedule(10 ** 9, B, 0.001, decay_step, 0.7)[0] == 1e-5       # the clip
    assert M.schedule(10 ** 9, B, 0.001, decay_step, 0.7)[1] == 0.99


def test_initial_weights_bounds_and_shapes():
    w = CW.initial_weights(13, 0)
    assert set(w) == set(CW.variable_names())
    assert np.isclose(CW.xavier_bound("conv1"), np.sqrt(6.0 / (3 + 192)))
    assert np.isclose(CW.xavier_bound("transform_net1/tconv1"), np.sqrt(6.0 / (3 + 192)))
    assert np.isclose(CW.xavier_bound("conv5"), np.sqrt(6.0 / (128 + 1024)))
    assert np.isclose(CW.xavier_bound("fc3", 13), np.sqrt(6.0 / (256 + 13)))
    for scope, _, fo, bn, shape in CW.LAYERS:
        arr = w[scope + "/weights"]
        assert arr.shape == tuple(13 if d is None else d for d in shape)
        if scope.endswith(("transform_XYZ", "transform_feat")):
            assert not arr.any()
        else:
            b = CW.xavier_bound(scope, 13)
            assert np.abs(arr).max() <= b and np.abs(arr).max() > 0.9 * b
        assert not w[scope + "/biases"].any()
        if bn:
            n = CW.bn_names(scope)
            assert (w[n["gamma"]] == 1).all() and not w[n["beta"]].any() and not w[n["mean"]].any() and not w[n["var"]].any()
    a, b = CW.initial_weights(13, 1), CW.initial_weights(13, 1)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_dropout_generator_keep_rate_and_keys():
    m = M.keep_mask(0, 0, 0, 32, 512)
    assert abs(m.mean() - 0.7) < 0.01
    assert not np.array_equal(m, M.keep_mask(0, 1, 0, 32, 512))           # the step moves it
    assert not np.array_equal(m[:, :256], M.keep_mask(0, 0, 1, 32, 256))  # so does the layer
    assert not np.array_equal(m, M.keep_mask(1, 0, 0, 32, 512))           # and the seed


def test_slot_names_and_checkpoint_round_trip(tmp_path):
    names = CW.variable_names()
    adam = CW.slot_names("adam")
    assert len(adam) == 2 * len(CW.trainable_names()) + 2 and "conv1/weights/Adam_1" in adam and "beta1_power" in adam
    assert CW.slot_names("momentum")[0] == CW.LAYERS[0][0] + "/weights/Momentum"
    w = CW.initial_weights(13, 0)
    full = dict(w)
    for n in adam:
        full[n] = np.zeros_like(w[n.rsplit("/", 1)[0]]) if n.endswith(("/Adam", "/Adam_1")) else np.array(0.9, np.float32)
    full[CW.STEP_NAME] = np.array(7, np.int32)
    prefix = str(tmp_path / "model-001.ckpt")
    tf_checkpoint.write_checkpoint(prefix, full)
    got = CW.load(prefix)
    assert set(got) == set(names)
    listed = set(n for n, _ in tf_checkpoint.list_variables(prefix))
    assert listed == set(names) | set(adam) | {CW.STEP_NAME}
    assert int(tf_checkpoint.load_checkpoint(prefix, lambda n: n == CW.STEP_NAME)[CW.STEP_NAME]) == 7
