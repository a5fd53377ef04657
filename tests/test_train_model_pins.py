"""CPU: the fp64 training model with pinned discrete decisions (oracle/train_model.py forward(pins=...)), the reference the
full-size trainer tests compare the GPU step against.  Pinning the model's own decisions must change nothing, and a
pinned decision that fp64 would take the other way must be reported with its distance from the boundary."""
import numpy as np


def _model_and_batch(n=128, b=3, seed=5):
    from geometric_adv_amd import weights as W
    from oracle.train_model import TrainModel
    tm = TrainModel(W.canonical(W.randomized_weights(n, seed=11), n), n)
    rng = np.random.default_rng(seed)
    x = (rng.random((b, n // 2, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    return tm, np.concatenate([x, x], axis=1)                # every point twice: exact ties in the max-pool


def _own_pins(c):
    return {"relu": [m.copy() for m in c["mask"]], "pool": c["pool"].copy(), "dec": [c["m1"].copy(), c["m2"].copy()]}


def test_pinning_the_models_own_decisions_is_bit_identical():
    from oracle.train_model import PARAM_GROUPS
    tm, x = _model_and_batch()
    loss, G, c = tm.loss_and_grads(x)
    assert (c["pool"].sum(axis=1) >= 2).all()                # the duplicated points do tie
    pins = _own_pins(c)
    idx = tuple(np.asarray(i) for i in _chamfer_idx(c["recon"], x))
    loss_p, G_p, c_p = tm.loss_and_grads(x, idx=idx, pins=pins)
    assert loss_p == loss
    assert np.array_equal(c_p["recon"], c["recon"])
    for k in PARAM_GROUPS:
        for j in range(len(G[k])):
            assert np.array_equal(G_p[k][j], G[k][j]), (k, j)
    assert all(v == (0, 0.0) for v in tm.pin_disagreements(c_p).values())
    assert tm.chamfer_pin_disagreements(c_p["recon"], x, idx) == (0, 0.0)


def _chamfer_idx(recon, gt):
    from oracle.attack_model import _o
    _, i1, _, i2 = _o().nn_distance(np.asarray(recon, np.float32), np.asarray(gt, np.float32))
    return i1.astype(np.int64), i2.astype(np.int64)


def test_a_flipped_decision_is_reported_with_its_boundary_distance():
    tm, x = _model_and_batch()
    c = tm.forward(x)
    pins = _own_pins(c)
    y2 = c["xhat"][2] * tm.p["gamma"][2] + tm.p["beta"][2]
    r, ch = np.unravel_index(np.argmin(np.abs(y2)), y2.shape)
    pins["relu"][2][r, ch] = ~pins["relu"][2][r, ch]
    cp = tm.forward(x, pins)
    rep = tm.pin_disagreements(cp)
    assert rep["relu2"] == (1, float(abs(y2[r, ch])))
    assert rep["relu0"] == rep["relu1"] == (0, 0.0)          # layers in front of the flip are untouched
    _, G, _ = tm.loss_and_grads(x)
    _, G_p, _ = tm.loss_and_grads(x, pins=pins)
    assert not np.array_equal(G_p["enc_w"][2], G["enc_w"][2])

    # a max-pool winner taken from the runner-up: reported with the gap between the two
    c = tm.forward(x)
    pins = _own_pins(c)
    h5 = c["h5"]
    top = np.sort(h5[0, :, 7])[::-1]
    runner = np.nonzero(h5[0, :, 7] == top[top < top[0]][0])[0]
    pins["pool"][0, :, 7] = False
    pins["pool"][0, runner, 7] = True
    cnt, gap = tm.pin_disagreements(tm.forward(x, pins))["pool"]
    assert cnt == 1 and gap == float(top[0] - top[top < top[0]][0])

    # a Chamfer match moved to another point: reported with the distance it adds
    recon = c["recon"]
    i1, i2 = _chamfer_idx(recon, x)
    j = int((i1[1, 3] + 1) % x.shape[1])
    i1b = i1.copy()
    i1b[1, 3] = j
    cnt, gap = tm.chamfer_pin_disagreements(recon, x, (i1b, i2))
    d = lambda k: float(((recon[1, 3] - x[1, k].astype(np.float64)) ** 2).sum())
    assert cnt == 1 and gap == (d(j) - d(i1[1, 3])) / max(d(i1[1, 3]), 1.0) and gap > 0
