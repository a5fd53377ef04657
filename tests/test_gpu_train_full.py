"""The training step (csrc/train.hip) against the fp64 model (oracle/train_model.py) at the shapes the small parity tests in
test_gpu_train.py cannot reach: the bench's 50 x 2048 (Chamfer through the screened scan, the backward statistics' unrolled
main loop), 130 x 1024 (the forward statistics' main loop, three chunks of the output layer's weight gradient), 2 x 32768
(the largest cloud, a 98 304-wide output layer), 1400 x 64 (a batch whose output-layer staging once needed more LDS than a
CU has), EMD at 8 x 2048, one Adam step at 50 x 2048, and clouds translated by 10 and 100.

At these sizes fp32 and fp64 cannot be made to take the same discrete decisions by redrawing the batch (50 x 2048 has
hundreds of ReLU inputs within 5e-6 of zero), so the oracle runs with the GPU's decisions PINNED: the encoder's ReLU masks
(the sign of fmaf(a, scale, shift), rebuilt on the host from the step's saved a_i and folded BN constants -- a * scale is
exact in double, so the sign is too), the max-pool winners (checked against the GPU's tie counts), the decoder's ReLU masks
and the Chamfer matches.  Each pin must be legitimate: wherever fp64 would decide otherwise, its fp64 value lies within
_pin_margin of the boundary (TrainModel.pin_disagreements).  Tolerances are the small tests': loss 1e-5 relative, recon 1e-5
absolute, gradients 5e-5 of each variable's norm (EMD: 2e-5 / 2e-4, the fast plan's fp32 pair weights)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHAMFER_MARGIN = 1e-6       # squared-distance gap of a pinned Chamfer match to fp64's nearest neighbour (relative above 1)


def _pin_margin(x):
    """Largest legitimate fp64 distance from its boundary of a decision where fp64 and the GPU disagree: 100 fp32 ulps of the
    input relative to its spread.  Layer 0's a = x . W + b is rounded at ulp(|x| |W|) while the batch norm divides by its
    spread, so a translated cloud carries proportionally more rounding into every later decision (measured: 7e-7 at t = 0,
    1.8e-5 at t = 10, 2e-4 at t = 100, ~10x under this margin)."""
    x = np.asarray(x, np.float64)
    return 100 * 2.0 ** -24 * float(np.abs(x).max() / x.reshape(-1, 3).std(axis=0).min())


def _clouds(seed, b, n, shift=0.0):
    rng = np.random.default_rng(seed)
    x = (rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    return (x + np.float32(shift)).astype(np.float32)


def _setup(n, b, seed=11, loss="chamfer"):
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.trainer import PointNetAETrainer
    from oracle.train_model import TrainModel
    w = W.randomized_weights(n, seed=seed)
    return w, PointNetAETrainer(w, n, batch_size=b, loss=loss), TrainModel(W.canonical(w, n), n, loss=loss)


def _pins(st, b, n):
    """The GPU step's discrete decisions, from its saved state."""
    relu = []
    for i in range(5):
        y = st["act"][i].astype(np.float64) * st["scale"][i].astype(np.float64) + st["shift"][i].astype(np.float64)
        relu.append(y > 0)
    h5 = np.maximum(st["act"][4].astype(np.float64) * st["scale"][4].astype(np.float64) + st["shift"][4].astype(np.float64), 0)
    h5 = h5.astype(np.float32).reshape(b, n, 128)
    pool = h5 == st["pool_max"][:, None, :]
    assert np.array_equal(pool.sum(axis=1), st["pool_ties"]), "max-pool winners rebuilt on the host differ from the GPU's"
    return {"relu": relu, "pool": pool, "dec": [st["d1"] > 0, st["d2"] > 0]}


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def _check_pins(tm, c, x, recon_gt=None, idx=None):
    rep = tm.pin_disagreements(c)
    if idx is not None:
        rep["chamfer"] = tm.chamfer_pin_disagreements(c["recon"], recon_gt, idx)
    margin = _pin_margin(x)
    print("pins fp64 disagrees with (count, largest boundary distance):", rep, "margin %.3g" % margin)
    return [(k, cnt, dist) for k, (cnt, dist) in rep.items() if dist > (CHAMFER_MARGIN if k == "chamfer" else margin)]


def _compare(tr, tm, x, gt=None, loss_tol=1e-5, recon_tol=1e-5, grad_tol=5e-5, grad_tol_for=None):
    from oracle.train_model import PARAM_GROUPS
    b, n = tr.batch_size, tr.n_points
    recon, loss = tr.forward_backward(x, gt)
    g_gpu = tr.gradients()
    st = tr.saved_state()
    pins = _pins(st, b, n)
    gt_ = x if gt is None else gt
    idx = (st["idx1"].astype(np.int64), st["idx2"].astype(np.int64)) if tm.loss == "chamfer" else None
    loss_ref, G, c = tm.loss_and_grads(x, gt, idx=idx, pins=pins)
    bad_pins = _check_pins(tm, c, x, gt_, idx)
    errs = {"loss": abs(float(loss.item()) - loss_ref) / abs(loss_ref),
            "recon": float(np.abs(recon.cpu().numpy() - c["recon"]).max())}
    worst, over = ("", 0.0), []
    for k in PARAM_GROUPS:
        for j in range(len(G[k])):
            if k == "enc_b":          # exactly zero behind a batch norm: both sides hold rounding noise only
                assert np.abs(g_gpu[k][j]).max() <= 1e-4 * np.abs(G["enc_w"][j]).max()
                continue
            e, name = _rel(g_gpu[k][j], G[k][j]), "%s[%d]" % (k, j)
            if e > worst[1]:
                worst = (name, e)
            if e > (grad_tol_for or {}).get(name, grad_tol):
                over.append((name, e))
    print("errors: loss %.3g  recon %.3g  worst gradient %s %.3g" % (errs["loss"], errs["recon"], worst[0], worst[1]))
    assert not bad_pins, bad_pins
    assert errs["loss"] <= loss_tol
    assert errs["recon"] <= recon_tol
    assert not over, over
    return st


@pytest.mark.parametrize("b,n", [(50, 2048), (130, 1024), (2, 32768), (1400, 64)])
def test_full_size_step_matches_the_pinned_oracle(b, n):
    """Chamfer at each shape: loss, recon and every variable's gradient."""
    _, tr, tm = _setup(n, b)
    _compare(tr, tm, _clouds(3, b, n))


@pytest.mark.parametrize("shift", [10.0, 100.0])
def test_translated_clouds_match_the_pinned_oracle(shift):
    """Batch norm makes everything after layer 0 invariant to translating the input; layer 0's batch statistics must not
    lose it either (a one-pass E[a^2] - mean^2 over fp32 per-tile sums did: at t = 100 the pinned decisions then sat up to
    1.7e-3 from their boundaries).  Two errors remain that the statistics do not cause: layer 0's weight gradient is the fp32
    sum of x * da over the rows, whose terms cancel to the sum of (x - mean x) * da, and a_0 itself is stored in fp32 at
    |a_0| ~ |x| |W|.  Measured at t = 100: enc_w[0] 2.6e-3 of its norm, recon 3.0e-5 absolute (t = 10: 3.0e-5 and 3.5e-6,
    within the untranslated tolerances); everything else within them at both shifts."""
    b, n = 50, 2048
    _, tr, tm = _setup(n, b)
    loose = shift > 10
    _compare(tr, tm, _clouds(3, b, n, shift), recon_tol=1e-4 if loose else 1e-5,
             grad_tol_for={"enc_w[0]": 5e-3} if loose else None)


def test_full_size_emd_step_matches_the_pinned_oracle():
    """loss 'emd' at 8 x 2048 against the C approx_match / match_cost_grad (ReLU masks and pool winners pinned; the plan
    is continuous in the reconstruction, nothing to pin there)."""
    b, n = 8, 2048
    _, tr, tm = _setup(n, b, loss="emd")
    _compare(tr, tm, _clouds(3, b, n), _clouds(77, b, n), loss_tol=2e-5, grad_tol=2e-4)


def test_full_size_adam_step_and_moving_averages():
    """One partial_fit at the bench shape against TrainModel.step with the GPU's decisions pinned: the weights after Adam
    where the gradient is solid (Adam's first step is lr * g / (|g| + 3e-7), so rounding-level gradients may step either
    way) and both moving averages."""
    from geometric_adv_amd import weights as W
    b, n, lr = 50, 2048, 0.0005
    w, tr, tm = _setup(n, b)
    x = _clouds(5, b, n)
    _, loss = tr.partial_fit(x)
    G = tr.gradients()                                                     # apply leaves the step's gradients in place
    st = tr.saved_state()
    pins = _pins(st, b, n)
    idx = (st["idx1"].astype(np.int64), st["idx2"].astype(np.int64))
    assert not _check_pins(tm, tm.forward(x, pins), x, x, idx)
    loss_ref, _ = tm.step(x, idx=idx, pins=pins)
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref)
    new = W.canonical(tr.export_weights(), n)
    old = W.canonical(w, n)
    for k in ("enc_w", "gamma", "beta", "dec_w", "dec_b"):
        for j in range(len(G[k])):
            solid = np.abs(G[k][j]) > 1e-4 * np.abs(G[k][j]).max()
            diff = np.abs(new[k][j].astype(np.float64) - tm.p[k][j])[solid]
            assert diff.size and diff.max() <= 2e-2 * lr, (k, j, diff.max())
            # every variable whose gradient outweighs Adam's epsilon (|g| > 1e-5 >> 3e-7; at B * n = 102 400 rows many
            # solid gradients do not) really moved by ~lr
            big = np.abs(G[k][j]) > 1e-5
            moved = np.abs(new[k][j].astype(np.float64) - np.asarray(old[k][j], np.float64))[big]
            assert moved.size == 0 or moved.min() > 0.5 * lr
    for i in range(5):
        assert np.allclose(new["mean"][i], tm.p["mean"][i], rtol=1e-5, atol=1e-6)
        assert np.allclose(new["var"][i], tm.p["var"][i], rtol=1e-4, atol=1e-7)


def test_largest_batch_step_runs_and_its_output_layer_gradient_is_right():
    """B = 4096 (the largest batch trainer_create accepts; 64 chunks of the output layer's weight gradient): the step runs,
    everything is finite, and d loss / d V2, d c2 equal the product of the step's own saved decoder activations with the
    Chamfer gradient of its own reconstruction and matches (fp64 on the host)."""
    b, n = 4096, 64
    _, tr, _ = _setup(n, b)
    x = _clouds(8, b, n)
    recon, loss = tr.forward_backward(x)
    G = tr.gradients()
    assert np.isfinite(float(loss.item()))
    assert all(np.isfinite(a).all() for v in G.values() for a in v)
    st = tr.saved_state()
    r = recon.cpu().numpy().astype(np.float64)
    gt = x.astype(np.float64)
    i1, i2 = st["idx1"].astype(np.int64), st["idx2"].astype(np.int64)
    ar = np.arange(b)[:, None]
    g = 2.0 / (b * n) * (r - gt[ar, i1])
    t2 = 2.0 / (b * n) * (gt - r[ar, i2])
    for k in range(b):
        np.subtract.at(g[k], i2[k], t2[k])
    g = g.reshape(b, 3 * n)
    d2 = st["d2"].astype(np.float64)
    assert _rel(G["dec_w"][2], d2.T @ g) <= 5e-5
    assert _rel(G["dec_b"][2], g.sum(0)) <= 5e-5
    d1 = [tr.partial_fit(x, want_recon=False)[1] for _ in range(3)]
    assert np.all(np.isfinite(d1))
