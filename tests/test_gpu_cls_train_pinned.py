"""GPU: the PointNet classifier training step (csrc/cls_train.hip) against the float64 model of tests/_cls_train_model64.py
with every discrete decision of the step PINNED to the GPU's own, at the shapes where the step's code changes path.

test_gpu_cls_train.py compares the step with the model's own decisions, so it can only run on batches where fp32 and fp64
decide alike; among the B * N * 3776 per-point ReLU inputs some lie within 1e-6 of zero in every batch, and each one that
flips moves a gradient by one row's share.  Here the model takes the step's decisions instead:
- the ReLU mask of every batch-norm layer, rebuilt on the host as (a * inv + shift) > 0 in float32 from the step's stored
  pre-BN activation a and folded constants (geoadv_cls_trainer_state PRE_BN, BN_INV, BN_SHIFT).  The library is built
  without contraction, so the device's test is two fp32 roundings that numpy reproduces bit for bit; the rebuild is checked
  bitwise: the first maximum of max(a * inv + shift, 0) over each cloud equals the step's pool_argmax everywhere;
- the three pools' rows (pool_argmax) and the two dropout masks.
Each pin must be legitimate: wherever fp64 would decide otherwise, its fp64 ReLU input (or pooled gap) lies within
_pin_margin of the boundary.

Tolerances (one step), each a few times the worst the MI355X measured:
- batch statistics, every case: each layer's batch mean and variance equal the float64 moments of its own stored pre-BN
  activation within 2^-22 / 2^-20 relative (measured at most 5.9e-8 everywhere, translated clouds included);
- pins: fp64 distance of a disagreeing pin from its boundary <= _pin_margin = PIN_ULPS fp32 ulps of max|x| / min std(x).
  Measured, in those ulps: 754 at 32 x 2048, 943 at + 10, 651 at + 100, 3678 at x 1e-2, 6886 at 4 x 16384 (PIN_ULPS 20000);
- gradients, ||g - g64|| <= tol * ||g64|| per trainable variable.  A gradient that is zero in fp64 must be exactly zero on
  the GPU.  The bn/beta of a pooled layer is compared relative to its bn/gamma gradient (only clouds whose maximum is not
  positive feed it); where every maximum is positive it is analytically zero and checked as rounding noise with the biases
  that feed a batch norm: NOISE_TOL of the layer's bn/gamma gradient (measured at most 2e-4).
  * well-conditioned batches (B >= 7, the one-cloud batch, and the 4 x 256 batch of distinct shapes): GRAD_TOL = 5e-4.
    Measured: 32 x 2048 seeds 2 / 3 4.5e-5 / 3.9e-5, duplicated halves 3.6e-5, clouds x 1e-2 1.5e-4, 300 x 32 7.3e-6,
    1024 x 16 5.5e-6, 7 x 5 1.1e-5, 1 x 512 1.4e-6, 4 x 256 distinct shapes 1.2e-4;
  * few-cloud batches (fc batch norms over 3 to 5 similar clouds, whose per-channel variance lies far below eps): the
    batch's own problem amplifies rounding.  kappa[v] = the largest relative change of v's fp64 gradient over KAPPA_DRAWS
    draws that move every input coordinate by one random fp32 rounding, decisions held (conditioning()); tol =
    max(GRAD_TOL, K_COND * kappa[v]).  kappa reaches 1e-3 at 3 x 1, 5.7e-4 at 4 x 16384, 7.5e-5 ... 2.9e-4 at 4 x 256 and
    8e-5 at 5 x 2048 (0.12 at 2 x 16384, whose two clouds leave too little to judge: that batch is replaced by 4 x 16384,
    the same 128-slice dT path).  Measured error / kappa at most 11.5 (4 x 16384; 9.2 at 4 x 256), K_COND = 35;
  * translated clouds: layer 0's a_0 = x . W + b and conv1's input u = x T1 are stored in fp32 at ulp(|x|), and that
    rounding reaches every later layer, so the gradients of almost every variable move with the shift: measured up to
    3.1e-4 at + 10 (43 variables above 2e-4) and 3.9e-3 at + 100 (56 variables).  Each such variable has its own
    tolerance in TRANSLATED_GRAD_TOL at three times its measured error; the others keep GRAD_TOL;
- loss (relative), logits / T1 / T2 (of their largest magnitude), parameters after Adam / Momentum where |g64| > 10 % of
  the variable's norm (of lr * max(1, ||g64||)) and moving averages (relative): fixed per batch kind in PROFILES.  Measured
  worst: well-conditioned 1.4e-5 / 2.7e-4 / 6e-5 / 9.7e-5 (+ 10 included); few-cloud 3.3e-5 / 6.8e-4 / 4.1e-4 / 2.5e-4;
  + 100 2.6e-4 / 1.8e-3 / 6e-5 / 9.1e-4.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cls_train_model64 as M  # noqa: E402
from geometric_adv_amd import cls_weights as CW  # noqa: E402

pytestmark = pytest.mark.gpu

PIN_ULPS = 20000
GRAD_TOL = 5e-4
K_COND = 35
KAPPA_DRAWS = 3
NOISE_TOL = 1e-3
# loss (relative), logits / T1 / T2 (of their largest magnitude), parameters after the update (of lr * max(1, ||g64||)) and
# moving averages (relative), fixed per batch kind
PROFILES = {
    "well": dict(loss=5e-5, out=1e-3, param=2.5e-4, moving=4e-4),
    "few": dict(loss=1e-4, out=2.5e-3, param=1.5e-3, moving=1e-3),
    "t100": dict(loss=1e-3, out=6e-3, param=2.5e-4, moving=3e-3),
}
# translated clouds: the variables whose measured gradient error exceeded 2e-4, each at three times its measured value
TRANSLATED_GRAD_TOL = {
    10.0: {
        "conv1/bn/beta": 6.3e-4, "conv1/bn/gamma": 8.8e-4, "conv2/bn/beta": 6.1e-4, "conv2/bn/gamma": 9.4e-4,
        "conv2/weights": 8.8e-4, "conv3/weights": 6.4e-4, "conv4/bn/gamma": 8.0e-4, "conv4/weights": 6.9e-4,
        "conv5/bn/gamma": 8.8e-4, "conv5/weights": 8.0e-4, "fc1/bn/gamma": 8.1e-4, "fc1/weights": 8.3e-4,
        "fc2/bn/gamma": 8.5e-4, "fc2/weights": 8.7e-4, "fc3/weights": 8.3e-4, "transform_net1/tconv1/bn/beta": 7.8e-4,
        "transform_net1/tconv1/bn/gamma": 6.1e-4, "transform_net1/tconv1/weights": 7.5e-4,
        "transform_net1/tconv2/bn/beta": 6.8e-4, "transform_net1/tconv2/weights": 6.1e-4,
        "transform_net1/tconv3/bn/gamma": 6.3e-4, "transform_net1/tconv3/weights": 6.1e-4,
        "transform_net1/tfc1/bn/beta": 6.6e-4, "transform_net1/tfc1/bn/gamma": 6.7e-4,
        "transform_net1/tfc1/weights": 6.2e-4, "transform_net1/tfc2/bn/beta": 7.3e-4,
        "transform_net1/tfc2/bn/gamma": 6.7e-4, "transform_net1/tfc2/weights": 6.5e-4,
        "transform_net1/transform_XYZ/weights": 6.7e-4, "transform_net2/tconv1/bn/beta": 7.1e-4,
        "transform_net2/tconv1/bn/gamma": 8.7e-4, "transform_net2/tconv1/weights": 8.1e-4,
        "transform_net2/tconv2/bn/beta": 6.9e-4, "transform_net2/tconv2/bn/gamma": 7.4e-4,
        "transform_net2/tconv2/weights": 7.7e-4, "transform_net2/tconv3/bn/gamma": 8.1e-4,
        "transform_net2/tconv3/weights": 8.3e-4, "transform_net2/tfc1/bn/gamma": 7.8e-4,
        "transform_net2/tfc1/weights": 8.3e-4, "transform_net2/tfc2/bn/gamma": 8.5e-4,
        "transform_net2/tfc2/weights": 8.7e-4, "transform_net2/transform_feat/biases": 6.4e-4,
        "transform_net2/transform_feat/weights": 8.4e-4,
    },
    100.0: {
        "conv1/bn/beta": 6.6e-3, "conv1/bn/gamma": 9.5e-3, "conv1/weights": 9.8e-3, "conv2/bn/beta": 7.3e-3,
        "conv2/bn/gamma": 7.7e-3, "conv2/weights": 7.5e-3, "conv3/bn/beta": 5.8e-3, "conv3/bn/gamma": 6.8e-3,
        "conv3/weights": 6.8e-3, "conv4/bn/beta": 5.2e-3, "conv4/bn/gamma": 8.1e-3, "conv4/weights": 7.8e-3,
        "conv5/bn/beta": 4.5e-3, "conv5/bn/gamma": 9.3e-3, "conv5/weights": 8.2e-3, "fc1/bn/beta": 4.6e-3,
        "fc1/bn/gamma": 9.9e-3, "fc1/weights": 9.1e-3, "fc2/bn/beta": 3.5e-3, "fc2/bn/gamma": 1.0e-2,
        "fc2/weights": 9.8e-3, "fc3/biases": 2.6e-3, "fc3/weights": 9.6e-3, "transform_net1/tconv1/bn/beta": 6.7e-3,
        "transform_net1/tconv1/bn/gamma": 5.7e-3, "transform_net1/tconv1/weights": 9.5e-3,
        "transform_net1/tconv2/bn/beta": 6.7e-3, "transform_net1/tconv2/bn/gamma": 6.5e-3,
        "transform_net1/tconv2/weights": 7.1e-3, "transform_net1/tconv3/bn/gamma": 6.4e-3,
        "transform_net1/tconv3/weights": 6.2e-3, "transform_net1/tfc1/bn/beta": 6.7e-3,
        "transform_net1/tfc1/bn/gamma": 6.6e-3, "transform_net1/tfc1/weights": 6.4e-3,
        "transform_net1/tfc2/bn/beta": 6.3e-3, "transform_net1/tfc2/bn/gamma": 6.4e-3,
        "transform_net1/tfc2/weights": 6.4e-3, "transform_net1/transform_XYZ/biases": 1.2e-2,
        "transform_net1/transform_XYZ/weights": 6.6e-3, "transform_net2/tconv1/bn/beta": 7.8e-3,
        "transform_net2/tconv1/bn/gamma": 9.9e-3, "transform_net2/tconv1/weights": 8.4e-3,
        "transform_net2/tconv2/bn/beta": 8.6e-3, "transform_net2/tconv2/bn/gamma": 1.1e-2,
        "transform_net2/tconv2/weights": 9.0e-3, "transform_net2/tconv3/bn/beta": 6.0e-3,
        "transform_net2/tconv3/bn/gamma": 9.9e-3, "transform_net2/tconv3/weights": 9.3e-3,
        "transform_net2/tfc1/bn/beta": 7.2e-3, "transform_net2/tfc1/bn/gamma": 1.1e-2,
        "transform_net2/tfc1/weights": 9.5e-3, "transform_net2/tfc2/bn/beta": 6.9e-3,
        "transform_net2/tfc2/bn/gamma": 1.1e-2, "transform_net2/tfc2/weights": 1.1e-2,
        "transform_net2/transform_feat/biases": 6.8e-3, "transform_net2/transform_feat/weights": 1.0e-2,
    },
}

BN = [(l, s) for l, (s, _, _, bn, _) in enumerate(CW.LAYERS) if bn]
POOLED = ["transform_net1/tconv3", "transform_net2/tconv3", "conv5"]
LIDX = {s: l for l, s in BN}
# Gradients that are zero in exact arithmetic: the biases that feed a batch norm, and the bn/beta of a pooled layer while
# every (cloud, channel) maximum is positive (its shift then reaches the next fc batch norm as a per-column constant).
FED_BIASES = set(s + "/biases" for _, s in BN)
POOLED_BETAS = set(s + "/bn/beta" for s in POOLED)


def analytic_zero(ref_grads):
    """The variables whose fp64 gradient is zero up to rounding (at most 1e-8 of the layer's bn/gamma gradient, where they
    are not analytically zero it is of order one)."""
    out = set(FED_BIASES)
    for k in POOLED_BETAS:
        gamma = np.linalg.norm(ref_grads[k.replace("/beta", "/gamma")])
        if np.linalg.norm(ref_grads[k]) <= 1e-8 * gamma:
            out.add(k)
    return out


def _per_point(scope):
    return "conv" in scope.rsplit("/", 1)[-1]


def _trainer(w, B, N, nc, **kw):
    from geometric_adv_amd.cls_trainer import PointNetClassifierTrainer
    return PointNetClassifierTrainer(weights=w, num_points=N, batch_size=B, num_classes=nc, **kw)


def _case(B, N, nc, seed, shift=0.0, scale=1.0, dup=False):
    """synthetic_weights(nc, seed) and a uniform batch, as test_gpu_cls_train.py draws them; dup: each cloud's second half
    repeats its first (every maximum attained twice)."""
    rng = np.random.default_rng(seed)
    w = CW.synthetic_weights(nc, seed)
    x = (rng.random((B, N, 3)) - 0.5).astype(np.float32)
    y = rng.integers(0, nc, B)
    if dup:
        x[:, N // 2:] = x[:, :N // 2]
    return w, (x * np.float32(scale) + np.float32(shift)).astype(np.float32), y


def _grad_tol(ref, k, grad_tol_for=None):
    """Gradient tolerance of variable k.  Few-cloud batches (ref carries kappa): GRAD_TOL, or K_COND times the variable's
    own conditioning where that is larger.  Every other batch: GRAD_TOL, or a named, measured value from grad_tol_for."""
    if "kappa" in ref:
        return max(GRAD_TOL, K_COND * ref["kappa"][k])
    return (grad_tol_for or {}).get(k, GRAD_TOL)


def _pin_margin(x):
    """Largest legitimate fp64 distance from its boundary of a decision where fp64 and the GPU disagree: PIN_ULPS fp32 ulps
    of the input relative to its spread (layer 0's a = x . W + b is rounded at ulp(|x| |W|) while the batch norm divides by
    the spread, so a translated cloud carries proportionally more rounding into every later decision)."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    return PIN_ULPS * 2.0 ** -24 * float(np.abs(x).max() / max(x.std(axis=0).min(), 1e-30))


def _pre(tr, l, rows=None):
    """float32 a * inv + shift of BN layer l (two fp32 roundings, as the device computes it), rows = a slice or None."""
    a = tr.state("pre_bn", l, device=True)
    a = (a if rows is None else a[rows]).cpu().numpy()
    return a * tr.state("bn_inv", l) + tr.state("bn_shift", l)


def _stats_error(tr, l, a):
    """Worst relative error of the step's batch mean / variance of BN layer l against the float64 moments of its own stored
    pre-BN activation a (the device adds the fp32 values in double and rounds once)."""
    a64 = a.astype(np.float64)
    m64 = a64.mean(0)
    v64 = ((a64 - m64) ** 2).mean(0)
    mg, vg = tr.state("bn_mean", l).astype(np.float64), tr.state("bn_var", l).astype(np.float64)
    return float((np.abs(mg - m64) / (np.abs(m64) + np.sqrt(v64))).max()), float((np.abs(vg - v64) / (v64 + 1e-30)).max())


def gpu_decisions(tr, B, N):
    """The step's discrete decisions: ({"relu": {scope: mask}, "dropout": [m0, m1]}, pool rows, worst batch-statistics
    errors), with the bitwise check of the rebuilt masks against the step's pool rows."""
    relu, arg, stats = {}, [], [0.0, 0.0]
    for l, s in BN:
        a = tr.state("pre_bn", l)
        pre = a * tr.state("bn_inv", l) + tr.state("bn_shift", l)
        relu[s] = pre > 0
        em, ev = _stats_error(tr, l, a)
        stats = [max(stats[0], em), max(stats[1], ev)]
        if s in POOLED:
            i = POOLED.index(s)
            got = tr.state("pool_argmax", i)
            first = np.argmax(np.maximum(pre, np.float32(0)).reshape(B, N, -1), axis=1)
            assert np.array_equal(first, got), (s, int(np.sum(first != got)))
            arg.append(got.astype(np.int64))
    return {"relu": relu, "dropout": [tr.state("dropout_mask", i).astype(np.float64) for i in range(2)]}, arg, stats


def run_pinned(w, x, y, nc, seed=0, optimizer="adam", step_k=0, kappa=False):
    """One step of a handle, then the model with all of that step's decisions pinned: (gpu dict, model dict, pins, rows).
    kappa: also measure the batch's conditioning (few-cloud batches)."""
    B, N = x.shape[:2]
    tr = _trainer(w, B, N, nc, optimizer=optimizer, seed=seed, step=step_k)
    loss, _ = tr.train_step(x, y)
    pins, arg, stats = gpu_decisions(tr, B, N)
    if B <= 64:      # the generator is restated in Python; at large B this costs seconds per layer
        for i, C in ((0, 512), (1, 256)):
            assert np.array_equal(pins["dropout"][i], M.keep_mask(seed, step_k, i, B, C)), i
    got = {"loss": loss, "grads": tr.gradients(), "new": tr.export_weights(slots=False), "stats": stats,
           "logits": tr.state("logits"), "t1": tr.state("t1"), "t2": tr.state("t2")}
    del tr
    ref = M.step(w, x.astype(np.float64), y, nc, step_k=step_k, seed=seed, optimizer=optimizer, pins=pins, force_argmax=arg)
    if kappa:
        ref["kappa"] = conditioning(w, x, y, nc, seed, optimizer, step_k, pins, arg, ref)
    return got, ref, pins, arg


_SHARED = {}


def shared_reference_case():
    """32 x 2048, seed 2: one step and its pinned model, computed once for the parity and the perturbation tests."""
    if "ref" not in _SHARED:
        w, x, y = _case(32, 2048, 13, 2)
        _SHARED["ref"] = (w, x, y) + run_pinned(w, x, y, 13, seed=2)
    return _SHARED["ref"]


def conditioning(w, x, y, nc, seed, optimizer, step_k, pins, arg, ref):
    """{variable: largest relative change of its fp64 gradient over KAPPA_DRAWS draws in which every input coordinate moves
    by one random fp32 rounding (relative 2^-24 N(0, 1)), all decisions held}: how much the step's own problem amplifies
    rounding.  The fc batch norms over a few clouds whose pooled features barely differ (per-channel variance far below eps)
    amplify it by 10^3 and more."""
    rng = np.random.default_rng(0)
    out = {}
    for _ in range(KAPPA_DRAWS):
        xp = x.astype(np.float64) * (1 + 2.0 ** -24 * rng.standard_normal(x.shape))
        moved = M.step(w, xp, y, nc, step_k=step_k, seed=seed, optimizer=optimizer, pins=pins, force_argmax=arg)
        for k, v in grad_errors(moved["grads"], ref["grads"]).items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def grad_errors(grads, ref_grads):
    """{variable: relative error} over the variables whose gradient is not analytically zero; a variable whose fp64 gradient
    is exactly zero reports inf unless the GPU's is exactly zero too."""
    out, zero = {}, analytic_zero(ref_grads)
    for k, g64 in ref_grads.items():
        if k in zero:
            continue
        gg = np.asarray(grads[k], np.float64).reshape(g64.shape)
        if k in POOLED_BETAS:     # only clouds whose maximum is not positive contribute: a residual of gamma's size
            scale = np.linalg.norm(ref_grads[k.replace("/beta", "/gamma")])
            out[k] = float(np.linalg.norm(gg - g64) / scale) if scale else (0.0 if not np.any(gg - g64) else float("inf"))
        elif not np.any(g64):
            out[k] = 0.0 if not np.any(gg) else float("inf")
        else:
            out[k] = _rel(gg, g64)
    return out


def errors(got, ref, x, grad_tol_for=None):
    rep = M.pin_disagreements(ref)
    margin = _pin_margin(x)
    err = {"pins": {k: v for k, v in rep.items() if v[0]}, "margin": margin, "stats": got["stats"],
           "bad_pins": {k: v for k, v in rep.items() if v[1] > margin},
           "loss": abs(got["loss"] - ref["loss"]) / abs(ref["loss"]) if ref["loss"] else abs(got["loss"])}
    for k in ("logits", "t1", "t2"):
        err[k] = float(np.abs(got[k].reshape(ref[k].shape) - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-300))
    err["grad"] = grad_errors(got["grads"], ref["grads"])
    err["over_tol"] = {k: v / _grad_tol(ref, k, grad_tol_for) for k, v in err["grad"].items()}
    err["kappa"] = ref.get("kappa")
    err["noise"] = {}
    zero = analytic_zero(ref["grads"])
    for k in zero:
        gamma = ref["grads"][k.rsplit("/", 1)[0].replace("/bn", "") + "/bn/gamma"]
        gg = got["grads"][k]
        err["noise"][k] = float(np.linalg.norm(gg) / np.linalg.norm(gamma)) if np.any(gamma) else \
            (0.0 if not np.any(gg) else float("inf"))
    err["param"] = {}
    for k, g64 in ref["grads"].items():
        if k in zero or not np.any(g64):
            continue
        sel = (np.abs(g64) > 0.1 * np.linalg.norm(g64)).reshape(-1)
        if sel.any():
            d = np.abs(np.asarray(got["new"][k], np.float64).reshape(-1)[sel] - ref["new_weights"][k].reshape(-1)[sel])
            err["param"][k] = float(d.max() / (ref["lr"] * max(1.0, float(np.linalg.norm(g64)))))
    err["moving"] = 0.0
    for _, s in BN:
        n = CW.bn_names(s)
        for f in ("mean", "var"):
            r = ref["new_weights"][n[f]]
            err["moving"] = max(err["moving"], float(np.abs(got["new"][n[f]] - r).max() / max(np.abs(r).max(), 1e-300)))
    return err


def report(name, err):
    worst = max(err["grad"].items(), key=lambda kv: kv[1])
    unit = err["margin"] / PIN_ULPS
    far = max([d for _, d in err["pins"].values()] or [0.0])
    print("\n%s: pins disagreeing %s (farthest %.3g = %.0f margin ulps) | stats %.2g / %.2g | loss %.3g logits %.3g "
          "t1 %.3g t2 %.3g | worst gradient %s %.3g | noise %.3g | param %.3g | moving %.3g" % (
              name, {k: (c, "%.2g" % d) for k, (c, d) in err["pins"].items()}, far, far / unit, err["stats"][0],
              err["stats"][1], err["loss"], err["logits"], err["t1"], err["t2"], worst[0], worst[1],
              max(err["noise"].values()), max(err["param"].values() or [0.0]), err["moving"]))
    top = sorted(err["grad"].items(), key=lambda kv: -kv[1])
    print("  gradient errors above GRAD_TOL:", ", ".join("%s %.3g" % kv for kv in top if kv[1] > GRAD_TOL) or "none")
    top = sorted(err["over_tol"].items(), key=lambda kv: -kv[1])[:3]
    print("  largest error / tolerance:", ", ".join("%s %.3g" % kv for kv in top))
    if err["kappa"]:
        ratio = sorted(((k, err["grad"][k] / err["kappa"][k]) for k in err["grad"] if err["kappa"][k] > 0),
                       key=lambda kv: -kv[1])[:3]
        print("  worst conditioning %.3g; largest error / kappa: %s" % (
            max(err["kappa"].values()), ", ".join("%s %.3g" % kv for kv in ratio)))


def check(err, profile="well"):
    t = PROFILES[profile]
    assert not err["bad_pins"], (err["bad_pins"], err["margin"])
    assert err["stats"][0] <= 2.0 ** -22 and err["stats"][1] <= 2.0 ** -20, err["stats"]
    assert err["loss"] <= t["loss"], err["loss"]
    for k in ("logits", "t1", "t2"):
        assert err[k] <= t["out"], (k, err[k])
    over = {k: (err["grad"][k], v) for k, v in err["over_tol"].items() if v > 1}
    assert not over, over
    noisy = {k: v for k, v in err["noise"].items() if v > NOISE_TOL}
    assert not noisy, noisy
    off = {k: v for k, v in err["param"].items() if v > t["param"]}
    assert not off, off
    assert err["moving"] <= t["moving"], err["moving"]


# ---- §3: pinned parity at the shapes where the step changes path -------------------------------------------------------

@pytest.mark.parametrize("optimizer", ["adam", "momentum"])
@pytest.mark.parametrize("seed", [46, 41, 59, 65])
def test_screened_seeds_meet_one_tolerance_pinned(seed, optimizer):
    """The small test's batches (4 x 256, 13 classes): unpinned their gradient errors spread from 4.4e-4 to 9.9e-3 with the
    seed; pinned, every seed meets one rule.  Their fc batch norms run over four similar clouds: few-cloud profile."""
    w, x, y = _case(4, 256, 13, seed)
    got, ref, _, _ = run_pinned(w, x, y, 13, seed=seed, optimizer=optimizer, kappa=True)
    err = errors(got, ref, x)
    report("4x256 seed %d %s" % (seed, optimizer), err)
    check(err, "few")


def test_reference_size_matches_the_pinned_model():
    """32 x 2048, seed 2 (its reference is shared with the perturbation test)."""
    w, x, y, got, ref, _, _ = shared_reference_case()
    err = errors(got, ref, x)
    report("32x2048 nc 13 seed 2 (reference size)", err)
    check(err)


SHAPES = [
    # (B, N, classes, seed, profile, why)
    (32, 2048, 13, 3, "well", "reference size"),
    (1, 512, 13, 1, "well", "fc batch norm over one cloud: variance 0, output relu(beta)"),
    (7, 5, 40, 1, "well", "N < 64, not a multiple of 4; ModelNet40's classes"),
    (3, 1, 13, 1, "few", "one point per cloud"),
    (300, 32, 13, 1, "well", "B > 256: two statistics chunks, split-K fc weight gradients"),
    (1024, 16, 13, 1, "well", "largest batch"),
    (4, 16384, 13, 1, "few", "largest cloud: per-cloud dT split 128 ways"),
    (5, 2048, 65, 1, "few", "fc3 across two 64-wide tiles"),
]


@pytest.mark.parametrize("B,N,nc,seed,profile,why", SHAPES, ids=["%dx%d-%d-s%d" % s[:4] for s in SHAPES])
def test_step_matches_the_pinned_model(B, N, nc, seed, profile, why):
    w, x, y = _case(B, N, nc, seed)
    got, ref, _, _ = run_pinned(w, x, y, nc, seed=seed, kappa=profile == "few")
    err = errors(got, ref, x)
    report("%dx%d nc %d seed %d (%s)" % (B, N, nc, seed, why), err)
    check(err, profile)


def test_one_class_has_exactly_zero_classifier_gradients():
    """One class: cross entropy is 0 and dlogits exactly 0, so fc3 ... fc1 and conv5 ... conv3 get exactly zero gradients;
    T-Net 2, conv2, conv1 and T-Net 1 get the regulariser's alone and must match the model."""
    w, x, y = _case(4, 256, 1, 1)
    assert not y.any()
    got, ref, _, _ = run_pinned(w, x, y, 1, seed=1, kappa=True)
    g = got["grads"]
    for s in ("fc3", "fc2", "fc1", "conv5", "conv4", "conv3"):
        for k in [n for n in g if n.startswith(s + "/")]:
            assert not np.any(g[k]), k
            assert not np.any(ref["grads"][k]), k
    err = errors(got, ref, x)
    report("4x256 one class", err)
    moved = [k for k, v in ref["grads"].items() if np.any(v) and k not in analytic_zero(ref["grads"])]
    assert any(k.startswith("transform_net1/") for k in moved) and "conv1/weights" in moved
    check(err, "few")


@pytest.mark.parametrize("shift", [10.0, 100.0])
def test_translated_clouds_match_the_pinned_model(shift):
    """Batch norm makes everything after layer 0 invariant to translating the input.  What remains of it in fp32: a_0 =
    x . W + b (T-Net 1's tconv1) and u = x T1 (conv1's input) are rounded at ulp(|x|), and those layers' weight gradients
    are fp32 sums of x * da whose terms cancel to the sum of (x - mean x) * da; the first two reach every later layer, so
    the variables named in TRANSLATED_GRAD_TOL get their measured tolerance.  The batch statistics themselves stay exact
    at every shift (the AE step once lost layer 0's variance here): every layer's mean and variance equal the float64
    moments of its stored pre-BN activation within a few fp32 roundings, as in every other case."""
    w, x, y = _case(32, 2048, 13, 2, shift=shift)
    got, ref, _, _ = run_pinned(w, x, y, 13, seed=2)
    err = errors(got, ref, x, TRANSLATED_GRAD_TOL[shift])
    report("32x2048 clouds + %g" % shift, err)
    check(err, "t100" if shift == 100.0 else "well")


def test_clouds_below_the_batch_norm_epsilon_match_the_pinned_model():
    """Clouds scaled by 1e-2: layer 0's variance (~1e-4) lies below eps = 1e-3, which then dominates its batch norm."""
    w, x, y = _case(32, 2048, 13, 2, scale=1e-2)
    got, ref, _, _ = run_pinned(w, x, y, 13, seed=2)
    assert float(ref["var"]["transform_net1/tconv1"].max()) < 1e-3
    err = errors(got, ref, x)
    report("32x2048 clouds x 1e-2", err)
    check(err)


# ---- §5: the tolerance has teeth -----------------------------------------------------------------------------------------

PERTURBATIONS = [
    ("regulariser at half weight", dict(reg_weight=0.0005)),
    ("dropout backward without 1 / 0.7", dict(perturb={"dropout_grad_unscaled": True})),
    ("conv4 batch-norm backward without xhat * m2", dict(perturb={"bn_no_m2": "conv4"})),
    ("fc batch-norm variance over B - 1", dict(perturb={"fc_var_unbiased": True})),
    ("T1 applied transposed", dict(perturb={"t1_transposed": True})),
]


def _family_case(B, N, nc, seed):
    """B clouds of distinct shapes (sphere, square, segment; random scale and offset), so that the fc batch norms see
    clouds that differ: a small batch as well conditioned as a large one."""
    rng = np.random.default_rng(seed)
    xs = []
    for i in range(B):
        c = i % 3
        if c == 0:
            p = rng.standard_normal((N, 3))
            p /= np.linalg.norm(p, axis=1, keepdims=True)
        elif c == 1:
            p = np.c_[rng.uniform(-1, 1, (N, 2)), np.zeros(N)]
        else:
            p = np.c_[rng.uniform(-1, 1, N), np.zeros((N, 2))]
        xs.append(rng.uniform(0.2, 0.5) * p + rng.uniform(-0.1, 0.1, 3))
    return CW.synthetic_weights(nc, seed), np.asarray(xs, np.float32), rng.integers(0, nc, B)


def _moved(got, ref, w, x, y, nc, pins, arg, seed, **kw):
    """Worst gradient error of the GPU step against the model restated with kw (same pins), in units of the tolerance."""
    bad = M.step(w, x.astype(np.float64), y, nc, seed=seed, pins=pins, force_argmax=arg, **kw)
    return max(v / _grad_tol(ref, k) for k, v in grad_errors(got["grads"], bad["grads"]).items())


@pytest.mark.parametrize("B,N", [(4, 256), (32, 2048)])
def test_perturbed_models_fail_the_tolerance(B, N):
    """Each restatement of the step that is wrong somewhere fails its tolerance against the unchanged GPU step, pinned alike.
    At 4 x 256 the clouds are of distinct shapes: on four similar clouds the fc batch norms amplify rounding about as much
    as a halved regulariser moves the gradients, and no tolerance could tell the two apart."""
    if B == 4:
        seed = 46
        w, x, y = _family_case(B, N, 13, seed)
        got, ref, pins, arg = run_pinned(w, x, y, 13, seed=seed)
        err = errors(got, ref, x)
        report("4x256 distinct shapes", err)
        check(err)
    else:
        seed = 2
        w, x, y, got, ref, pins, arg = shared_reference_case()
    moved = {name: _moved(got, ref, w, x, y, 13, pins, arg, seed, **kw) for name, kw in PERTURBATIONS}
    _SHARED.clear()
    print("\n%dx%d: worst gradient error / tolerance against each perturbed model:" % (B, N),
          ", ".join("%s %.3g" % kv for kv in moved.items()))
    weak = {k: v for k, v in moved.items() if not v > 1}
    assert not weak, weak


@pytest.mark.parametrize("B,N", [(4, 256), (32, 2048)])
def test_pool_gradient_goes_to_the_first_maximum_pinned(B, N):
    """Clouds whose second half repeats the first: every maximum is attained twice.  The step's rows are the first maxima
    (gpu_decisions checks them bitwise against the host's first maximum), the pinned comparison meets its tolerance, and
    crediting both copies of each maximum fails it by orders of magnitude.  Sending the gradient to the LAST maximum instead
    leaves every variable's gradient unchanged here -- the two copies are identical through every layer and the weight
    gradients sum over rows -- so that rule is held by the row check alone: the last maxima differ from the step's rows
    wherever a maximum is positive."""
    w, x, y = _case(B, N, 4, 4, dup=True)
    tr = _trainer(w, B, N, 4, seed=4)
    tr.train_step(x, y)
    for i, s in enumerate(POOLED):
        relu = np.maximum(_pre(tr, LIDX[s]), np.float32(0)).reshape(B, N, -1)
        rows = N - 1 - np.argmax(relu[:, ::-1, :], axis=1)
        pos = relu.max(axis=1) > 0
        got = tr.state("pool_argmax", i)
        assert (got < N // 2).all()
        assert (rows[pos] != got[pos]).all() and pos.any()
    del tr
    few = B < 32
    got, ref, pins, arg = run_pinned(w, x, y, 4, seed=4, kappa=few)
    err = errors(got, ref, x)
    report("%dx%d duplicated halves" % (B, N), err)
    check(err, "few" if few else "well")
    both = M.step(w, x.astype(np.float64), y, 4, seed=4, pins=pins, force_argmax=arg,
                  perturb={"pool_also": [a + N // 2 for a in arg]})
    moved = max(v / _grad_tol(ref, k) for k, v in grad_errors(got["grads"], both["grads"]).items())
    print("  crediting both copies: worst gradient error / tolerance %.3g" % moved)
    assert moved > 100, moved


# ---- §4: the largest row count, without the model --------------------------------------------------------------------------

def test_largest_row_count_statistics_pool_rows_and_output_layer():
    """512 x 2048 = 2^20 rows (the most cls_trainer_create accepts; 4096 statistics chunks per per-point layer, B > 256):
    the loss and every gradient are finite; every layer's batch statistics are the float64 moments of its stored pre-BN
    activation; the pool rows are the host's first maxima; fc3's gradients are h_F2^T dlogits and sum dlogits in float64,
    with h_F2 and dlogits rebuilt from the step's own state."""
    import torch
    B, N, nc = 512, 2048, 13
    w, x, y = _case(B, N, nc, 7)
    tr = _trainer(w, B, N, nc, seed=7)
    loss, _ = tr.train_step(x, y)
    assert np.isfinite(loss)
    g = tr.gradients()
    assert all(np.isfinite(v).all() for v in g.values())
    slab = 32        # clouds per slice of a per-point layer: 65536 rows
    worst_m = worst_v = 0.0
    for l, s in BN:
        rows = B * N if _per_point(s) else B
        C = CW.LAYERS[l][2]
        a_dev = tr.state("pre_bn", l, device=True)
        assert tuple(a_dev.shape) == (rows, C)
        k0 = a_dev[0].cpu().numpy().astype(np.float64)        # shift: sums of (a - a[0]) keep the variance
        s1, s2 = np.zeros(C), np.zeros(C)
        step = slab * N if _per_point(s) else rows
        for r0 in range(0, rows, step):
            d = a_dev[r0:r0 + step].cpu().numpy().astype(np.float64) - k0
            s1 += d.sum(0)
            s2 += (d * d).sum(0)
        m64 = k0 + s1 / rows
        v64 = s2 / rows - (s1 / rows) ** 2
        mg, vg = tr.state("bn_mean", l).astype(np.float64), tr.state("bn_var", l).astype(np.float64)
        em = np.abs(mg - m64) / (np.abs(m64) + np.sqrt(v64))
        ev = np.abs(vg - v64) / (v64 + 1e-30)
        worst_m, worst_v = max(worst_m, float(em.max())), max(worst_v, float(ev.max()))
        assert em.max() <= 2.0 ** -22 and ev.max() <= 2.0 ** -20, (s, float(em.max()), float(ev.max()))
        if s in POOLED:
            got = tr.state("pool_argmax", POOLED.index(s))
            for b0 in range(0, B, slab):
                pre = _pre(tr, l, slice(b0 * N, (b0 + slab) * N))
                first = np.argmax(np.maximum(pre, np.float32(0)).reshape(slab, N, C), axis=1)
                assert np.array_equal(first, got[b0:b0 + slab]), (s, b0)
        del a_dev
    l2 = LIDX["fc2"]
    h = np.maximum(_pre(tr, l2), np.float32(0)) / np.float32(M.KEEP) * tr.state("dropout_mask", 1)
    z = tr.state("logits").astype(np.float64)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    p[np.arange(B), y] -= 1.0
    dl = p / B
    ew = _rel(g["fc3/weights"].reshape(256, nc), h.astype(np.float64).T @ dl)
    eb = _rel(g["fc3/biases"], dl.sum(0))
    print("\n512x2048: statistics worst mean %.3g var %.3g (relative); fc3 weights %.3g biases %.3g" % (worst_m, worst_v, ew, eb))
    assert ew <= 1e-5 and eb <= 1e-5, (ew, eb)
    del tr
    torch.cuda.synchronize()
