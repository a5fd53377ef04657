"""CPU: where the bounds of tests/test_gpu_attack_forms.py above 8192 points come from.  The project's tolerances were established up
to 8192 points; that file keeps them for its larger cases (G, H: 10001 ... 16385 points) because the project's own float32 numpy model --
AEModel(..., np.float32) under AttackModel -- meets them against float64 on those cases' inputs.  This test runs that comparison (first
forward, gradient with the matches pinned to the float64 model's, loss rows) and asserts it; the figures it prints (-s) are the ones
quoted there as F32_MODEL.  No GPU is involved."""
import numpy as np
import pytest

import test_gpu_attack_forms as T

LARGE = [(name, variant) for name, variant in T.RUNS if T.CASES[name]["n"] > 8192]
_CACHE = {}


def _models(n):
    from geometric_adv_amd import weights as W
    from oracle.attack_model import AEModel
    if _CACHE.get("n") != n:
        _CACHE.clear()
        canon = W.canonical(W.randomized_weights(n), n)
        _CACHE.update(n=n, m64=AEModel(canon, n, np.float64), m32=AEModel(canon, n, np.float32), idx={})
    return _CACHE["m64"], _CACHE["m32"], _CACHE["idx"]


def test_the_quoted_table_names_every_large_case():
    assert sorted(T.F32_MODEL) == sorted("%s-%s" % r for r in LARGE)
    for key, row in T.F32_MODEL.items():
        for what, err in row.items():
            assert np.isfinite(err) and err <= T.TOL[what], (key, what)


@pytest.mark.parametrize("name,variant", LARGE, ids=["%s-%s" % r for r in LARGE])
def test_float32_model_meets_the_tolerances_above_8192_points(name, variant):
    from oracle.attack_model import AttackModel
    case = T.CASES[name]
    b, n = case["b"], case["n"]
    m64, m32, idx = _models(n)
    x, gt, p0 = T._inputs(case, T._steer_points(case, case["H"]))
    adv_type, dist_type, kw = T.VARIANTS[variant]
    tz = m32.encode(gt).astype(np.float32)
    dw = np.resize(np.array([1.0, 150.0, 0.3], np.float32), b)
    am64, am32 = [AttackModel(m, x, gt, tz.astype(m.dt), dw.astype(m.dt), adv_type, dist_type, lr=T.LR, **kw) for m in (m64, m32)]
    for am in (am64, am32):
        am.init_pert(p0)
    if name not in idx:                                       # the matches do not depend on the loss configuration
        idx[name] = am64.forward()["idx"]
    f64, f32 = am64.forward(idx_override=idx[name]), am32.forward(idx_override=idx[name])
    g64, g32 = am64.gradient(f64), am32.gradient(f32)
    scale = np.abs(g64).reshape(b, -1).max(1)[:, None, None]
    err = dict(adv=np.abs(f32["adv"] - f64["adv"]).max(), latent=np.abs(f32["z"] - f64["z"]).max(),
               recon=np.abs(f32["recon"] - f64["recon"]).max(), grad=np.abs(g32 / scale - g64 / scale).max())
    fourth = "loss_max" if dist_type == "pert" else "max_dist"
    rows = [np.abs(f32[k].astype(np.float64) - f64[k]).max() / np.abs(f64[k]).max()
            for k in ("loss_adv", "loss_dist", "loss_pert", fourth, "input_dist", "loss_ae")]
    if adv_type == "latent":
        err["latent_loss"] = rows.pop(0)
    err["rows"] = max(rows)
    print("\n%-10s %-4s " % (name, variant) + "  ".join("%s %.2e" % kv for kv in err.items()))
    for what, e in err.items():
        assert np.isfinite(e) and e <= T.TOL[what], "%s-%s: the float32 model misses the bound on %s (%.3e > %.1e)" % (name, variant, what, e, T.TOL[what])
