"""Writes tests/golden/attack_plan_parent.npz: what three attack iterations give on an MI355X, and what every forward of them
launched, in each form the forward chooses among (TEST INFRASTRUCTURE; run ONCE on the GPU, at the commit whose bits and launch
decisions must be kept -- the parent of the change that plans the symmetric scan's launch before launching it):

    python tools/make_golden_attack_plan.py [--out tests/golden/attack_plan_parent.npz]

tests/test_gpu_attack_plan_bits.py imports CASES and compute() from here, rebuilds the same inputs and compares bit for bit.

Per case: AdvAE at learning_rate 1e-3, three iterations of one run() call each.  Stored: "plan" [4][9] -- the nine entries of
geoadv_attack_test_plan after the first forward and after each iteration's --, "search" [4][2] -- search_state() at the same
points --, pert, adv, recon, latent, grad, the four index arrays and "hist" [3][6][B].  compute() also asserts, through
_test_plan() and search_state(), the form the case is there for (CASES).  A case whose arrays total at most 64 KB is stored raw
("<case>/<array>"), any other as the SHA-256 of each array's bytes ("<case>/<array>.sha256").
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RAW_LIMIT = 64 * 1024
FILE_LIMIT = 300 * 1024
WEIGHT_SEED = 5
LR = 1e-3
PLAN_KEYS = ("symmetric", "screened", "rtiles", "rslices", "rows", "loss", "grad", "H", "range")
ROWS = ("final", "partials", "packed", "merge_launch")
LOSS = ("metrics", "fused", "riders")
GRAD = ("none", "fused_1pass", "fused_general", "step_fx_1pass", "step_fx_general", "step_sorted")

# name: b, n, Configuration fields, what every forward's _test_plan() must report (`form`), and optionally: scattered (the clouds
# of tests/test_gpu_backward_chain.py: duplicated columns, cloud 0 perturbed until the paired search hands it back), loss_form
# (_test_loss_form), searched (search_state()[0]).  One case per branch of the forward, at the smallest shape that reaches it.
CASES = {
    "packed_fused": dict(b=16, n=256, conf={}, form=dict(symmetric=True, screened=False, rtiles=1, rows="packed", loss="fused")),
    "packed_riders": dict(b=16, n=256, conf={"loss_in_scan": "always"}, form=dict(symmetric=True, rows="packed", loss="riders")),
    "partials_fused": dict(b=32, n=1025, conf={"chamfer_prune": False}, searched=False,
                           form=dict(symmetric=True, screened=False, rtiles=1, rows="partials", loss="fused")),
    "partials_riders": dict(b=32, n=1025, conf={"chamfer_prune": False, "loss_in_scan": "always"}, searched=False,
                            form=dict(symmetric=True, rtiles=1, rows="partials", loss="riders")),
    # two row super-tiles: the merge launch; 2049 <= 4096 points and the symmetric scan: the search rides in the scan's launch
    "merge_launch": dict(b=3, n=2049, conf={"chamfer_prune": "always"}, searched=True,
                         form=dict(symmetric=True, screened=False, rtiles=2, rows="merge_launch", loss="fused", grad="fused_general")),
    # cloud 0 is handed back: the scan's second pair has work, and with the search riding the scan the verdicts alternate between
    # the two flag buffers from forward to forward
    "handed_back": dict(b=33, n=2048, conf={"chamfer_prune": "always"}, scattered=True, searched=True,
                        form=dict(symmetric=True, screened=False, rtiles=1, rows="packed", loss="fused")),
    # more than 4096 points: the search in a launch of its own, ahead of the scans
    "search_own_launch": dict(b=1, n=4097, conf={"chamfer_prune": "always"}, searched=True,
                              form=dict(symmetric=True, rows="merge_launch", loss="fused")),
    "screened": dict(b=64, n=2048, conf={"chamfer_prune": False}, searched=False,
                     form=dict(symmetric=True, screened=True, rtiles=1, rows="partials", loss="fused")),
    # below 4096 points in the batch: the two-scan kernel and the masked encoder backward
    "two_scan": dict(b=2, n=256, conf={}, searched=False, form=dict(symmetric=False, rows="final", loss="fused")),
    "search_beside_latent": dict(b=29, n=256, conf={"chamfer_kernel": "two_scan", "chamfer_prune": "always"}, searched=True,
                                 form=dict(symmetric=False, rows="final", loss="fused")),
    # the EMD launch lies between the scan and the loss launch: never hosted, whatever loss_in_scan says
    "emd": dict(b=16, n=256, conf={"emd_weight": 0.5}, form=dict(symmetric=True, rows="packed", loss="fused")),
    "emd_always": dict(b=16, n=256, conf={"emd_weight": 0.5, "loss_in_scan": "always"}, form=dict(symmetric=True, rows="packed", loss="fused")),
    # bit 0: packed words only from 9 slices on -- 8 partials instead; bit 1: the general gradient body, words folded through LDS
    "loss_form_1": dict(b=16, n=256, conf={}, loss_form=1, form=dict(symmetric=True, rslices=8, rows="partials", loss="fused", grad="fused_1pass")),
    "loss_form_2": dict(b=16, n=256, conf={}, loss_form=2, form=dict(symmetric=True, rows="packed", loss="fused", grad="fused_general")),
    "latent_pert": dict(b=16, n=256, conf={"loss_adv_type": "latent", "loss_dist_type": "pert"},
                        form=dict(symmetric=True, loss="metrics", grad="none", H=0)),
}


def _cloud(seed, b, n):
    rng = np.random.default_rng(seed)
    return (rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def inputs(b, n, scattered):
    x, gt = _cloud(601, b, n), _cloud(602, b, n)
    rng = np.random.default_rng(603)
    p0 = (1e-3 * rng.standard_normal((b, n, 3))).astype(np.float32)
    if scattered:
        for a in (x, gt):
            a[:, n // 2] = a[:, 3]
            a[:, n - 1] = a[:, 3]
        p0[0] = (0.3 * (rng.random((n, 3)) - 0.5)).astype(np.float32)
    return x, gt, p0


_models = {}


def _model(n):
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    if n not in _models:
        _models.clear()
        w = W.randomized_weights(n, seed=WEIGHT_SEED)
        _models[n] = (w, PointNetAE(w, n))
    return _models[n]


def compute(name):
    """dict array name -> numpy array of one case (needs the GPU)."""
    import torch
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    case = CASES[name]
    b, n = case["b"], case["n"]
    w, ae = _model(n)
    x, gt, p0 = inputs(b, n, case.get("scattered", False))
    at = AdvAE("golden", Configuration(batch_size=b, n_points=n, weights=w, learning_rate=LR, num_iterations=3,
                                       num_iterations_thresh=1, **case["conf"]), ae=ae)
    at.set_inputs(x, gt, ae.transform(gt), np.resize(np.array([1.0, 150.0, 0.3], np.float32), b))
    at.init_pert(p0, reset_optimizer=True)
    if "loss_form" in case:
        at._test_loss_form(case["loss_form"])
    plans, search, hist = [], [], []

    def look():
        p = at._test_plan()
        for k, v in case["form"].items():
            assert p[k] == v, "%s: the forward reports %s = %r, the case is there for %r" % (name, k, p[k], v)
        s = at.search_state()
        if "searched" in case:
            assert s[0] is case["searched"], name
        plans.append([int(p["symmetric"]), int(p["screened"]), p["rtiles"], p["rslices"], ROWS.index(p["rows"]), LOSS.index(p["loss"]),
                      GRAD.index(p["grad"]), p["H"], p["range"]])
        search.append([int(s[0]), s[1]])

    look()
    for it in range(3):
        h = torch.empty((1, 6, b), dtype=torch.float32, device=at.device)
        at.run(it, 1, 1, h)
        look()
        hist.append(h[0].cpu().numpy())
    at.status()
    if case.get("scattered"):
        assert 1 <= search[-1][1] < b, "%s: cloud 0 alone was scattered, %d clouds are handed back" % (name, search[-1][1])
    out = {k: v.cpu().numpy() for k, v in at.peek().items()}
    out["plan"] = np.array(plans, np.int32)
    out["search"] = np.array(search, np.int32)
    out["hist"] = np.stack(hist)
    ae.status()
    return out


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attack_plan_parent.npz"))
    a = ap.parse_args()
    out = {}
    for case in CASES:
        arrays = compute(case)
        raw = sum(v.nbytes for v in arrays.values()) <= RAW_LIMIT
        for k, v in arrays.items():
            assert np.isfinite(v).all() if v.dtype.kind == "f" else True, (case, k)
            if raw or k in ("plan", "search"):                      # (the read-outs are always stored raw: a mismatch names its entry)
                out["%s/%s" % (case, k)] = v
            else:
                out["%s/%s.sha256" % (case, k)] = np.array(sha256(v))
        print(case, "raw" if raw else "sha256", "plan", arrays["plan"].tolist(), "search", arrays["search"].tolist(), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    size = os.path.getsize(a.out)
    assert size < FILE_LIMIT, size
    print("wrote %s (%d bytes, %d keys)" % (a.out, size, len(out)))


if __name__ == "__main__":
    main()
