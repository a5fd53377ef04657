"""The loop's loss / Chamfer-gradient launch in its short form (packed row minima from 8 column slices on, one-pass gradient body:
csrc/loss_cgrad.h) against the forms it replaced (geoadv_attack_test_loss_form: bit 0 = partials per slice at 8 slices, bit 1 = the
general gradient body and the packed words folded through LDS): trajectories bit for bit, then us per iteration, alternating, the
median of REPS windows of 400 iterations and their spread.
    python tools/debug/loss_form_ab.py [B ...]"""
import os, sys, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from geometric_adv_amd import weights as W
from geometric_adv_amd.adv_ae import AdvAE, Configuration
from geometric_adv_amd.autoencoder import PointNetAE
N = 2048
ITERS = int(os.environ.get("ITERS", "60"))
REPS = int(os.environ.get("REPS", "7"))
FORMS = (0, 1, 2, 3)
w = W.synthetic_weights(N, seed=7); ae = PointNetAE(w, N)
for B in [int(a) for a in sys.argv[1:]] or [32, 64, 4, 10, 16]:
    rng = np.random.default_rng(B)
    x = rng.random((B, N, 3), dtype=np.float32) - np.float32(0.5); gt = rng.random((B, N, 3), dtype=np.float32) - np.float32(0.5)
    hs, ats = {}, {}
    for form in FORMS:
        at = AdvAE("a", Configuration(batch_size=B, n_points=N, weights=w, num_iterations=ITERS + 10 ** 5, num_iterations_thresh=50), ae=ae)
        at._test_loss_form(form)
        at.set_inputs(x, gt, ae.transform(gt), 1.0); at.init_pert(None, reset_optimizer=True)
        h = torch.empty((ITERS, 6, B), device=ae.device)
        at.run(0, ITERS, 50, h); at.status()
        hs[form] = h.cpu().numpy(); ats[form] = at
    same = all(bool(np.array_equal(hs[0], hs[f])) and all(torch.equal(ats[0].peek()[k], ats[f].peek()[k]) for k in ("pert", "idx_r1", "idx_a1", "grad"))
               for f in FORMS[1:])
    us = {f: [] for f in FORMS}
    for rep in range(REPS):
        for f in FORMS:
            at = ats[f]
            at.run(ITERS, 20, 10 ** 6); torch.cuda.synchronize()
            t0 = time.perf_counter(); at.run(ITERS + 20, 400, 10 ** 6); torch.cuda.synchronize()
            us[f].append((time.perf_counter() - t0) / 400 * 1e6)
    print(json.dumps({"B": B, "bit_identical_iterations": ITERS if same else False,
                      "us_per_it_median": {str(f): round(float(np.median(us[f])), 2) for f in FORMS},
                      "us_per_it_spread": {str(f): round(max(us[f]) - min(us[f]), 2) for f in FORMS}}), flush=True)
    del ats
