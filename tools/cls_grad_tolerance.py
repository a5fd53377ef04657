"""CPU: the measurement behind the constants of tests/test_gpu_cls_grad.py (no GPU involved).

    python tools/cls_grad_tolerance.py [--out profiles/cls_grad_tolerance.json]

1. F32_PRE_ERR / F32_LOGIT_ERR: the torch graph of tests/_cls_grad_model64.py in float32 against float64 on a broad sample
   of the test's cloud generator (seeds 0 .. 3 of every (classes, n)): per layer max |pre32 - pre64| / max |pre64| over a
   cloud, and max |Z32 - Z64| / max |Z64|; the worst over the sample.
2. CASE_SEED: per (classes, n) the first seed whose three clouds keep TWICE the margins the test asks for (4 x the errors
   of step 1), for all three losses, in the float64 model alone.
3. F32_GRAD_ERR: on the chosen cases, all three losses, float32 (float64's winners handed in) against float64: max-abs
   over the cloud / the cloud's max-abs gradient; the worst cloud.
The test file carries the printed values."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--max_seed", type=int, default=2000)
    ap.add_argument("--forward", type=int, default=1, help="0: keep the test file's F32_PRE_ERR / F32_LOGIT_ERR (skip step 1)")
    flags = ap.parse_args(argv)
    import _cls_grad_model64 as G
    import test_gpu_cls_grad as T

    def both(C, n, loss, seed):
        x, y = T.make_case(seed, C, n, loss)
        r = G.grad_model(T._weights(C), x, y, loss, T.KAPPA)
        f = G.grad_model(T._weights(C), x, y, loss, T.KAPPA, winners=r["winners"], dtype=torch.float32)
        return r, f

    pre_err, logit_err = dict(T.F32_PRE_ERR), T.F32_LOGIT_ERR
    for C in (13, 40) if flags.forward else ():
        for n in T.NS:
            for seed in range(4):
                r, f = both(C, n, "xent", seed)
                for s in r["margin_layers"]:
                    for c in range(T.CLOUDS):
                        e = np.abs(f["pres"][s][c] - r["pres"][s][c]).max() / np.abs(r["pres"][s][c]).max()
                        pre_err[s] = max(pre_err.get(s, 0.0), float(e))
                e = np.abs(f["logits"] - r["logits"]).max(1) / np.abs(r["logits"]).max(1)
                logit_err = max(logit_err, float(e.max()))
    print("F32_LOGIT_ERR = %.2e" % logit_err)
    print("F32_PRE_ERR = {%s}" % ", ".join('"%s": %.2e' % kv for kv in pre_err.items()))
    T.F32_PRE_ERR, T.F32_LOGIT_ERR = {k: float("%.2e" % v) for k, v in pre_err.items()}, float("%.2e" % logit_err)

    seeds = {}
    for C in (13, 40):
        for n in T.NS:
            found = []
            for seed in range(flags.max_seed):
                if all(T.keep_mask(G.grad_model(T._weights(C), *T.make_case((seed,), C, n, loss), loss, T.KAPPA), factor=1.25).all()
                       for loss in G.LOSSES):
                    found.append(seed)
                    if len(found) == T.CLOUDS:
                        break
            else:
                raise SystemExit("fewer than %d seeds below %d for %s" % (T.CLOUDS, flags.max_seed, (C, n)))
            seeds[(C, n)] = tuple(found)
            print("seed", (C, n), seeds[(C, n)], flush=True)
    print("CASE_SEED = %r" % seeds)

    worst, rows = 0.0, []
    for (C, n), seed in seeds.items():
        for loss in G.LOSSES:
            r, f = both(C, n, loss, seed)
            scale = np.abs(r["grad"]).reshape(T.CLOUDS, -1).max(1)
            e = np.abs(f["grad"] - r["grad"]).reshape(T.CLOUDS, -1).max(1) / scale
            rows.append(dict(classes=C, n=n, loss=loss, seed=seed, f32_grad_err=e.tolist(), max_abs_grad=scale.tolist()))
            worst = max(worst, float(e.max()))
    print("F32_GRAD_ERR = %.2e" % worst)
    if flags.out:
        with open(flags.out, "w") as fh:
            json.dump(dict(f32_pre_err=pre_err, f32_logit_err=logit_err, case_seed={"%d,%d" % k: v for k, v in seeds.items()},
                           f32_grad_err=worst, cases=rows), fh, indent=1)


if __name__ == "__main__":
    main()
