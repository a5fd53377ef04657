"""CPU: the measurement behind the constants of tests/test_gpu_cls_grad.py (no GPU involved).

    python tools/cls_grad_tolerance.py [--out profiles/cls_grad_tolerance.json]

1. F32_PRE_ERR / F32_LOGIT_ERR: the torch graph of tests/_cls_grad_model64.py in float32 against float64 on a broad sample
   of the test's cloud generator (seeds 0 .. 3 of every (classes, n)): per layer max |pre32 - pre64| / max |pre64| over a
   cloud, and max |Z32 - Z64| / max |Z64|; the worst over the sample.
2. CASE_SEED: per (classes, n) the first seed whose three clouds keep TWICE the margins the test asks for (4 x the errors
   of step 1), for all three losses, in the float64 model alone.
3. F32_GRAD_ERR: on the chosen cases, all three losses, float32 (float64's winners handed in) against float64: max-abs
   over the cloud / the cloud's max-abs gradient; the worst cloud.
The test file carries the printed values.

    python tools/cls_grad_tolerance.py --tiles 1 [--out profiles/cls_grad_tiles_tolerance.json]

the same for tests/test_gpu_cls_grad_tiles.py (sphere clouds of 700 ... 8192 points, one cloud at a time):
1. F32_PRE_ERR / F32_LOGIT_ERR on seeds 0 .. 7 of every (classes, n) and two clouds of 8192 points; float32 runs with the
   winners AND the ReLU masks of float64 pinned (relu_override), as the test resolves masks instead of screening them.
2. CASE_SEED: per (classes, n, b) the first two unused seeds whose cloud meets the test's caps (check_caps: no open head
   unit, the CW margins, at most 64 open per-point units and 8 % of the winner rows) for all three losses.
3. MOST_TILES: among spheres of 8192 points (seeds 0 .. 5, radius 0.45 and 1, both classifiers) that meet the caps, the one
   with the most distinct winner rows in one pool.
4. F32_GRAD_ERR on the chosen clouds, all three losses; the errors of step 1 are extended by these clouds and steps 2 - 4
   repeated if that moved a window."""
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
    ap.add_argument("--tiles", type=int, default=0, help="1: the constants of tests/test_gpu_cls_grad_tiles.py")
    flags = ap.parse_args(argv)
    import _cls_grad_model64 as G
    if flags.tiles:
        return tiles(flags, G)
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


def tiles(flags, G):
    import test_gpu_cls_grad_tiles as T

    def pinned32(C, x, y, loss, r):
        masks = {s: r["pres"][s] > 0 for s in r["pres"]}
        return G.grad_model(T._weights(C), x[None], np.array([y]), loss, T.KAPPA, winners=r["winners"], dtype=torch.float32,
                            relu_override=masks)

    pre_err, logit_err = {}, [0.0]

    def forward_errors(C, x, r):
        f = pinned32(C, x, 0, "xent", r)
        moved = False
        for s in list(G.HEADS) + sorted({s for u in G.UNDER.values() for s in u}):
            e = float(np.abs(f["pres"][s][0] - r["pres"][s][0]).max() / np.abs(r["pres"][s][0]).max())
            moved |= e > pre_err.get(s, 0.0)
            pre_err[s] = max(pre_err.get(s, 0.0), e)
        logit_err[0] = max(logit_err[0], float(np.abs(f["logits"] - r["logits"]).max() / np.abs(r["logits"]).max()))
        return moved

    def publish():
        T.F32_PRE_ERR = {k: float("%.2e" % v) for k, v in pre_err.items()}
        T.F32_LOGIT_ERR = float("%.2e" % logit_err[0])
        T.WINDOW = {s: (8 if s in G.HEADS else 2) * e for s, e in T.F32_PRE_ERR.items()}

    def meets_caps(C, x, seed, own, losses=G.LOSSES):
        labels = T.labels_of(seed, C, own["logits"][0])
        try:
            for loss in losses:
                T.check_caps(G.grad_model(T._weights(C), x[None], np.array([labels[loss]]), loss, T.KAPPA), loss)
        except AssertionError as e:
            return str(e)
        return None

    for C in (13, 40):
        for n, count in ((700, 8), (1024, 8), (2048, 8), (8192, 2)):
            for seed in range(count):
                x = T.sphere(seed, n)
                forward_errors(C, x, T.forward64(C, x))
    for attempt in range(3):
        publish()
        print("F32_LOGIT_ERR = %.2e" % logit_err[0])
        print("F32_PRE_ERR = {%s}" % ", ".join('"%s": %.2e' % kv for kv in pre_err.items()), flush=True)
        seeds, winners, chosen = {}, {}, []
        for C in (13, 40):
            nxt = {}
            for n, b in T.CASES:
                found, seed = [], nxt.get(n, 0)
                while len(found) < 2:
                    x = T.sphere(seed, n)
                    own = T.forward64(C, x)
                    why = meets_caps(C, x, seed, own)
                    if why is None:
                        found.append(seed)
                        chosen.append((C, n, seed, 1.0 * T.RADIUS))
                        winners.setdefault((n, b), []).append([len(G.winner_rows(own, 0, p)) for p in range(3)])
                    else:
                        print("  left out: classes %d n %d seed %d: %s" % (C, n, seed, why))
                    seed += 1
                    if seed > flags.max_seed:
                        raise SystemExit("no seeds for %s" % ((C, n, b),))
                nxt[n] = seed
                seeds[(C, n, b)] = tuple(found)
        print("CASE_SEED = %r" % seeds)
        for k, v in winners.items():
            v = np.array(v)
            print("n %d b %d: distinct winners %s, slot tiles %s" % (k + (
                " / ".join("%d-%d" % (v[:, p].min(), v[:, p].max()) for p in range(3)),
                " / ".join("%d-%d" % (-(-v[:, p].min() // 64), -(-v[:, p].max() // 64)) for p in range(3)))), flush=True)
        best = None
        for C in (13, 40):
            for radius in (T.RADIUS, 1.0):
                for seed in range(6):
                    x = T.sphere(seed, 8192, radius)
                    own = T.forward64(C, x)
                    cnt = [len(G.winner_rows(own, 0, p)) for p in range(3)]
                    why = meets_caps(C, x, seed, own, ("xent",))
                    print("  most tiles: classes %d radius %.2f seed %d winners %s %s" % (C, radius, seed, cnt, why or ""), flush=True)
                    if why is None and (best is None or max(cnt) > best["winners"]):
                        best = dict(num_classes=C, n=8192, seed=seed, radius=radius, loss="xent", pool=int(np.argmax(cnt)), winners=max(cnt))
        print("MOST_TILES = %r  (slot tile %d of 16)" % (best, -(-best["winners"] // 64)))
        chosen.append((best["num_classes"], 8192, best["seed"], best["radius"]))
        worst, moved = 0.0, False
        for C, n, seed, radius in chosen:
            x = T.sphere(seed, n, radius)
            own = T.forward64(C, x)
            moved |= forward_errors(C, x, own)
            for loss, y in T.labels_of(seed, C, own["logits"][0]).items():
                if n == 8192 and loss != best["loss"]:
                    continue
                r = G.grad_model(T._weights(C), x[None], np.array([y]), loss, T.KAPPA)
                f = pinned32(C, x, y, loss, r)
                worst = max(worst, float(T.row_err(f["grad"][0], r["grad"][0]).max()))
        print("F32_GRAD_ERR = %.2e" % worst, flush=True)
        if not moved:
            break
        print("the chosen clouds moved a forward error: once more")
    if flags.out:
        with open(flags.out, "w") as fh:
            json.dump(dict(f32_pre_err=pre_err, f32_logit_err=logit_err[0], f32_grad_err=worst, most_tiles=best,
                           case_seed={"%d,%d,%d" % k: v for k, v in seeds.items()}), fh, indent=1)


if __name__ == "__main__":
    main()
