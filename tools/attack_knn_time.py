"""Timing of the attack iteration with and without the kNN outlier term (geoadv_attack_config.knn_weight; the second instance of
csrc/knn_loss.hip's launch called from do_step) at 32 x 2048 and 10 x 2048 points, chamfer / chamfer losses, a random-init victim.

    python tools/attack_knn_time.py [--iters 200] [--windows 20] [--bench-json FILE] [--out profiles/attack_knn_time.json]

Arms, per batch size: knn_weight = 0 and knn_weight = 5 (knn_k 5, knn_alpha 1.05), one handle each on the same inputs.  Every
arm is warmed up; then `windows` timed windows per arm, the arms alternating, each window the FIRST `iters` iterations of an
attack (perturbation and Adam slots reset before the clock starts; one geoadv_attack_run between two device events).  Reported
per arm: the median ms per iteration over the windows, the smallest and the largest window, and the spread (largest minus
smallest over the median).  For the arm with the term, the public op alone (ops.knn_outlier_loss with its allocations, 100
back-to-back calls) on the source clouds and on the adversarial clouds a window ends with: the term's cost follows the cloud.
After the windows each handle runs the same `iters` iterations once more under AdvAE.profile(True): ms per iteration of every
kernel class (events around each class's launches: they include the dispatch gaps, and the events themselves slow the loop, so
these do not add up to the window figure).
--bench-json: a file of bench.py result lines recorded elsewhere (the parent commit and this one, alternating) copied into the
output under "bench_default_path" as they are."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import weights as W
from geometric_adv_amd.adv_ae import AdvAE, Configuration, PROF_NAMES
from geometric_adv_amd.autoencoder import PointNetAE

N, K, ALPHA, WEIGHT = 2048, 5, 1.05, 5.0
BATCHES = (32, 10)


def window_ms(at, iters):
    """ms per iteration of `iters` iterations from the SAME start (the perturbation and Adam's slots are reset before the clock
    starts): the term's cost depends on the cloud -- its search on how the points cluster, its gradient launch on how many masked
    points name one neighbour -- and the cloud moves with every iteration, so windows that continued one another would time
    different work."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    at.init_pert(reset_optimizer=True)
    torch.cuda.synchronize()
    start.record()
    at.run(0, iters, iters + 1)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def op_ms(pc, calls=100):
    from geometric_adv_amd import ops
    ops.knn_outlier_loss(pc, K, ALPHA)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        ops.knn_outlier_loss(pc, K, ALPHA)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--windows", type=int, default=20)
    p.add_argument("--bench-json", type=str, default=None)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "attack_knn_time.py measures on the GPU"
    assert a.windows >= 1 and a.iters >= 1
    rng = np.random.default_rng(0)
    v = rng.normal(size=(2 * max(BATCHES), N, 3))
    v = v / np.linalg.norm(v, axis=2, keepdims=True) * (1.0 + 0.02 * rng.normal(size=(2 * max(BATCHES), N, 1)))
    clouds = (0.5 * v).astype(np.float32)                      # noisy spheres: a surface with a few points off it
    w = W.randomized_weights(N)
    ae = PointNetAE(w, N)
    arms = {}
    for b in BATCHES:
        x, gt = clouds[:b], clouds[max(BATCHES):max(BATCHES) + b]
        tz = ae.transform(gt).astype(np.float32)
        for name, weight in (("knn_weight_0", 0.0), ("knn_weight_5", WEIGHT)):
            conf = Configuration(batch_size=b, n_points=N, weights=None, chamfer_prune="pinned", knn_weight=weight, knn_k=K, knn_alpha=ALPHA)
            at = AdvAE("attack_knn_time", conf, ae=ae)
            at.set_inputs(x, gt, tz, 1.0)
            at.init_pert(reset_optimizer=True)
            arms["%s_b%d" % (name, b)] = at
    for at in arms.values():                                   # warm-up: code objects load, the search's verdicts settle
        window_ms(at, 20)
    runs = {name: [] for name in arms}
    for _ in range(a.windows):
        for name, at in arms.items():
            runs[name].append(window_ms(at, a.iters))
    out = {"what": "attack_knn_time", "n": N, "knn_k": K, "knn_alpha": ALPHA, "knn_weight": WEIGHT, "batches": list(BATCHES),
           "iterations_per_window": a.iters, "windows": a.windows, "device": torch.cuda.get_device_name(0)}
    for name, r in runs.items():
        med = float(np.median(r))
        out[name] = {"median_ms": round(med, 5), "min_ms": round(min(r), 5), "max_ms": round(max(r), 5),
                     "spread": round((max(r) - min(r)) / med, 4)}
    for name, at in arms.items():                              # the public op alone on the clouds the term worked on (with its allocations)
        if not name.startswith("knn_weight_5"):
            continue
        b = at.B
        out[name]["op_alone_ms"] = {"on_the_sources": round(op_ms(torch.as_tensor(clouds[:b], device=at.device)), 5),
                                    "on_adv_after_a_window": round(op_ms(at.peek()["adv"]), 5)}
    for name, at in arms.items():                              # the profiler's classes, in a run of their own
        at.init_pert(reset_optimizer=True)
        at.profile(True)
        at.run(0, a.iters, a.iters + 1)
        torch.cuda.synchronize()
        read = at.profile_read()
        at.profile(False)
        out[name]["class_ms_per_iteration"] = {c: round(read[c][1] / a.iters, 5) for c in PROF_NAMES}
        out[name]["class_launch_scopes_per_iteration"] = {c: round(read[c][0] / a.iters, 3) for c in PROF_NAMES}
    if a.bench_json:
        with open(a.bench_json) as f:
            out["bench_default_path"] = json.load(f)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
