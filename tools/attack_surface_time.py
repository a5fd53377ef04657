"""Timing of the attack iteration without the kNN term, with it under the SOR rule and with it under the surface rule
(geoadv_attack_config.knn_rule / knn_thresh; the surface instances of csrc/knn_loss.hip's launch called from do_step) at
32 x 2048 and 10 x 2048 points, chamfer / chamfer losses, a random-init victim.  The protocol of tools/attack_knn_time.py.

    python tools/attack_surface_time.py [--iters 200] [--windows 20] [--bench-json FILE] [--out profiles/attack_surface_time.json]

Arms, per batch size, one handle each on the same inputs: knn_weight = 0; knn_weight = 5 under the SOR rule (knn_k 5, knn_alpha
1.05); knn_weight = 5 under the surface rule (knn_k 2, knn_thresh 0.04).  Every arm is warmed up; then `windows` timed windows
per arm, the arms alternating, each window the FIRST `iters` iterations of an attack (perturbation and Adam slots reset before
the clock starts; one geoadv_attack_run between two device events).  Reported per arm: the median ms per iteration over the
windows, the smallest and the largest window, and the spread (largest minus smallest over the median).  For the arms with the
term, the public op alone under the arm's rule (ops.knn_outlier_loss with its allocations, 100 back-to-back calls) on the source
clouds and on the adversarial clouds a window ends with, and how many points the rule masks there.  After the windows each
handle runs the same `iters` iterations once more under AdvAE.profile(True): ms per iteration of every kernel class (events
around each class's launches: they include the dispatch gaps, and the events themselves slow the loop, so these do not add up
to the window figure).
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

N, WEIGHT = 2048, 5.0
BATCHES = (32, 10)
ARMS = {        # name -> Configuration arguments, the op's arguments under the arm's rule
    "term_off": (dict(knn_weight=0.0), None),
    "sor_k5": (dict(knn_weight=WEIGHT, knn_k=5, knn_alpha=1.05), dict(k=5, alpha=1.05)),
    "surface_k2": (dict(knn_weight=WEIGHT, knn_k=2, knn_rule="surface", knn_thresh=0.04), dict(k=2, rule="surface", thresh=0.04)),
}


def window_ms(at, iters):
    """ms per iteration of `iters` iterations from the SAME start (the perturbation and Adam's slots are reset before the clock
    starts): the term's cost follows the cloud, and the cloud moves with every iteration."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    at.init_pert(reset_optimizer=True)
    torch.cuda.synchronize()
    start.record()
    at.run(0, iters, iters + 1)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def op_ms(pc, op_args, calls=100):
    from geometric_adv_amd import ops
    ops.knn_outlier_loss(pc, **op_args)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        ops.knn_outlier_loss(pc, **op_args)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def masked_per_cloud(pc, op_args):
    from geometric_adv_amd import ops
    return float(ops.knn_outlier_loss(pc, want_grad=False, return_parts=True, **op_args)[5][:, 3].mean())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--windows", type=int, default=20)
    p.add_argument("--bench-json", type=str, default=None)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "attack_surface_time.py measures on the GPU"
    assert a.windows >= 1 and a.iters >= 1
    rng = np.random.default_rng(0)
    v = rng.normal(size=(2 * max(BATCHES), N, 3))
    v = v / np.linalg.norm(v, axis=2, keepdims=True) * (1.0 + 0.02 * rng.normal(size=(2 * max(BATCHES), N, 1)))
    clouds = (0.5 * v).astype(np.float32)                      # noisy spheres: a surface with a few points off it
    ae = PointNetAE(W.randomized_weights(N), N)
    arms, op_args = {}, {}
    for b in BATCHES:
        x, gt = clouds[:b], clouds[max(BATCHES):max(BATCHES) + b]
        tz = ae.transform(gt).astype(np.float32)
        for name, (conf_args, op) in ARMS.items():
            conf = Configuration(batch_size=b, n_points=N, weights=None, chamfer_prune="pinned", **conf_args)
            at = AdvAE("attack_surface_time", conf, ae=ae)
            at.set_inputs(x, gt, tz, 1.0)
            at.init_pert(reset_optimizer=True)
            arms["%s_b%d" % (name, b)] = at
            op_args["%s_b%d" % (name, b)] = op
    for at in arms.values():                                   # warm-up: code objects load, the search's verdicts settle
        window_ms(at, 20)
    runs = {name: [] for name in arms}
    for _ in range(a.windows):
        for name, at in arms.items():
            runs[name].append(window_ms(at, a.iters))
    out = {"what": "attack_surface_time", "n": N, "knn_weight": WEIGHT, "arms": {k: v[0] for k, v in ARMS.items()},
           "batches": list(BATCHES), "iterations_per_window": a.iters, "windows": a.windows, "device": torch.cuda.get_device_name(0)}
    for name, r in runs.items():
        med = float(np.median(r))
        out[name] = {"median_ms": round(med, 5), "min_ms": round(min(r), 5), "max_ms": round(max(r), 5),
                     "spread": round((max(r) - min(r)) / med, 4)}
    for name, at in arms.items():                              # the public op alone on the clouds the term worked on (with its allocations)
        if op_args[name] is None:
            continue
        src, adv = torch.as_tensor(clouds[:at.B], device=at.device), at.peek()["adv"]
        out[name]["op_alone_ms"] = {"on_the_sources": round(op_ms(src, op_args[name]), 5),
                                    "on_adv_after_a_window": round(op_ms(adv, op_args[name]), 5)}
        out[name]["masked_points_per_cloud"] = {"on_the_sources": round(masked_per_cloud(src, op_args[name]), 2),
                                                "on_adv_after_a_window": round(masked_per_cloud(adv, op_args[name]), 2)}
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
