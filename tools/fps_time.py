"""Timing of farthest point sampling (ops.farthest_point_sample, csrc/sampling.hip) against the same algorithm written as a
torch-eager loop on the GPU, at the shapes a user of the package would run.

    python tools/fps_time.py [--repeats 3] [--out profiles/fps_time.json]

Per shape b x n -> m: both arms are warmed up, then timed `repeats` times each, the arms alternating.  A timed window is a
number of back-to-back calls between two device events, sized from the warm-up so that it lasts about 0.1 s (one call for the
torch loop, whose single call is longer than that).  Reported per arm: the median ms per call, every run, and the spread (largest
minus smallest run over the median); for the kernel also ns per pick (ms per call / m: the clouds of a batch run side by side,
one per compute unit) and the ratio torch / kernel.  Beside them the paper estimate the kernel was designed against (about
0.8 us per pick at n = 16384, 0.2 us at n = 2048, one cloud per compute unit), which is an estimate and not a measurement.
The row also says whether the two arms picked the same indices on the timed input: torch's sum over the three squares and its
arg-max among equal distances are its own, so a difference there is not an error of either arm (the kernel is pinned to its
numpy model by tests/test_gpu_fps.py).

Then the two forms of the kernel against each other where both exist (b = 1, 32, 256, 2048 clouds of n = 64 ... 1024 points,
m = n / 2): 200 calls per window, three windows per form, alternating; the ratio wave-per-cloud / workgroup-per-cloud is what
the by-size rule of form "auto" rests on."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import ops

SHAPES = [(32, 2048, 1024), (256, 2048, 512), (32, 16384, 2048), (1, 16384, 2048)]
ESTIMATE_NS_PER_PICK = {2048: 200.0, 16384: 800.0}      # from per-instruction cycle figures, before any run
COMPUTE_UNITS = 256


def torch_fps(x, m):
    """The algorithm in torch eager: per pick a gather, the squared distances, a minimum and an arg-max."""
    b, n, _ = x.shape
    rows = torch.arange(b, device=x.device)
    t = torch.full((b, n), float("inf"), device=x.device)
    idx = torch.empty((b, m), dtype=torch.int64, device=x.device)
    cur = torch.zeros(b, dtype=torch.int64, device=x.device)
    for s in range(m):
        idx[:, s] = cur
        d = x - x[rows, cur][:, None, :]
        t = torch.minimum(t, (d * d).sum(2))
        cur = torch.argmax(t, dim=1)
    return idx


def window_ms(f, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        f()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def shape_row(b, n, m, repeats, dev):
    x = torch.from_numpy(np.random.default_rng(b + n).random((b, n, 3), dtype=np.float32) - np.float32(0.5)).to(dev)
    arms = {"kernel": lambda: ops.farthest_point_sample(x, m), "torch_loop": lambda: torch_fps(x, m)}
    same = bool((arms["kernel"]().to(torch.int64) == arms["torch_loop"]()).all().item())      # first calls: code objects load here
    calls = {}
    for name, f in arms.items():                                                                # warm-up, and the window's size
        calls[name] = max(1, min(500, int(math.ceil(100.0 / max(window_ms(f, 1), 1e-3)))))
        window_ms(f, min(calls[name], 10))
    runs = {name: [] for name in arms}
    for _ in range(repeats):
        for name, f in arms.items():
            runs[name].append(window_ms(f, calls[name]))
    row = {"what": "kernel_and_torch_loop", "b": b, "n": n, "m": m, "same_indices": same, "plan": list(ops.farthest_point_sample_plan(n))}
    for name, r in runs.items():
        med = float(np.median(r))
        row[name + "_ms"] = round(med, 4)
        row[name + "_ms_runs"] = [round(v, 4) for v in r]
        row[name + "_spread"] = round((max(r) - min(r)) / med, 4)
        row[name + "_calls_per_window"] = calls[name]
    row["kernel_ns_per_pick"] = round(row["kernel_ms"] * 1e6 / m, 1)
    row["torch_over_kernel"] = round(row["torch_loop_ms"] / row["kernel_ms"], 2)
    est = ESTIMATE_NS_PER_PICK[n] * math.ceil(b / COMPUTE_UNITS)
    row["estimate_ns_per_pick_not_measured"] = est
    row["kernel_over_estimate"] = round(row["kernel_ns_per_pick"] / est, 2)
    print(json.dumps(row), flush=True)
    return row


def form_rows(repeats, dev):
    rows = []
    for b in (1, 32, 256, 2048):
        for n in (64, 128, 256, 512, 1024):
            x = torch.from_numpy(np.random.default_rng(n).random((b, n, 3), dtype=np.float32)).to(dev)
            forms = {f: (lambda f=f: ops.farthest_point_sample(x, n // 2, form=f)) for f in ("workgroup", "wave")}
            for f in forms.values():
                window_ms(f, 20)
            runs = {name: [] for name in forms}
            for _ in range(repeats):
                for name, f in forms.items():
                    runs[name].append(window_ms(f, 200))
            row = {"what": "forms", "b": b, "n": n, "m": n // 2, "auto_takes": ops.farthest_point_sample_plan(n)[0]}
            for name, r in runs.items():
                row[name + "_ms"] = round(float(np.median(r)), 5)
                row[name + "_ms_runs"] = [round(v, 5) for v in r]
            row["wave_over_workgroup"] = round(row["wave_ms"] / row["workgroup_ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "fps_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    rows = [shape_row(b, n, m, a.repeats, dev) for b, n, m in SHAPES] + form_rows(a.repeats, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
