"""Timing of the two baseline defenses' device side (ops.sor_filter, ops.random_drop; csrc/stat_defense.hip) at 32 x 2048
points, against the same computations written in torch eager on the same GPU.

    python tools/stat_defense_time.py [--calls 200] [--windows 20] [--out profiles/stat_defense_time.json]

Arms:
  sor_filter_with_knn   ops.sor_filter(pc, k=2, alpha=1.1): the kNN distances (ops.knn_dists) and the filter
  sor_kernel_alone      ops.sor_filter(pc, knn, k=2, alpha=1.1) on distances computed before the window
  torch_sor             IF-Defense's form: torch.cdist, topk(k + 1, largest=False), the mean of the k distances, mean + alpha * std
                        per cloud, a stable argsort of the mask to pack inliers and outliers, the padding by gather
  random_drop           ops.random_drop(pc, 500, seed, counter=call ordinal, return_idx=True)
  torch_srs             torch.rand + argsort per cloud, the kept points gathered in point order and padded
Every arm is warmed up; then `windows` timed windows per arm, the arms alternating, each window `calls` back-to-back calls
between two device events (an op's call includes the allocation of its outputs and the launch, as a user's call does).  Reported
per arm: the median ms per call over the windows, the smallest and the largest window, and the spread (largest minus smallest over
the median).  No ratio is asserted anywhere: the kernels are launch- and latency-bound at this size (DESIGN), and the torch arms
are what a user would otherwise write, not the same rule (torch's reductions have their own order, its generator its own
stream)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import ops

B, N, K, ALPHA, DROP = 32, 2048, 2, 1.1, 500


def pack(pc, mask):
    """The points with mask in point order, padded with the last of them -> (packed, count)."""
    n = pc.shape[1]
    order = torch.argsort((~mask).to(torch.uint8), dim=1, stable=True)
    count = mask.sum(dim=1, keepdim=True)
    slot = torch.arange(n, device=pc.device)[None, :]
    src = torch.where(slot < count, order, torch.gather(order, 1, (count - 1).clamp(min=0)))
    return torch.gather(pc, 1, src.unsqueeze(-1).expand(-1, -1, 3)), count


def torch_sor(pc, k, alpha):
    d = torch.cdist(pc, pc)
    score = d.topk(k + 1, dim=2, largest=False).values[:, :, 1:].mean(dim=2)
    thresh = score.mean(dim=1, keepdim=True) + alpha * score.std(dim=1, keepdim=True)
    inl = score <= thresh
    inlier, _ = pack(pc, inl)
    outlier, num = pack(pc, ~inl)
    return outlier, num, inlier


def torch_srs(pc, drop):
    b, n, _ = pc.shape
    order = torch.argsort(torch.rand((b, n), device=pc.device), dim=1)
    mask = torch.ones((b, n), dtype=torch.bool, device=pc.device)
    mask.scatter_(1, order[:, :drop], False)
    kept, _ = pack(pc, mask)
    return kept, torch.sort(order[:, :drop], dim=1).values


def window_ms(f, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        f()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--windows", type=int, default=20)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "stat_defense_time.py measures on the GPU"
    assert a.windows >= 1 and a.calls >= 1
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    v = rng.normal(size=(B, N, 3))
    pc = torch.from_numpy((v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float32)).to(dev)       # clouds on the unit sphere
    knn = ops.knn_dists(pc, K)
    step = [0]

    def srs():
        step[0] += 1
        return ops.random_drop(pc, DROP, 0, counter=step[0], return_idx=True)
    arms = {"sor_filter_with_knn": lambda: ops.sor_filter(pc, k=K, alpha=ALPHA),
            "sor_kernel_alone": lambda: ops.sor_filter(pc, knn, k=K, alpha=ALPHA),
            "torch_sor": lambda: torch_sor(pc, K, ALPHA),
            "random_drop": srs,
            "torch_srs": lambda: torch_srs(pc, DROP)}
    # what the arms compute, side by side (not timed): the torch form's own summation order may move a borderline point
    o_num = ops.sor_filter(pc, knn, k=K, alpha=ALPHA)[2].to(torch.int64)
    t_num = torch_sor(pc, K, ALPHA)[1].reshape(-1)
    for f in arms.values():                                   # warm-up: code objects load, torch picks its algorithms
        window_ms(f, 10)
    runs = {name: [] for name in arms}
    for _ in range(a.windows):
        for name, f in arms.items():
            runs[name].append(window_ms(f, a.calls))
    out = {"what": "stat_defense_time", "b": B, "n": N, "k": K, "alpha": ALPHA, "drop": DROP, "calls_per_window": a.calls,
           "windows": a.windows, "device": torch.cuda.get_device_name(0),
           "sor_outliers_per_cloud_mean": round(float(o_num.float().mean().item()), 2),
           "sor_clouds_where_torch_counts_differ": int((o_num != t_num).sum().item())}
    for name, r in runs.items():
        med = float(np.median(r))
        out[name] = {"median_ms": round(med, 5), "min_ms": round(min(r), 5), "max_ms": round(max(r), 5),
                     "spread": round((max(r) - min(r)) / med, 4)}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
