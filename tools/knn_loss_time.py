"""Timing of the kNN outlier loss (ops.knn_outlier_loss; csrc/knn_loss.hip) at 32 x 2048 and 10 x 2048 points, k = 5,
alpha = 1.05, against the same loss and gradient written in torch eager on the same GPU.

    python tools/knn_loss_time.py [--calls 200] [--windows 20] [--out profiles/knn_loss_time.json]

Arms, per batch size:
  op             ops.knn_outlier_loss(pc, 5, 1.05): the search (geoadv_knn_point_ws) and the new launch, with the allocation of the
                 outputs and of the workspace, as a user's call
  launch_alone   the launch after the search alone (geoadv_debug_knn_outlier_loss_launch) on a workspace that holds the search of
                 the same clouds, outputs allocated before the window
  torch          cdist, topk(k + 1, largest=False), a gather of the neighbours, the score, mean + alpha * std, the masked mean,
                 autograd for the gradient (the mask detached, as the rule holds it constant)
Every arm is warmed up; then `windows` timed windows per arm, the arms alternating, each window `calls` back-to-back calls
between two device events.  Reported per arm: the median ms per call over the windows, the smallest and the largest window, and
the spread (largest minus smallest over the median).  No ratio is asserted: the torch arm is what a user would otherwise write,
not the same rule (its reductions have their own order, so a borderline point may change sides)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import _lib, ops

N, K, ALPHA = 2048, 5, 1.05
BATCHES = (32, 10)


def torch_knn_loss(pc, k, alpha):
    x = pc.detach().clone().requires_grad_(True)
    with torch.no_grad():
        idx = torch.cdist(x, x).topk(k + 1, dim=2, largest=False).indices[:, :, 1:]
    b, n, _ = x.shape
    nb = x[torch.arange(b, device=x.device)[:, None, None], idx]
    score = ((x.unsqueeze(2) - nb) ** 2).sum(-1).mean(-1)
    with torch.no_grad():
        mask = score > score.mean(dim=1, keepdim=True) + alpha * score.std(dim=1, keepdim=True)
    loss = (score * mask).sum(dim=1) / n
    loss.sum().backward()
    return loss.detach(), x.grad


def window_ms(f, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        f()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def launch_alone(pc):
    """-> a callable that repeats the launch after the search on a workspace one full call has filled."""
    b, n, _ = pc.shape
    lib = _lib.lib()
    wb = int(lib.geoadv_knn_outlier_loss_workspace_bytes(b, n, K))
    ws = torch.empty(wb, dtype=torch.uint8, device=pc.device)
    loss = torch.empty((b,), dtype=torch.float64, device=pc.device)
    grad = torch.empty_like(pc)
    _lib.check(lib.geoadv_knn_outlier_loss(0, b, n, K, ALPHA, _lib.ptr(pc), _lib.ptr(loss), _lib.ptr(grad), None, None, None, None,
                                           _lib.ptr(ws), wb, _lib.stream_handle()), "knn_outlier_loss")
    want = (loss.clone(), grad.clone())

    def f():
        _lib.check(lib.geoadv_debug_knn_outlier_loss_launch(b, n, K, ALPHA, _lib.ptr(pc), _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), wb,
                                                            _lib.stream_handle()), "debug_knn_outlier_loss_launch")
    f()
    assert torch.equal(loss, want[0]) and torch.equal(grad, want[1]), "the launch alone must repeat the call's bits"
    return f


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--windows", type=int, default=20)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "knn_loss_time.py measures on the GPU"
    assert a.windows >= 1 and a.calls >= 1
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    v = rng.normal(size=(max(BATCHES), N, 3))
    v = v / np.linalg.norm(v, axis=2, keepdims=True) * (1.0 + 0.02 * rng.normal(size=(max(BATCHES), N, 1)))
    clouds = torch.from_numpy(v.astype(np.float32)).to(dev)          # noisy unit spheres: a surface with a few points off it
    arms, side = {}, {}
    for b in BATCHES:
        pc = clouds[:b].contiguous()
        arms["op_b%d" % b] = lambda pc=pc: ops.knn_outlier_loss(pc, K, ALPHA)
        arms["launch_alone_b%d" % b] = launch_alone(pc)
        arms["torch_b%d" % b] = lambda pc=pc: torch_knn_loss(pc, K, ALPHA)
        # what the arms compute, side by side (not timed)
        loss, grad, _, mask, _, _ = ops.knn_outlier_loss(pc, K, ALPHA, return_parts=True)
        t_loss, t_grad = torch_knn_loss(pc, K, ALPHA)
        side["b%d" % b] = {"masked_per_cloud_mean": round(float(mask.sum(dim=1).float().mean().item()), 2),
                           "loss_largest_relative_difference_to_torch": float(((loss - t_loss.double()).abs() / loss).max().item()),
                           "grad_largest_difference_to_torch": float((grad - t_grad).abs().max().item()),
                           "grad_largest": float(grad.abs().max().item())}
    for f in arms.values():                                   # warm-up: code objects load, torch picks its algorithms
        window_ms(f, 10)
    runs = {name: [] for name in arms}
    for _ in range(a.windows):
        for name, f in arms.items():
            runs[name].append(window_ms(f, a.calls))
    out = {"what": "knn_loss_time", "n": N, "k": K, "alpha": ALPHA, "batches": list(BATCHES), "calls_per_window": a.calls,
           "windows": a.windows, "device": torch.cuda.get_device_name(0), "side_by_side": side}
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
