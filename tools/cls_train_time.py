"""ms per PointNet classifier training step (csrc/cls_train.hip through PointNetClassifierTrainer) and the same step in torch
eager fp32 autograd on the same GPU, at B = 32 x 2048 by default; prints one JSON line.

    python tools/cls_train_time.py [--batch 32] [--points 2048] [--steps 20] [--warmup 3]

The per-kernel split comes from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d <out> -o cls -- python tools/cls_train_time.py --steps 5 --no-eager

bound_ms is the derived fp32-MFMA bound of the direct form's multiply-adds (forward, data and weight gradients of every
layer, 155 TF/s), not a measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geometric_adv_amd import cls_weights as CW  # noqa: E402
from geometric_adv_amd.cls_trainer import PointNetClassifierTrainer  # noqa: E402


def direct_flops(B, N, nc):
    rows = {True: B * N, False: B}
    macs = 0
    for scope, fi, fo, bn, _ in CW.LAYERS:
        fo = nc if fo is None else fo
        point = scope.split("/")[-1].startswith(("tconv", "conv"))
        macs += 3 * rows[point] * fi * fo            # forward, data gradient, weight gradient
    macs += 3 * B * N * (3 * 3 + 64 * 64)           # u = x T1, v = h2 T2 and their gradients
    return 2.0 * macs


def eager_step_fn(w, nc, dev):
    P = {}
    for scope, fi, fo, bn, _ in CW.LAYERS:
        fo = nc if fo is None else fo
        names = [(scope + "/weights", (fi, fo)), (scope + "/biases", (fo,))]
        if bn:
            names += [(scope + "/bn/gamma", (fo,)), (scope + "/bn/beta", (fo,))]
        for n, shape in names:
            P[n] = torch.tensor(np.asarray(w[n], np.float32).reshape(shape), device=dev).requires_grad_(True)
    opt = torch.optim.Adam(P.values(), lr=1e-3, eps=1e-8)

    def lin(h, s):
        return h @ P[s + "/weights"] + P[s + "/biases"]

    def layer(h, s):
        a = lin(h, s)
        dims = tuple(range(a.dim() - 1))
        m = a.mean(dims)
        v = ((a - m) ** 2).mean(dims)
        return torch.relu((a - m) / torch.sqrt(v + 1e-3) * P[s + "/bn/gamma"] + P[s + "/bn/beta"])

    def tnet(h, p, k, last):
        g = layer(layer(layer(h, p + "/tconv1"), p + "/tconv2"), p + "/tconv3").max(dim=1)[0]
        g = layer(layer(g, p + "/tfc1"), p + "/tfc2")
        return (lin(g, p + "/" + last) + torch.eye(k, device=dev).reshape(-1)).reshape(-1, k, k)

    def step(x, y):
        t1 = tnet(x, "transform_net1", 3, "transform_XYZ")
        h2 = layer(layer(x @ t1, "conv1"), "conv2")
        t2 = tnet(h2, "transform_net2", 64, "transform_feat")
        g = layer(layer(layer(h2 @ t2, "conv3"), "conv4"), "conv5").max(dim=1)[0]
        g = torch.nn.functional.dropout(layer(g, "fc1"), 0.3)
        g = torch.nn.functional.dropout(layer(g, "fc2"), 0.3)
        e = t2 @ t2.transpose(1, 2) - torch.eye(64, device=dev)
        loss = torch.nn.functional.cross_entropy(lin(g, "fc3"), y) + 0.0005 * (e ** 2).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    return step


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    B, N, nc, dev = a.batch, a.points, a.classes, torch.device("cuda:0")
    rng = np.random.default_rng(0)
    x = torch.from_numpy((rng.random((B, N, 3)) - 0.5).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, nc, B)).to(dev)
    w = CW.synthetic_weights(nc, 0)
    tr = PointNetClassifierTrainer(weights=w, num_points=N, batch_size=B, num_classes=nc)
    ms = timed(lambda: tr.train_step(x, y), a.steps, a.warmup)
    flops = direct_flops(B, N, nc)
    out = {"batch": B, "points": N, "ms_per_step": ms, "gflop_direct": flops / 1e9, "bound_ms": flops / 155e12 * 1e3,
           "fraction_of_bound": flops / 155e12 * 1e3 / ms}
    if not a.no_eager:
        step = eager_step_fn(w, nc, dev)
        out["eager_ms_per_step"] = timed(lambda: step(x, y), a.steps, a.warmup)
        out["eager_over_hip"] = out["eager_ms_per_step"] / ms
    print(json.dumps(out))


if __name__ == "__main__":
    main()
