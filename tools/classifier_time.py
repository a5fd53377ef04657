"""Timing of the PointNet classifier forward (PointNetClassifier.logits: csrc/classifier.hip) at N = 2048 and
B in {1, 10, 32}, against a torch-eager fp32 version of the same graph on the same GPU.

    python tools/classifier_time.py [--batch 32 ...] [--reps 20] [--out classifier_time.json]

Per batch size: ms per call (device events around `reps` back-to-back calls, median of five windows after warm-up),
algorithmic GFLOP (2 x 434 569 multiply-adds per point, the graph's count with T1 / T2 folded into conv1 / conv3), and
the fraction of the 157.3 TFLOP/s fp32 matrix peak.  Kernel times come from a separate run of this script under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/classifier_time.py --batch 32`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import cls_weights as CW
from geometric_adv_amd.classifier import PointNetClassifier

MACS_PER_POINT = 434569
PEAK_TFLOPS = 157.3


def eager_model(w, dev):
    """The graph in torch eager fp32 (BN folded into scale / shift like the kernels; transforms as two bmm's)."""
    T = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)
    P = {}
    for scope, fi, fo, bn, _ in CW.LAYERS:
        W = T(w[scope + "/weights"]).reshape(fi, -1)
        b = T(w[scope + "/biases"])
        if bn:
            n = CW.bn_names(scope)
            inv = T(w[n["gamma"]]) * torch.rsqrt(T(w[n["var"]]) + CW.BN_EPS)
            P[scope] = (W, inv, b * inv + (T(w[n["beta"]]) - T(w[n["mean"]]) * inv))
        else:
            P[scope] = (W, None, b)
    eye3, eye64 = torch.eye(3, device=dev).flatten(), torch.eye(64, device=dev).flatten()

    def layer(x, s):
        W, sc, sh = P[s]
        return torch.relu(torch.matmul(x, W) * sc + sh)

    def lin(x, s, extra=0):
        W, _, b = P[s]
        return torch.matmul(x, W) + b + extra

    def tnet(x, p, last, eye, k):
        h = layer(layer(layer(x, p + "/tconv1"), p + "/tconv2"), p + "/tconv3").amax(dim=1)
        h = layer(layer(h, p + "/tfc1"), p + "/tfc2")
        return lin(h, p + "/" + last, eye).view(-1, k, k)

    def f(x):
        t1 = tnet(x, "transform_net1", "transform_XYZ", eye3, 3)
        h = layer(layer(torch.bmm(x, t1), "conv1"), "conv2")
        t2 = tnet(h, "transform_net2", "transform_feat", eye64, 64)
        h = layer(layer(layer(torch.bmm(h, t2), "conv3"), "conv4"), "conv5").amax(dim=1)
        return lin(layer(layer(h, "fc1"), "fc2"), "fc3")
    return f


def time_ms(f, reps):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ws = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            f()
        b.record()
        b.synchronize()
        ws.append(a.elapsed_time(b) / reps)
    return sorted(ws)[2]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, nargs="+", default=[1, 10, 32])
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--num_classes", type=int, default=13)
    p.add_argument("--no_eager", action="store_true", help="skip the torch-eager yardstick (kernel-trace runs)")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "classifier_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    w = CW.synthetic_weights(a.num_classes, seed=0)
    clf = PointNetClassifier(None, num_classes=a.num_classes, weights=w, device=dev)
    eager = eager_model(w, dev)
    rows = []
    for b in a.batch:
        x = torch.rand((b, a.n, 3), device=dev) - 0.5
        gflop = 2.0 * MACS_PER_POINT * b * a.n / 1e9
        ms = time_ms(lambda: clf.logits(x), a.reps)
        row = {"batch": b, "n": a.n, "ms": round(ms, 4), "gflop": round(gflop, 2),
               "frac_fp32_peak": round(gflop / (ms * 1e-3) / (PEAK_TFLOPS * 1e3), 3)}
        if not a.no_eager:
            with torch.no_grad():
                ems = time_ms(lambda: eager(x), max(2, a.reps // 4))
                ref = eager(x)
            got = clf.logits(x)
            row.update(eager_ms=round(ems, 4), speedup_vs_eager=round(ems / ms, 2),
                       max_abs_diff_vs_eager=float((got - ref).abs().max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
