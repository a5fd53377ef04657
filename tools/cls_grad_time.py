"""MI355X: time of PointNetClassifier.input_gradient against torch eager fp32 autograd of the same graph, next to the forward.

    python tools/cls_grad_time.py [--out profiles/cls_grad_time.json] [--windows 10] [--calls 20]

Shapes 32 x 2048 and 10 x 2048, 13 classes, synthetic weights, cross-entropy loss.  Device events around `calls`
back-to-back calls per window; the arms (input_gradient, the forward, torch autograd, torch forward) alternate window by
window after a warm-up; median and spread = (max - min) / median per arm.  Each call includes its outputs' allocations."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EMA = "%s/bn/%s/bn/moments/%s/ExponentialMovingAverage"


class TorchGraph:
    """The inference graph in torch fp32 on the device (matmul, folded batch norm, relu, amax), differentiable in x."""

    def __init__(self, w, dev):
        self.p = {}
        for k in w:
            if k.endswith("/weights"):
                s = k[:-len("/weights")]
                W = torch.tensor(np.asarray(w[k], np.float32).reshape(-1, np.asarray(w[k]).shape[-1]), device=dev)
                b = torch.tensor(np.asarray(w[s + "/biases"], np.float32), device=dev)
                if s + "/bn/gamma" in w:
                    inv = np.asarray(w[s + "/bn/gamma"], np.float64) / np.sqrt(np.asarray(w[EMA % (s, s, "Squeeze_1")], np.float64) + 1e-3)
                    sh = np.asarray(w[s + "/bn/beta"], np.float64) - np.asarray(w[EMA % (s, s, "Squeeze")], np.float64) * inv
                    self.p[s] = (W, b, torch.tensor(inv.astype(np.float32), device=dev), torch.tensor(sh.astype(np.float32), device=dev))
                else:
                    self.p[s] = (W, b, None, None)

    def layer(self, h, s):
        W, b, inv, sh = self.p[s]
        a = h @ W + b
        return a if inv is None else torch.relu(a * inv + sh)

    def tnet(self, h, p, last, K):
        for s in ("tconv1", "tconv2", "tconv3"):
            h = self.layer(h, p + "/" + s)
        h = h.amax(dim=1)
        for s in ("tfc1", "tfc2"):
            h = self.layer(h, p + "/" + s)
        return (self.layer(h, p + "/" + last) + torch.eye(K, device=h.device).flatten()).view(-1, K, K)

    def logits(self, x):
        h = torch.bmm(x, self.tnet(x, "transform_net1", "transform_XYZ", 3))
        for s in ("conv1", "conv2"):
            h = self.layer(h, s)
        h = torch.bmm(h, self.tnet(h, "transform_net2", "transform_feat", 64))
        for s in ("conv3", "conv4", "conv5"):
            h = self.layer(h, s)
        h = h.amax(dim=1)
        for s in ("fc1", "fc2"):
            h = self.layer(h, s)
        return self.layer(h, "fc3")

    def input_gradient(self, x, y):
        x = x.detach().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(self.logits(x), y, reduction="none")
        return loss, torch.autograd.grad(loss.sum(), x)[0]


def window(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_grad_time.json"))
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    flags = ap.parse_args(argv)
    from geometric_adv_amd import cls_weights as CW
    from geometric_adv_amd.classifier import PointNetClassifier
    dev = torch.device("cuda:0")
    w = CW.synthetic_weights(13, seed=13)
    clf = PointNetClassifier(None, num_classes=13, weights=w)
    graph = TorchGraph(w, dev)
    result = dict(device=torch.cuda.get_device_name(0), windows=flags.windows, calls=flags.calls, shapes={})
    for b in (32, 10):
        x = torch.tensor((np.random.default_rng(b).random((b, 2048, 3)) - 0.5).astype(np.float32), device=dev)
        y32 = torch.tensor(np.random.default_rng(b + 1).integers(0, 13, b).astype(np.int32), device=dev)
        y64 = y32.to(torch.int64)
        arms = {"input_gradient": lambda: clf.input_gradient(x, y32, "xent"),
                "forward": lambda: clf.forward(x),
                "torch_autograd": lambda: graph.input_gradient(x, y64),
                "torch_forward": lambda: graph.logits(x)}
        g_op = clf.input_gradient(x, y32, "xent")[1]
        g_t = graph.input_gradient(x, y64)[1]
        agree = float((g_op - g_t).abs().amax() / g_t.abs().amax())
        for fn in arms.values():
            window(fn, 5)
        times = {k: [] for k in arms}
        for _ in range(flags.windows):
            for k, fn in arms.items():
                times[k].append(window(fn, flags.calls))
        shape = {"max_gradient_difference_to_torch_over_max_gradient": agree}
        for k, v in times.items():
            med = float(np.median(v))
            shape[k] = dict(median_ms=med, spread=float((max(v) - min(v)) / med), windows_ms=v)
        shape["input_gradient_over_torch_autograd"] = shape["input_gradient"]["median_ms"] / shape["torch_autograd"]["median_ms"]
        result["shapes"]["%dx2048" % b] = shape
        print(b, {k: (round(v["median_ms"], 4), round(v["spread"], 3)) for k, v in shape.items() if isinstance(v, dict)}, "agree", agree, flush=True)
    os.makedirs(os.path.dirname(flags.out), exist_ok=True)
    with open(flags.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
