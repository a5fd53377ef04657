"""ms per AtlasNet training step (csrc/atlas_train.hip through AtlasNetTrainer) and the same step in torch eager fp32
autograd + torch.optim.Adam on the same GPU; prints one JSON line.

    python tools/atlas_train_time.py [--batch 32] [--points 2048] [--primitives 25] [--per-primitive 100] [--steps 20]
                                     [--warmup 3] [--repeats 3]

Both sides take the same template points (given, not drawn).  The eager side batches the primitives' decoders with
torch.bmm and finds Chamfer's nearest neighbours from the full distance matrix.  The per-kernel split comes from

    rocprofv3 --kernel-trace --stats -d <out> -o atlas -- python tools/atlas_train_time.py --steps 5 --step-only

bound_ms is the derived fp32-MFMA bound of the step's multiply-adds (forward, data and weight gradients, 155 TF/s).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geometric_adv_amd import atlas_weights as AW  # noqa: E402
from geometric_adv_amd.atlas_trainer import AtlasNetTrainer  # noqa: E402


def step_flops(B, n, nb, p, num_layers):
    macs = 3 * B * n * (3 * 64 + 64 * 128 + 128 * 1024) + 3 * B * 2 * 1024 * 1024
    macs += 3 * nb * B * p * (1024 * 512 + num_layers * 512 * 512 + 512 * 3) + 3 * nb * p * 2 * 1024
    return 2.0 * macs


def eager_step_fn(state, nb, num_layers, dbn, tmpl, dev):
    keys = AW.parameter_names(nb, num_layers, dbn)
    P = {k: torch.tensor(np.asarray(state[k], np.float32), device=dev) for k in keys if k.startswith("encoder.")}
    names = AW.dec_layers(num_layers)
    D = {}
    for name, fi, fo, bn in names:           # the primitives' decoders stacked: weights (nb, fi, fo), vectors (nb, 1, fo)
        D[name + ".weight"] = torch.tensor(np.stack([np.asarray(state["decoder.decoder.%d.%s.weight" % (q, name)]).reshape(fo, fi).T
                                                     for q in range(nb)]), device=dev)
        D[name + ".bias"] = torch.tensor(np.stack([state["decoder.decoder.%d.%s.bias" % (q, name)] for q in range(nb)])[:, None], device=dev)
        if bn and dbn:
            for f in ("weight", "bias", "running_mean", "running_var"):
                D[bn + "." + f] = torch.tensor(np.stack([state["decoder.decoder.%d.%s.%s" % (q, bn, f)] for q in range(nb)]).reshape(-1), device=dev)
    params = list(P.values()) + [v for k, v in D.items() if "running" not in k]
    for v in params:
        v.requires_grad_(True)
    run = {i: [torch.tensor(state["encoder.bn%d.running_%s" % (i, f)], device=dev) for f in ("mean", "var")] for i in range(1, 6)}
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.999))
    t = torch.tensor(tmpl, device=dev)

    def lin(x, k):
        w = P[k + ".weight"]
        return x @ w.reshape(w.shape[0], -1).t() + P[k + ".bias"]

    def bn(a, i):
        flat = a.reshape(-1, a.shape[-1])
        return F.batch_norm(flat, run[i][0], run[i][1], P["encoder.bn%d.weight" % i], P["encoder.bn%d.bias" % i], training=True,
                            momentum=0.1, eps=1e-5).reshape(a.shape)

    def dbn_(a, name):                       # a (nb, rows, C): statistics per primitive = per channel of (rows, nb * C)
        if not dbn:
            return a
        q, rows, C = a.shape
        flat = a.permute(1, 0, 2).reshape(rows, q * C)
        y = F.batch_norm(flat, D[name + ".running_mean"], D[name + ".running_var"], D[name + ".weight"], D[name + ".bias"], training=True,
                         momentum=0.1, eps=1e-5)
        return y.reshape(rows, q, C).permute(1, 0, 2)

    def step(x):
        B = x.shape[0]
        opt.zero_grad(set_to_none=True)
        h = torch.relu(bn(lin(x, "encoder.conv1"), 1))
        h = torch.relu(bn(lin(h, "encoder.conv2"), 2))
        h = bn(lin(h, "encoder.conv3"), 3).max(dim=1)[0]
        h = torch.relu(bn(lin(h, "encoder.lin1"), 4))
        z = torch.relu(bn(lin(h, "encoder.lin2"), 5))
        t1 = torch.bmm(t, D["conv1.weight"]) + D["conv1.bias"]                     # (nb, p, 1024)
        a = (t1[:, None] + z[None, :, None]).reshape(nb, -1, 1024)
        a = torch.relu(dbn_(a, "bn1"))
        for name, fi, fo, b in names[1:-1]:
            a = torch.relu(dbn_(torch.bmm(a, D[name + ".weight"]) + D[name + ".bias"], b))
        out = torch.bmm(a, D["last_conv.weight"]) + D["last_conv.bias"]            # (nb, B * p, 3)
        recon = out.reshape(nb, B, -1, 3).permute(1, 0, 2, 3).reshape(B, -1, 3)
        d = ((x[:, :, None, :] - recon[:, None, :, :]) ** 2).sum(-1)
        loss = d.min(2)[0].mean() + d.min(1)[0].mean()
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
    ap.add_argument("--primitives", type=int, default=25)
    ap.add_argument("--per-primitive", type=int, default=100)
    ap.add_argument("--num-layers", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--step-only", action="store_true", help="time nothing but the HIP step (for a kernel trace of the step alone)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n, nb, p, nl = a.batch, a.points, a.primitives, a.per_primitive, a.num_layers
    opt, state = AW.synthetic_state(nb, nl, True, seed=0, number_points_eval=max(4, min(p, 100)) * nb)
    opt["number_points"] = nb * p
    x = torch.tensor((np.random.default_rng(0).random((B, n, 3)) - 0.5).astype(np.float32), device=dev)
    tmpl = np.random.default_rng(1).random((nb, p, 2)).astype(np.float32)
    tr = AtlasNetTrainer(weights=state, options=opt, num_points=n, batch_size=B, seed=1)
    tr._template.copy_(torch.tensor(tmpl, device=dev))
    from geometric_adv_amd import _lib
    L = _lib.lib()

    def hip_step():            # the raw handle call with the template given: no host-side work in the timed loop
        _lib.check(L.geoadv_atlas_trainer_step(tr._h, _lib.ptr(x), 1, _lib.ptr(tr._template), None, _lib.stream_handle()), "step")

    out = {"batch": B, "points": n, "primitives": nb, "per_primitive": p, "steps": a.steps, "hip_ms": [], "eager_ms": []}
    if a.step_only:
        out["hip_ms"].append(round(timed(hip_step, a.steps, a.warmup), 3))
        print(json.dumps(out))
        return
    eager = None if a.no_eager else eager_step_fn(state, nb, nl, True, tmpl, dev)
    for _ in range(a.repeats):
        out["hip_ms"].append(round(timed(hip_step, a.steps, a.warmup), 3))
        if eager:
            out["eager_ms"].append(round(timed(lambda: eager(x), a.steps, a.warmup), 3))
    out["bound_ms"] = round(step_flops(B, n, nb, p, nl) / 155e12 * 1e3, 3)
    out["mfma_fraction"] = round(out["bound_ms"] / min(out["hip_ms"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
