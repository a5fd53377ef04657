"""ms per FoldingNet training step (csrc/fold_train.hip through FoldingNetTrainer) and the same step in torch eager fp32
autograd + torch.optim.Adam on the same GPU; prints one JSON line.

    python tools/fold_train_time.py [--batch 8] [--points 2048] [--steps 20] [--warmup 3] [--repeats 3]

Both sides run the same graph with the picks given: the eager side takes cov and the neighbour columns of the HIP step and
excludes graph building; hip_ms includes geoadv's graph build (kNN, covariance, CSR, picks), hip_graph_ms is that part alone
(timed through FoldingNetAE.graph, the same kernels as the step's own build without its pick kernel: hip_ms - hip_graph_ms
compares with eager_ms on the assumption that the two builds cost the same).  The per-kernel split comes from

    rocprofv3 --kernel-trace --stats -d <out> -o fold -- python tools/fold_train_time.py --steps 5 --step-only

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
from geometric_adv_amd import fold_weights as FW  # noqa: E402
from geometric_adv_amd.fold_trainer import FoldingNetTrainer, LAYERS  # noqa: E402

G2 = FW.GRID * FW.GRID


def step_flops(B, n):
    macs = 0
    for pre, fi, fo, conv, bn in LAYERS:
        if pre.startswith("decoder"):
            rows = B * G2
            if pre.endswith("conv1"):                 # the code rows act once per cloud
                macs += 3 * (B * 512 * fo + rows * (fi - 512) * fo)
                continue
        else:
            rows = B * n if conv else B
        macs += 3 * rows * fi * fo
    return 2.0 * macs


def eager_step_fn(state, cov, cols, dev):
    P = {k: torch.tensor(np.asarray(state[k], np.float32), device=dev).requires_grad_(True) for k in FW.parameter_names()}
    run = {i: [torch.tensor(state["encoder.bn%d.running_%s" % (i, f)], device=dev) for f in ("mean", "var")] for i in range(1, 7)}
    opt = torch.optim.Adam(P.values(), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-6)
    B, n = cov.shape[:2]
    ar = torch.arange(B, device=dev)[:, None, None]
    c = [cols[0].long(), cols[1].long()]
    grid = torch.tensor(FW.grid(), device=dev)[None].expand(B, G2, 2)

    def lin(x, k):
        w = P[k + ".weight"]
        return x @ w.reshape(w.shape[0], -1).t() + P[k + ".bias"]

    def bn(a, i):
        flat = a.reshape(-1, a.shape[-1])
        return F.batch_norm(flat, run[i][0], run[i][1], P["encoder.bn%d.weight" % i], P["encoder.bn%d.bias" % i], training=True,
                            momentum=0.1, eps=1e-5).reshape(a.shape)

    def pool(h, p):
        return torch.relu(torch.max(h[ar, c[p]].max(dim=2)[0], h))

    def step(x):
        opt.zero_grad(set_to_none=True)
        h = torch.cat([x, cov], 2)
        for i in (1, 2, 3):
            h = torch.relu(bn(lin(h, "encoder.conv%d" % i), i))
        h = torch.relu(bn(lin(pool(h, 0), "encoder.conv4"), 4))
        h = bn(lin(pool(h, 1), "encoder.conv5"), 5).max(dim=1)[0]
        code = lin(torch.relu(bn(lin(h, "encoder.fc1"), 6)), "encoder.fc2")
        rep = code[:, None, :].expand(B, G2, 512)
        a = torch.relu(lin(torch.relu(lin(torch.cat([rep, grid], 2), "decoder.fold1.conv1")), "decoder.fold1.conv2"))
        mid = lin(a, "decoder.fold1.conv3")
        a = torch.relu(lin(torch.relu(lin(torch.cat([rep, mid], 2), "decoder.fold2.conv1")), "decoder.fold2.conv2"))
        recon = lin(a, "decoder.fold2.conv3")
        d = ((x[:, :, None, :] - recon[:, None, :, :]) ** 2).sum(-1)
        loss = (d.min(2)[0].mean(1) + d.min(1)[0].mean(1)).mean()
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--step-only", action="store_true", help="time nothing but the HIP step (for a kernel trace of the step alone)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n = a.batch, a.points
    state = FW.synthetic_state(0)
    x = torch.tensor((np.random.default_rng(0).random((B, n, 3)) - 0.5).astype(np.float32), device=dev)
    tr = FoldingNetTrainer(weights=state, num_points=n, batch_size=B, seed=1)
    tr.train_step(x)
    picks = tr.state("picks")
    cov, cols = torch.tensor(tr.state("cov"), device=dev), torch.tensor(tr.state("cols"), device=dev)
    pk = torch.tensor(picks, device=dev)
    tr._picks.copy_(pk)
    from geometric_adv_amd import _lib
    L = _lib.lib()

    def hip_step():            # the raw handle call with the picks given: no host-side validation in the timed loop
        _lib.check(L.geoadv_fold_trainer_step(tr._h, _lib.ptr(x), 0, _lib.ptr(tr._picks), None, None, _lib.stream_handle()), "step")

    ae = tr.eval_model()
    out = {"batch": B, "points": n, "steps": a.steps, "hip_ms": [], "hip_graph_ms": [], "eager_ms": []}
    eager = None if a.no_eager else eager_step_fn(state, cov, cols, dev)
    if a.step_only:
        out["hip_ms"].append(round(timed(hip_step, a.steps, a.warmup), 3))
        print(json.dumps(out))
        return
    for _ in range(a.repeats):
        out["hip_ms"].append(round(timed(hip_step, a.steps, a.warmup), 3))
        out["hip_graph_ms"].append(round(timed(lambda: ae.graph(x), a.steps, a.warmup), 3))
        if eager:
            out["eager_ms"].append(round(timed(lambda: eager(x), a.steps, a.warmup), 3))
    out["bound_ms"] = round(step_flops(B, n) / 155e12 * 1e3, 3)
    out["gflop_per_cloud"] = round(step_flops(B, n) / B / 1e9, 2)
    out["mfma_fraction"] = round(out["bound_ms"] / (min(out["hip_ms"]) - min(out["hip_graph_ms"])), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
