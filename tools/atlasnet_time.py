"""Timing of the AtlasNet auto-encoder forward (AtlasNetAE.forward: csrc/atlasnet.hip) at N = 2048, 25 x 100 SQUARE,
num_layers 2 and B in {1, 10, 32}, against a torch-eager fp32 version of the same graph on the same GPU.

    python tools/atlasnet_time.py [--batch 32 ...] [--reps 20] [--out atlasnet_time.json]

Per batch size: ms per call (device events around `reps` back-to-back calls, median of five windows after warm-up),
algorithmic GFLOP (encoder 2 n 139 456 + head 2 x 2 x 1024^2, decoder 2 P (dim 1024 + 1024 x 512 + num_layers 512^2 + 512 x 3)
per cloud) and the fraction of the 157.3 TFLOP/s fp32 matrix peak.  Kernel times come from a separate run of this script
under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/atlasnet_time.py --batch 32 --no_eager`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import atlas_weights as AW
from geometric_adv_amd.atlasnet import AtlasNetAE

PEAK_TFLOPS = 157.3


def gflop_per_cloud(n, P, num_layers, dim=2):
    enc = 2.0 * n * (3 * 64 + 64 * 128 + 128 * 1024) + 2.0 * 2 * 1024 * 1024
    dec = 2.0 * P * (dim * 1024 + 1024 * 512 + num_layers * 512 * 512 + 512 * 3)
    return (enc + dec) / 1e9


def eager_model(state, tmpl, num_layers, dev):
    """The graph in torch eager fp32: BN folded into scale / shift like the kernels, the per-point layers as matmuls, one
    decoder MLP per primitive (as the reference's module list runs them)."""
    T = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)

    def fold(w, b, bn):
        W = T(state[w]).reshape(T(state[w]).shape[0], -1).t().contiguous()
        if bn is None or (bn + ".weight") not in state:
            return W, None, T(state[b])
        inv = T(state[bn + ".weight"]) * torch.rsqrt(T(state[bn + ".running_var"]) + AW.BN_EPS)
        return W, inv, (T(state[b]) - T(state[bn + ".running_mean"])) * inv + T(state[bn + ".bias"])

    enc = [fold("encoder.%s.weight" % n, "encoder.%s.bias" % n, "encoder.bn%d" % (i + 1))
           for i, (n, _, _) in enumerate(AW.ENC_LAYERS)]
    decs = []
    for p in range(len(tmpl)):
        d = "decoder.decoder.%d." % p
        decs.append([fold(d + n + ".weight", d + n + ".bias", (d + bn) if bn else None)
                     for n, _, _, bn in AW.dec_layers(num_layers)])
    tt = T(tmpl)

    def apply(x, L, relu=True):
        W, sc, sh = L
        y = torch.matmul(x, W)
        y = y * sc + sh if sc is not None else y + sh
        return torch.relu(y) if relu else y

    def f(x):
        h = apply(apply(x, enc[0]), enc[1])
        h = apply(h, enc[2], relu=False).amax(dim=1)
        z = apply(apply(h, enc[3]), enc[4])
        outs = []
        for p, L in enumerate(decs):
            W, sc, sh = L[0]
            a = torch.matmul(tt[p], W)[None] + z[:, None, :]
            a = torch.relu(a * sc + sh) if sc is not None else torch.relu(a + sh)
            for l in L[1:-1]:
                a = apply(a, l)
            outs.append(apply(a, L[-1], relu=False))
        return z, torch.cat(outs, dim=1)
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
    p.add_argument("--nb_primitives", type=int, default=25)
    p.add_argument("--num_layers", type=int, default=2)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--no_eager", action="store_true", help="skip the torch-eager yardstick (kernel-trace runs)")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "atlasnet_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    opt, state = AW.synthetic_state(a.nb_primitives, a.num_layers, True, seed=0)
    ae = AtlasNetAE(options=opt, state=state, device=dev)
    eager = eager_model(state, ae.template, a.num_layers, dev)
    rows = []
    for b in a.batch:
        x = torch.rand((b, a.n, 3), device=dev) - 0.5
        gflop = b * gflop_per_cloud(a.n, ae.num_points, a.num_layers)
        ms = time_ms(lambda: ae.forward(x), a.reps)
        row = {"batch": b, "n": a.n, "points_out": ae.num_points, "ms": round(ms, 4), "gflop": round(gflop, 2),
               "frac_fp32_peak": round(gflop / (ms * 1e-3) / (PEAK_TFLOPS * 1e3), 3)}
        if not a.no_eager:
            with torch.no_grad():
                ems = time_ms(lambda: eager(x), max(2, a.reps // 4))
                ref = eager(x)[1]
            got = ae.forward(x)[1]
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
