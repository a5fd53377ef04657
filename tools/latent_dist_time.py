"""The latent distance matrix of prepare_indices_for_attack --get_latent_nn_idx at the size of the real test set (n = 4379 codes
of d = 128): ops.latent_dist_matrix (GPU events around each launch, median of --reps launches after --warmup) and the whole GPU
path scorer.get_latent_dist_mat (host array in, host array out, wall clock) against the host form it replaces,
scorer.latent_dist_mat_host (wall clock, --host_reps runs), in one process; the two matrices are compared bit for bit.
One JSON line.  Not part of bench.py.

    python tools/latent_dist_time.py [--n 4379] [--d 128] [--reps 20] [--timeout 600]
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import ops
from geometric_adv_amd.scorer import get_latent_dist_mat, latent_dist_mat_host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4379)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host_reps", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=600, help="seconds after which the run gives up")
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.timeout, exit=True)
    assert torch.cuda.is_available(), "needs a GPU: there is no fallback"
    rng = np.random.default_rng(0)
    x = rng.standard_normal((args.n, args.d)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    for _ in range(args.warmup):
        out = ops.latent_dist_matrix(xd)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ops.latent_dist_matrix(xd)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    whole = []
    for _ in range(3):
        t0 = time.perf_counter()
        gpu = get_latent_dist_mat(x)
        whole.append(time.perf_counter() - t0)
    host_s = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        host = latent_dist_mat_host(x)
        host_s.append(time.perf_counter() - t0)
    kernel_ms = statistics.median(ms)
    flop = 3.0 * args.n * args.n * args.d
    print(json.dumps({"n": args.n, "d": args.d, "device": torch.cuda.get_device_name(0),
                      "kernel_ms_median": kernel_ms, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "reps": args.reps,
                      "kernel_fp32_TFLOPs": flop / kernel_ms / 1e9,
                      "gpu_path_host_to_host_s_median": statistics.median(whole),
                      "host_form_s_min": min(host_s), "host_form_s": host_s, "host_cpus": os.cpu_count(),
                      "bit_equal": bool(np.array_equal(gpu.view(np.uint32), host.view(np.uint32))),
                      "out_bit_equal": bool(np.array_equal(out.cpu().numpy().view(np.uint32), host.view(np.uint32)))}))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
