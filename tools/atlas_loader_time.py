"""Timing of the loader in front of the AtlasNet training step: train_atlasnet's host path (every batch sliced out of a host
array and uploaded) against its device path (resident clouds, one ops.augment_batch launch per batch), without operators and
with all five, and the two new kernels alone.

    python tools/atlas_loader_time.py [--clouds 4000] [--n 2048] [--batch 32] [--epochs 3] [--launches 200]
                                      [--out profiles/atlas_loader_time.json]

Epoch rows: wall time of one pass of train_atlasnet's loop (shuffle, batch, AtlasNetTrainer.train_step, which ends in reading
the loss back: a device synchronisation per step) in ms per epoch; one warm-up epoch per form, then `epochs` timed epochs per
form, the forms alternating epoch by epoch.  Reported: the median, every epoch, and the spread (largest minus smallest epoch)
of each form.  Kernel rows: `launches` calls back to back between two device events, in us per call including the output's
allocation and the launch; three repetitions, the median and their spread."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import ops
from geometric_adv_amd.device_data import CloudAugmenter
from train_loader_time import alternate, summary

ALL_FIVE = dict(translation=True, rotation_axis=(1,), rotation_3D=True, anisotropic_scaling=True, flips=(0, 2))


def epoch_row(a, dev):
    from geometric_adv_amd.atlas_trainer import AtlasNetTrainer
    B = a.batch
    pcs = (np.random.default_rng(0).random((a.clouds, a.n, 3), dtype=np.float32) - np.float32(0.5))
    resident = ops.normalize_clouds(torch.from_numpy(pcs).to(dev), "UnitBall")
    pcs = resident.cpu().numpy()                       # the host path trains on the same clouds
    tr = AtlasNetTrainer(num_points=a.n, batch_size=B, seed=0, device=dev)
    rng = np.random.RandomState(0)

    def epoch(batch_of):
        order = rng.permutation(a.clouds)
        for s in range(0, a.clouds - B + 1, B):
            tr.train_step(batch_of(order[s:s + B]))

    plain, five = CloudAugmenter(seed=0), CloudAugmenter(seed=0, **ALL_FIVE)
    forms = {"host_path": lambda: epoch(lambda idx: pcs[idx]),
             "device_path": lambda: epoch(lambda idx: plain(resident, idx, counter=tr.counters()[1])),
             "device_path_five_operators": lambda: epoch(lambda idx: five(resident, idx, counter=tr.counters()[1]))}
    row = {"what": "atlasnet_epoch", "clouds": a.clouds, "n": a.n, "batch": B, "steps": a.clouds // B}
    row.update(summary(alternate(forms, a.epochs)))
    row["device_minus_host_ms"] = round(row["device_path_ms"] - row["host_path_ms"], 3)
    row["five_operators_minus_host_ms"] = round(row["device_path_five_operators_ms"] - row["host_path_ms"], 3)
    print(json.dumps(row), flush=True)
    return row


def back_to_back(f, launches, repeats=3):
    for k in range(5):
        f(k)
    us = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for k in range(launches):
            f(k)
        stop.record()
        torch.cuda.synchronize()
        us.append(start.elapsed_time(stop) * 1e3 / launches)
    return {"us_per_call_incl_allocation_and_launch": round(float(np.median(us)), 3), "us_per_call_runs": [round(u, 3) for u in us],
            "spread_us": round(max(us) - min(us), 3)}


def kernel_rows(a, dev):
    rows = []
    data = torch.rand((a.batch * 4, a.n, 3), device=dev) - 0.5
    idx = torch.from_numpy(np.random.default_rng(0).permutation(a.batch * 4)[:a.batch].astype(np.int32)).to(dev)
    five = CloudAugmenter(seed=0, **ALL_FIVE)
    for name, f in (("augment_batch_gather_only", lambda k: ops.augment_batch(data, idx)),
                    ("augment_batch_five_operators", lambda k: ops.augment_batch(data, idx, five.fields(k))),
                    ("augment_batch_five_operators_sampled", lambda k: ops.augment_batch(data, idx, dict(five.fields(k), sample=1)))):
        row = {"what": name, "batch": a.batch, "n": a.n, "launches": a.launches}
        row.update(back_to_back(f, a.launches))
        rows.append(row)
        print(json.dumps(row), flush=True)
    big = torch.rand((a.batch, 30000, 3), device=dev) - 0.5
    for kind in ("UnitBall", "BoundingBox"):
        for name, x in (("n%d" % a.n, data[:a.batch].contiguous()), ("n30000", big)):
            row = {"what": "normalize_clouds_%s_%s" % (kind, name), "batch": a.batch, "n": int(x.shape[1]), "launches": a.launches}
            row.update(back_to_back(lambda k: ops.normalize_clouds(x, kind), a.launches))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--clouds", type=int, default=4000)
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--epochs", type=int, default=3)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "atlas_loader_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    rows = [epoch_row(a, dev)] + kernel_rows(a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
