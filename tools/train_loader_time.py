"""Timing of the loader in front of the training steps: host batches (in_out.PointCloudDataSet: the set reordered on the host every
epoch, every batch sliced there and uploaded) against resident clouds (device_data.DevicePointCloudDataSet: one
ops.batch_gather launch per batch), and the classifier's epoch with the jitter drawn on the host against --jitter_on_device.

    python tools/train_loader_time.py [--clouds 4000 30000] [--n 2048] [--batch 50] [--epochs 5] [--cls_clouds 1024]
                                      [--out profiles/train_loader_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/train_loader_time.py --kernel_only 200

AE rows: wall time of PointNetAETrainer._single_epoch_train (it ends in the loss's .item(), a device synchronisation) in ms per
epoch; one warm-up epoch per form, then `epochs` timed epochs per form, the two forms alternating epoch by epoch.  Reported:
the median, every epoch, and the spread (largest minus smallest epoch) of each form.  The same is done with Gaussian noise,
z rotation and denoising on the resident set (the work the reference does in numpy on the host is not rebuilt here).
Classifier rows: one epoch of train_classifier's loop (shuffle, jitter, train_step) over `cls_clouds` clouds at B = 32.
--kernel_only K: K launches of geoadv_batch_gather at batch x n with noise and rotation and nothing else, for a profiler run of
its own; the row also gives the launches' back-to-back time by device events."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from geometric_adv_amd import ops
from geometric_adv_amd.device_data import Augmentation, DevicePointCloudDataSet, rand_rotation_matrix
from geometric_adv_amd.in_out import PointCloudDataSet


def epoch_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(forms, epochs):
    """{name: f} -> {name: [ms per timed epoch]}: one warm-up call each, then the forms in turn, `epochs` times."""
    for f in forms.values():
        f()
    times = {k: [] for k in forms}
    for _ in range(epochs):
        for k, f in forms.items():
            times[k].append(epoch_ms(f))
    return times


def summary(times):
    out = {}
    for k, t in times.items():
        out[k + "_ms"] = round(float(np.median(t)), 3)
        out[k + "_ms_epochs"] = [round(x, 3) for x in t]
        out[k + "_spread_ms"] = round(max(t) - min(t), 3)
    return out


def ae_rows(a, dev):
    from geometric_adv_amd.trainer import PointNetAETrainer, initial_weights
    rows = []
    for clouds in a.clouds:
        rng = np.random.default_rng(0)
        pcs = (rng.random((clouds, a.n, 3), dtype=np.float32) - np.float32(0.5))
        np.random.seed(1)
        host, resident = PointCloudDataSet(pcs, copy=False), DevicePointCloudDataSet(pcs, device=dev)
        tr = PointNetAETrainer(initial_weights(a.n, seed=0), a.n, batch_size=a.batch, device=dev)
        augment = Augmentation(gauss_sigma=0.01, z_rotate=True, seed=0)
        forms = {"host_set": lambda: tr._single_epoch_train(host), "device_set": lambda: tr._single_epoch_train(resident),
                 "device_set_augmented": lambda: tr._single_epoch_train(resident, augment=augment, denoising=True)}
        row = {"what": "ae_epoch", "clouds": clouds, "n": a.n, "batch": a.batch, "steps": clouds // a.batch}
        row.update(summary(alternate(forms, a.epochs)))
        row["device_minus_host_ms"] = round(row["device_set_ms"] - row["host_set_ms"], 3)
        row["speedup"] = round(row["host_set_ms"] / row["device_set_ms"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del host, resident, tr, pcs
    return rows


def cls_row(a, dev):
    from geometric_adv_amd.cls_trainer import PointNetClassifierTrainer
    from geometric_adv_amd.train_classifier import jitter_point_cloud, shuffle_data
    B, N = 32, a.n
    rng = np.random.default_rng(0)
    data = (rng.random((a.cls_clouds, N, 3), dtype=np.float32) - np.float32(0.5))
    label = rng.integers(0, 13, a.cls_clouds)
    tr = PointNetClassifierTrainer(num_points=N, batch_size=B, num_classes=13, seed=0, device=dev)
    data_dev = torch.from_numpy(data).to(dev)
    steps = a.cls_clouds // B
    epoch = [0]

    def host_jitter():
        d, l, _ = shuffle_data(data, label)
        for bi in range(steps):
            tr.train_step(jitter_point_cloud(d[bi * B:(bi + 1) * B]).astype(np.float32), l[bi * B:(bi + 1) * B])

    def device_jitter():
        idx = np.arange(len(label))
        np.random.shuffle(idx)
        l = label[idx]
        for bi in range(steps):
            x = ops.batch_gather(data_dev, idx[bi * B:(bi + 1) * B], dict(seed=0, counter=epoch[0] * steps + bi, noise_sigma=0.01, noise_clip=0.05))
            tr.train_step(x, l[bi * B:(bi + 1) * B])
        epoch[0] += 1

    row = {"what": "classifier_epoch", "clouds": a.cls_clouds, "n": N, "batch": B, "steps": steps}
    row.update(summary(alternate({"host_jitter": host_jitter, "jitter_on_device": device_jitter}, a.epochs)))
    row["speedup"] = round(row["host_jitter_ms"] / row["jitter_on_device_ms"], 3)
    print(json.dumps(row), flush=True)
    return row


def kernel_row(a, dev):
    data = torch.rand((a.batch * 4, a.n, 3), device=dev) - 0.5
    index = np.random.default_rng(0).permutation(a.batch * 4)[:a.batch]
    rot = torch.from_numpy(rand_rotation_matrix(seed=0)).to(dev)
    idx = torch.from_numpy(index.astype(np.int32)).to(dev)
    aug = dict(seed=0, noise_sigma=0.01)
    for k in range(5):
        ops.batch_gather(data, idx, dict(aug, counter=k), rot, want_clean=True)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for k in range(a.kernel_only):
        ops.batch_gather(data, idx, dict(aug, counter=k), rot, want_clean=True)
    stop.record()
    torch.cuda.synchronize()
    moved = a.batch * a.n * 12
    row = {"what": "batch_gather_back_to_back", "batch": a.batch, "n": a.n, "launches": a.kernel_only,
           "us_per_call_incl_allocation_and_launch": round(start.elapsed_time(stop) * 1e3 / a.kernel_only, 3),
           "bytes_read": moved, "bytes_written": 2 * moved}
    print(json.dumps(row), flush=True)
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--clouds", type=int, nargs="+", default=[4000])
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--batch", type=int, default=50)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--cls_clouds", type=int, default=1024, help="0: skip the classifier row")
    p.add_argument("--kernel_only", type=int, default=0, help="K > 0: only K launches of the gather kernel (for a profiler run)")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "train_loader_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    if a.kernel_only > 0:
        rows = [kernel_row(a, dev)]
    else:
        rows = ae_rows(a, dev)
        if a.cls_clouds >= 32:
            rows.append(cls_row(a, dev))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
