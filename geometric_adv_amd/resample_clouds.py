"""Reduce point clouds to a fixed number of points by farthest point sampling on MI355X: the step in front of every model of
this package for clouds that are larger than the model's input (16 384-point scans, AtlasNet's denser ShapeNet clouds) or
that are not stored in farthest-point order, where taking the first N points is not a uniform subset.

    python -m geometric_adv_amd.resample_clouds --input clouds.npy --output clouds_2048.npy --n_points 2048

Reads a float array (k, n, 3) and writes (k, n_points, 3) float32: per cloud the start point, then n_points - 1 times the point
farthest from those chosen so far (ops.farthest_point_sample, csrc/sampling.hip; the rule is in include/geoadv.h).  The output
holds the input's bits, in farthest-point order; --n_points n reorders only, and every prefix of the result is then itself
a farthest-point sample.  --save_idx also writes the chosen indices (k, n_points) int32.

  --start first    every cloud starts at its point 0 (default)
  --start random   cloud i starts at np.random.RandomState(seed).randint(0, n, size=k)[i]

Clouds of more than 16 384 points are refused: one compute unit holds a cloud in registers, and that is its limit.
"""
import argparse

import numpy as np

MAX_POINTS = 16384      # ops.FPS_MAX_POINTS, repeated here so that a file is refused before torch or a device is touched


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--input', type=str, required=True, help='.npy file of clouds (k, n, 3)')
    p.add_argument('--output', type=str, required=True, help='.npy file to write: (k, n_points, 3) float32')
    p.add_argument('--n_points', type=int, required=True, help='points per output cloud, 1 <= n_points <= n')
    p.add_argument('--batch_size', type=int, default=64, help='clouds per launch')
    p.add_argument('--start', type=str, default='first', choices=['first', 'random'], help='the first point of every cloud')
    p.add_argument('--seed', type=int, default=0, help='seed of --start random')
    p.add_argument('--save_idx', type=str, default=None, help='.npy file to write the chosen indices to: (k, n_points) int32')
    p.add_argument('--device', type=str, default='cuda:0')
    return p


def load_clouds(path, n_points):
    """The clouds of `path` as float32 (k, n, 3); ValueError for a wrong shape, n beyond the limit or n_points outside [1, n]."""
    clouds = np.load(path)
    if clouds.ndim != 3 or clouds.shape[2] != 3 or clouds.dtype.kind != 'f':
        raise ValueError('%s: expected a float array of shape (k, n, 3), got %s of shape %s' % (path, clouds.dtype, clouds.shape))
    k, n, _ = clouds.shape
    if n > MAX_POINTS:
        raise ValueError('%s: clouds of %d points; farthest point sampling holds a cloud on one compute unit and is limited to '
                         '%d points per cloud' % (path, n, MAX_POINTS))
    if k < 1 or not 1 <= n_points <= n:
        raise ValueError('%s: --n_points %d for %d clouds of %d points; need at least one cloud and 1 <= n_points <= n' % (path, n_points, k, n))
    return np.ascontiguousarray(clouds, dtype=np.float32)


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Resample clouds flags:', flags)
    if flags.batch_size < 1:
        raise ValueError('--batch_size must be at least 1')
    clouds = load_clouds(flags.input, flags.n_points)
    k, n, _ = clouds.shape
    start = np.random.RandomState(flags.seed).randint(0, n, size=k) if flags.start == 'random' else np.zeros(k, dtype=np.int64)

    import torch
    from . import ops
    dev = torch.device(flags.device)
    out = np.empty((k, flags.n_points, 3), dtype=np.float32)
    idx = np.empty((k, flags.n_points), dtype=np.int32)
    for lo in range(0, k, flags.batch_size):
        hi = min(lo + flags.batch_size, k)
        batch = torch.from_numpy(clouds[lo:hi]).to(dev)
        i, pts = ops.farthest_point_sample(batch, flags.n_points, start=start[lo:hi], return_points=True)
        idx[lo:hi] = i.cpu().numpy()
        out[lo:hi] = pts.cpu().numpy()
    np.save(flags.output, out)
    if flags.save_idx:
        np.save(flags.save_idx, idx)
    print('%d clouds: %d -> %d points, written to %s' % (k, n, flags.n_points, flags.output))


if __name__ == '__main__':
    main()
