"""Writes tests/golden/atlas_augment.npz from the REFERENCE's own transfer/atlasnet/dataset/pointcloud_processor.py (TEST
INFRASTRUCTURE; needs a checkout of the reference project and runs on the CPU -- never on the GPU machines, where the tests
only read the fixture):

    python tools/make_golden_atlas_augment.py --reference <checkout of the reference project>

The reference's module is imported as it is (numpy and torch are all it needs).  torch is seeded, clouds of b = 4 are drawn,
and the DataAugmentation methods are called in the Augmenter's order (dataset/augmenter.py) with keep_track=True; the fp32
operators the reference drew are read back from operation.transforms[i].operator and laid out as the records of
geoadv_augment_batch (include/geoadv.h).  Data only:

  cases                          the names of the augmentation cases
  aug__<case>__cfg               [rot_axes, rot_3d, scale, flip_axes, translate] of the case (fields of geoadv_cloud_augment)
  aug__<case>__n<n>__in          the clouds (4, n, 3) fp32
  aug__<case>__n<n>__rec         the reference's operators (4, 45) fp32
  aug__<case>__n<n>__out         the reference's result (4, n, 3) fp32
  norm__<kind>__n<n>__{in,out}   Normalization.normalize_unitL2ball_functional / normalize_bounding_box_functional; at
                                 n = 7 and 64 the points of cloud 2 all coincide and cloud 3 holds one NaN coordinate (both come
                                 out all NaN), at n = 1 every cloud is one point (all NaN)

Every operator alone at n = 7, all of them together (axial rotations about 0, 1 and 2) at n = 1, 7 and 64.  While writing, the
float64 model of tests/_cloud_draws64.py is held against every recorded result: within BOUND_UNITS * 2^-24 * max|result| per
cloud, NaN in the same places (the bound of tests/test_cloud_prepare_host.py).
"""
import argparse
import importlib.util
import os.path as osp
import sys

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.join(ROOT, 'tests'))
import _cloud_draws64 as D  # noqa: E402

BOUND_UNITS = 8
B = 4
# name -> (rotation_axis, rotation_3D, anisotropic_scaling, flips, translation, the point counts)
CASES = {'axial0': ([0], False, False, [], False, (7,)), 'axial1': ([1], False, False, [], False, (7,)),
         'axial2': ([2], False, False, [], False, (7,)), 'rot3d': ([], True, False, [], False, (7,)),
         'scale': ([], False, True, [], False, (7,)), 'flip': ([], False, False, [0, 2], False, (7,)),
         'trans': ([], False, False, [], True, (7,)), 'all': ([0, 1, 2], True, True, [0, 2], True, (1, 7, 64))}


def load_reference(checkout):
    path = osp.join(checkout, 'transfer', 'atlasnet', 'dataset', 'pointcloud_processor.py')
    spec = importlib.util.spec_from_file_location('reference_pointcloud_processor', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def within_bound(model, got, what):
    assert np.array_equal(np.isnan(model), np.isnan(got)), what + ': NaN in different places'
    for c in range(got.shape[0]):
        if np.isnan(got[c]).any():
            continue
        err, unit = np.abs(model[c] - got[c]).max(), 2.0 ** -24 * np.abs(model[c]).max()
        assert err <= BOUND_UNITS * unit, '%s cloud %d: %.2f units' % (what, c, err / unit)
        print('%-28s cloud %d: %.2f units of 2^-24 max|result|' % (what, c, err / unit))


def augment_case(P, x, axes, rot3d, scale, flips, trans):
    """The Augmenter's __call__ with keep_track -> (record (b, 45), result (b, n, 3))."""
    op = P.DataAugmentation(x.clone(), keep_track=True)
    rec = np.stack([D.identity_record() for _ in range(x.shape[0])])
    t = 0
    for axis in axes:
        op.random_axial_rotation(axis=axis)
        rec[:, D.AXIAL + 9 * axis:D.AXIAL + 9 * axis + 9] = op.transforms[t].operator.numpy().reshape(-1, 9)
        t += 1
    if rot3d:
        op.random_rotation()
        rec[:, D.ROT3D:D.ROT3D + 9] = op.transforms[t].operator.numpy().reshape(-1, 9)
        t += 1
    if scale:
        op.random_anisotropic_scaling()
        rec[:, D.SCALE:D.SCALE + 3] = op.transforms[t].operator.numpy().reshape(-1, 3)
        t += 1
    if len(flips) > 0:
        op.random_flips(flips)
        rec[:, D.FLIP:D.FLIP + 3] = op.transforms[t].operator.numpy().reshape(-1, 3)
        t += 1
    if trans:
        op.random_translation()
        rec[:, D.TRANS:D.TRANS + 3] = op.transforms[t].operator.numpy().reshape(-1, 3)
        t += 1
    assert t == len(op.transforms) and rec.dtype == np.float32
    return rec, op.points.numpy().copy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ap.add_argument('--out', default=osp.join(ROOT, 'tests', 'golden', 'atlas_augment.npz'))
    a = ap.parse_args()
    P = load_reference(a.reference)
    torch.manual_seed(20191101)
    out = {'cases': np.array(sorted(CASES))}
    for name in sorted(CASES):
        axes, rot3d, scale, flips, trans, sizes = CASES[name]
        out['aug__%s__cfg' % name] = np.array([sum(1 << k for k in axes), int(rot3d), int(scale), sum(1 << k for k in flips), int(trans)], np.int32)
        for n in sizes:
            x = torch.rand(B, n, 3) - 0.5
            rec, res = augment_case(P, x, axes, rot3d, scale, flips, trans)
            model = np.stack([D.apply(x[c].numpy(), rec[c]) for c in range(B)])
            within_bound(model, res, 'aug %s n=%d' % (name, n))
            key = 'aug__%s__n%d__' % (name, n)
            out[key + 'in'], out[key + 'rec'], out[key + 'out'] = x.numpy().copy(), rec, res
    functional = {'UnitBall': P.Normalization.normalize_unitL2ball_functional, 'BoundingBox': P.Normalization.normalize_bounding_box_functional}
    for kind in sorted(functional):
        for n in (1, 7, 64):
            x = (torch.rand(B, n, 3) - 0.5) * torch.tensor([1.0, 0.6, 0.3]) + torch.tensor([0.2, -0.1, 0.05])
            if n > 1:
                x[2] = torch.tensor([0.25, -0.5, 0.125])      # few bits: the reference's fp32 mean of n copies is exact as well
                x[3, n // 2, 1] = float('nan')
            res = functional[kind](x).numpy().copy()
            model = np.stack([D.normalize64(x[c].numpy(), kind) for c in range(B)])
            within_bound(model, res, 'norm %s n=%d' % (kind, n))
            assert np.isnan(res[2]).all() and np.isnan(res[3]).all() and (n == 1 or not np.isnan(res[:2]).any())
            key = 'norm__%s__n%d__' % (kind, n)
            out[key + 'in'], out[key + 'out'] = x.numpy().copy(), res
    np.savez_compressed(a.out, **out)
    print('wrote', a.out, osp.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
