"""Writes tests/golden/prepare_indices.npz from the REFERENCE's own attacker/prepare_indices_for_attack.py (TEST
INFRASTRUCTURE; needs a checkout of the reference project, run on a host that has one -- never on the GPU machines, where the
tests only read the .npz):

    python tools/make_golden_prepare_indices.py --reference <checkout of the reference project>

The script is read at run time and executed as it is with --get_rand_idx 1 --get_latent_nn_idx 1 and an ABSOLUTE --ae_folder
in a temporary directory (osp.join lets an absolute path win over the script's project directory).  src/general_utils.py
(get_dist_mat) and src/adversary_utils.py (load_data) are the reference's own modules, imported by path.  What the script
imports at its top but this host does not have, and these two stages never call, is replaced by stubs:
  - tensorflow, src.tf_utils.reset_tf_graph and external.structural_losses.tf_nndistance.nn_distance (the Chamfer stage),
  - seaborn (general_utils' plotting),
  - src.in_out.create_dir makes the folder.

The synthetic eval folder: n = 40 latent codes of d = 128 in 4 classes of 5, 17, 4 and 14 instances, rows at the scales 0.01,
1 and 30, and num_instance_per_class = 6, so that two classes are smaller than the request and padded with -1.  numpy's
default sort is unstable, so the generator asserts that the order is free of ties: no two latent rows are equal, and within
every row the distances inside each class segment are pairwise distinct.

Contents: the inputs (latent_vectors, slice_idx, pc_classes, num_instance_per_class) and the three arrays the reference
wrote (sel_idx_rand, latent_dist_mat, latent_nn_idx).
"""
import argparse
import os
import os.path as osp
import sys
import tempfile
import types

import numpy as np

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
PC_CLASSES = ['chair', 'table', 'car', 'lamp']
CLASS_SIZES = [5, 17, 4, 14]
BNECK = 128
NUM_INSTANCE_PER_CLASS = 6
SUFFIX = '4l.npy'
OUTPUTS = {'sel_idx_rand': 'sel_idx_rand_%d_test_set_%s' % (NUM_INSTANCE_PER_CLASS, SUFFIX),
           'latent_dist_mat': 'latent_dist_mat_test_set_' + SUFFIX, 'latent_nn_idx': 'latent_nn_idx_test_set_' + SUFFIX}


def synthetic_inputs(seed=11):
    """-> (latent_vectors [n, BNECK] float32 with rows of mixed scale, slice_idx [classes + 1])."""
    rng = np.random.default_rng(seed)
    n = sum(CLASS_SIZES)
    scale = np.array([0.01, 1.0, 30.0], np.float32)[rng.integers(0, 3, n)]
    latent = (rng.standard_normal((n, BNECK)).astype(np.float32) * scale[:, None]).astype(np.float32)
    return latent, np.concatenate([[0], np.cumsum(CLASS_SIZES)])


def write_eval_folder(ae_folder, latent, slice_idx, with_point_clouds=False):
    """The files prepare_indices_for_attack reads under <ae_folder>/eval (with_point_clouds: also the clouds, which the
    reference loads whatever the stage)."""
    ev = osp.join(ae_folder, 'eval')
    os.makedirs(ev, exist_ok=True)
    np.save(osp.join(ev, 'pc_classes_' + SUFFIX), np.array(PC_CLASSES))
    np.save(osp.join(ev, 'slice_idx_test_set_' + SUFFIX), slice_idx)
    np.save(osp.join(ev, 'latent_vectors_test_set_' + SUFFIX), latent)
    if with_point_clouds:
        np.save(osp.join(ev, 'point_clouds_test_set_' + SUFFIX), np.zeros((len(latent), 4, 3), np.float32))
    return ev


def _import_by_path(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _stubs(reference):
    def refuse(*args, **kwargs):
        raise RuntimeError('not part of the golden run')

    def module(name, package=False, **attrs):
        m = types.ModuleType(name)
        if package:
            m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    module('tensorflow', placeholder=refuse, Session=refuse, float32=None, reduce_mean=refuse)
    module('seaborn', heatmap=refuse)
    module('src', package=True)
    module('src.in_out', create_dir=lambda p: (os.makedirs(p, exist_ok=True), p)[1])
    module('src.tf_utils', reset_tf_graph=refuse)
    module('external', package=True)
    module('external.structural_losses', package=True)
    module('external.structural_losses.tf_nndistance', nn_distance=refuse)
    _import_by_path('src.general_utils', osp.join(reference, 'src', 'general_utils.py'))
    _import_by_path('src.adversary_utils', osp.join(reference, 'src', 'adversary_utils.py'))


def run_reference(reference, ae_folder):
    script = osp.join(reference, 'attacker', 'prepare_indices_for_attack.py')
    with open(script) as f:
        code = compile(f.read(), script, 'exec')
    argv, path = sys.argv, list(sys.path)
    sys.argv = [script, '--ae_folder', osp.abspath(ae_folder), '--get_rand_idx', '1', '--get_latent_nn_idx', '1',
                '--num_instance_per_class', '%d' % NUM_INSTANCE_PER_CLASS]
    try:
        exec(code, {'__name__': '__main__', '__file__': script})
    finally:
        sys.argv, sys.path[:] = argv, path


def assert_no_ties(latent, slice_idx, dist_mat):
    assert len(np.unique(latent, axis=0)) == len(latent), 'two latent rows are equal'
    for i in range(len(dist_mat)):
        for j in range(len(slice_idx) - 1):
            seg = dist_mat[i, slice_idx[j]:slice_idx[j + 1]]
            assert len(np.unique(seg)) == len(seg), 'row %d has equal distances inside class %d' % (i, j)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ap.add_argument('--out', default=osp.join(ROOT, 'tests', 'golden', 'prepare_indices.npz'))
    args = ap.parse_args()
    latent, slice_idx = synthetic_inputs()
    _stubs(args.reference)
    with tempfile.TemporaryDirectory() as top:
        ae_folder = osp.join(top, 'log', 'ae')
        ev = write_eval_folder(ae_folder, latent, slice_idx, with_point_clouds=True)
        before = set(os.listdir(ev))
        run_reference(args.reference, ae_folder)
        assert set(os.listdir(ev)) - before == set(OUTPUTS.values()), sorted(set(os.listdir(ev)) - before)
        arrays = {'latent_vectors': latent, 'slice_idx': slice_idx, 'pc_classes': np.array(PC_CLASSES),
                  'num_instance_per_class': np.array(NUM_INSTANCE_PER_CLASS)}
        for key, name in OUTPUTS.items():
            arrays[key] = np.load(osp.join(ev, name))
    assert_no_ties(latent, slice_idx, arrays['latent_dist_mat'])
    assert (arrays['sel_idx_rand'] == -1).sum(axis=1).tolist() == [max(0, NUM_INSTANCE_PER_CLASS - s) for s in CLASS_SIZES]
    np.savez_compressed(args.out, **arrays)
    print('wrote %s (%d bytes)' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
