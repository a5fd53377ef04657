"""Writes tests/golden/classifier_eval.npz from the REFERENCE's own classifier/provider.py and classifier/evaluate_classifier.py
(TEST INFRASTRUCTURE; needs a checkout of the reference project, run on a host that has one -- never on the GPU machines,
where the tests only read the .npz):

    python tools/make_golden_classifier_eval.py --reference <checkout of the reference project>

(a) ROTATION.  classifier/provider.py (numpy only) is imported by path and its rotate_point_cloud_by_angle run on the clouds
of rotation_inputs() at ROTATION_ANGLES.  The largest cloud (1, 16384) draws its points, in random order, from a pool of 1021
distinct random points, so that the recorded arrays compress; the others are uniform in the unit cube, and the (3, 33) one
starts with zeros of both signs, tiny and huge coordinates.

(b) REPORTS.  evaluate_classifier.py is read at run time and executed as it is (with --save_graphs 0), with `__file__` placed
in a temporary top folder so that its top_out_dir is that folder.  src/general_utils.py and src/adversary_utils.py are the
reference's own modules, imported by path.  What they import but this host does not have is replaced by stubs:
  - seaborn and pandas (general_utils' plotting, never called),
  - src.autoencoder.Configuration.load reads <path>.json (the attack configuration, as run_attack writes it),
  - src.in_out.create_dir makes the folder.
The synthetic pipeline tree: three classes of four test clouds (8 points each), all attacked, num_pc_for_attack 2,
num_pc_for_target 2 (8 attacks per class), two distance weights, random predictions in the *_pc_recon_pred.npy files
run_classifier writes (class 'chair' has the defense-on-clean-input file defended_source_recon_pred.npy, the others
defended_pc_recon_pred.npy), and random analysis_results indices.  It is evaluated without and with correct_pred_only (the
predicted test-set labels leave class 'table' a single correctly predicted cloud, so target rows are padded; a few labels
differ from their slice's class, so that the choice of targets shows in the reports), for every data type, and for target / adversarial with both classification types: COMBOS.

Contents: rot_in__<b>x<n>, rot_out__<b>x<n>__<angle index>, rot_angles; the tree's input arrays under tree__<name>; and the
three text files of every run under text__<correct_pred_only>__<data_type>__<classification_type>__<file name>.
"""
import argparse
import json
import os
import os.path as osp
import sys
import tempfile
import types

import numpy as np

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))

# ---- (a) rotation ----------------------------------------------------------------------------------------------------
ROTATION_SHAPES = [(1, 1), (3, 33), (5, 64), (2, 100), (1, 16384)]
ROTATION_ANGLES = [0.0, 2 * np.pi / 3, 5 / float(12) * np.pi * 2, np.pi, 2 * np.pi + 0.7]


def rotation_inputs(seed=23):
    """{(b, n): float32 clouds (b, n, 3)}."""
    rng = np.random.default_rng(seed)
    out = {}
    for b, n in ROTATION_SHAPES:
        if n == 16384:
            pool = (rng.random((1021, 3)) - 0.5).astype(np.float32)
            x = pool[rng.integers(0, len(pool), (b, n))]
        else:
            x = (rng.random((b, n, 3)) - 0.5).astype(np.float32)
        if (b, n) == (3, 33):
            x[0, :6] = np.array([[0, 0, 0], [-0.0, 1, -0.0], [1e-30, -1e-30, 1e-38], [1e30, -1e30, 3e37], [1, 0, 0], [0, 0, -1]],
                                np.float32)
        out[(b, n)] = np.ascontiguousarray(x)
    return out


# ---- (b) the tiny pipeline tree ----------------------------------------------------------------------------------------
PC_CLASSES = ['chair', 'table', 'car']
PER_CLASS = 4
N_POINTS = 8
NUM_PC_FOR_ATTACK, NUM_PC_FOR_TARGET = 2, 2
DIST_WEIGHTS = [0.5, 1.0]
DEFENSE_FOLDER = 'defense_critical_res'
SUFFIX = '3l.npy'
COMBOS = [('target', 'hit_target'), ('target', 'avoid_source'), ('adversarial', 'hit_target'), ('adversarial', 'avoid_source'),
          ('source', 'hit_target'), ('before_defense', 'hit_target'), ('after_defense', 'hit_target')]


def synthetic_tree(seed=5):
    """{name: array} of everything evaluate_classifier reads from the tree that is not a constant."""
    rng = np.random.default_rng(seed)
    n_test, n_cls = PER_CLASS * len(PC_CLASSES), len(PC_CLASSES)
    n_att = NUM_PC_FOR_ATTACK * (n_cls - 1) * NUM_PC_FOR_TARGET
    # labels that are not all their slice's class, so that WHICH target is picked (what correct_pred_only changes) shows
    t = {'pc_label': np.array([0, 0, 0, 0, 1, 1, 0, 2, 2, 2, 1, 2], np.int8)}
    pred = t['pc_label'].copy()
    pred[[1, 4, 6, 7]] = [2, 0, 1, 1]               # chair: cloud 1 wrong; table: only cloud 1 right; car: all right
    t['pc_pred_labels'] = pred
    nn = np.zeros((n_test, n_test), np.int16)
    for r in range(n_test):
        for c in range(n_cls):
            nn[r, c * PER_CLASS:(c + 1) * PER_CLASS] = rng.permutation(PER_CLASS)
    t['nn_idx'] = nn
    t['sel_idx'] = np.stack([rng.permutation(PER_CLASS)[:NUM_PC_FOR_ATTACK + 1] for _ in range(n_cls)]).astype(np.int64)
    for name in PC_CLASSES:
        t['norm_min_idx__' + name] = rng.integers(0, len(DIST_WEIGHTS), n_att).astype(np.int64)
        t['per_target_class_idx__' + name] = rng.integers(0, NUM_PC_FOR_TARGET, (NUM_PC_FOR_ATTACK, n_cls - 1)).astype(np.int16)
        t['target_all_idx__' + name] = rng.integers(0, n_cls - 1, NUM_PC_FOR_ATTACK).astype(np.int64)
        for k in ('target_pred', 'adversarial_pred', 'source_pred', 'defended_pred'):
            t[k + '__' + name] = rng.integers(0, n_cls, (1, n_att)).astype(np.int8)
    return t


def write_tree(top, t, correct_pred_only, full=False):
    """The files evaluate_classifier reads under <top>/log/ae/eval (full=True: also the ones only the reference loads).
    Returns the attack folder."""
    ev = osp.join(top, 'log', 'ae', 'eval')
    att = osp.join(ev, 'attack_res')
    os.makedirs(att, exist_ok=True)
    n_test = PER_CLASS * len(PC_CLASSES)
    conf = {'class_names': PC_CLASSES, 'target_pc_idx_type': 'chamfer_nn_complete', 'num_pc_for_attack': NUM_PC_FOR_ATTACK,
            'num_pc_for_target': NUM_PC_FOR_TARGET, 'correct_pred_only': int(correct_pred_only), 'dist_weight_list': DIST_WEIGHTS}
    with open(osp.join(att, 'attack_configuration.json'), 'w') as f:
        json.dump(conf, f)
    np.save(osp.join(ev, 'pc_classes_' + SUFFIX), np.array(PC_CLASSES))
    np.save(osp.join(ev, 'slice_idx_test_set_' + SUFFIX), np.arange(0, n_test + 1, PER_CLASS))
    np.save(osp.join(ev, 'pc_label_test_set_' + SUFFIX), t['pc_label'])
    np.save(osp.join(ev, 'pc_pred_labels_test_set_' + SUFFIX), t['pc_pred_labels'])
    np.save(osp.join(ev, 'chamfer_nn_idx_complete_test_set_' + SUFFIX), t['nn_idx'])
    np.save(osp.join(ev, 'sel_idx.npy'), t['sel_idx'])
    if full:
        for base in ('point_clouds_test_set', 'reconstructions_test_set'):
            np.save(osp.join(ev, '%s_%s' % (base, SUFFIX)), np.zeros((n_test, N_POINTS, 3), np.float32))
        np.save(osp.join(ev, 'latent_vectors_test_set_' + SUFFIX), np.zeros((n_test, 4), np.float32))
    dfn = osp.join(att, DEFENSE_FOLDER)
    for name in PC_CLASSES:
        n_att = t['norm_min_idx__' + name].shape[0]
        for d in (osp.join(att, name, 'analysis_results'), osp.join(att, 'classifier_res_orig', name),
                  osp.join(att, 'classifier_res', name), osp.join(dfn, 'classifier_res_orig', name),
                  osp.join(dfn, 'classifier_res', name)):
            os.makedirs(d, exist_ok=True)
        np.save(osp.join(att, name, 'dist_weight.npy'), np.array(DIST_WEIGHTS))
        for key, base in (('norm_min_idx', 'source_target_norm_min_idx'),
                          ('per_target_class_idx', 'source_target_norm_min_per_target_class_idx'),
                          ('target_all_idx', 'source_target_norm_min_target_all_idx')):
            np.save(osp.join(att, name, 'analysis_results', base + '.npy'), t[key + '__' + name])
        if full:
            for base in ('adversarial_pc_input', 'adversarial_pc_recon'):
                np.save(osp.join(att, name, base + '.npy'), np.zeros((len(DIST_WEIGHTS), n_att, N_POINTS, 3), np.float32))
        np.save(osp.join(att, 'classifier_res_orig', name, 'target_pc_recon_pred.npy'), t['target_pred__' + name])
        np.save(osp.join(att, 'classifier_res', name, 'adversarial_pc_recon_pred.npy'), t['adversarial_pred__' + name])
        np.save(osp.join(dfn, 'classifier_res_orig', name, 'source_pc_recon_pred.npy'), t['source_pred__' + name])
        if name == PC_CLASSES[0]:                   # defense on clean input: [n]
            np.save(osp.join(dfn, 'classifier_res', name, 'defended_source_recon_pred.npy'), t['defended_pred__' + name][0])
        else:                                       # defense on adversarial input: [1, n]
            np.save(osp.join(dfn, 'classifier_res', name, 'defended_pc_recon_pred.npy'), t['defended_pred__' + name])
    return att


def report_dir(att, data_type):
    """<attack folder>/.../over_classes of a data type (evaluate_classifier.py:49-61)."""
    sub = {'target': 'classifier_res_orig', 'adversarial': 'classifier_res',
           'source': osp.join(DEFENSE_FOLDER, 'classifier_res_orig'), 'before_defense': osp.join(DEFENSE_FOLDER, 'classifier_res'),
           'after_defense': osp.join(DEFENSE_FOLDER, 'classifier_res')}[data_type]
    return osp.join(att, sub, 'over_classes')


def report_names(data_type, classification_type):
    if data_type in ('before_defense', 'after_defense'):
        s = '_' + data_type
    else:
        s = '' if data_type == 'source' else '_' + classification_type
    return ['targeted_attacks%s.txt' % s, 'untargeted_attacks%s.txt' % s, 'eval_stats%s.txt' % s]


def cli_args(data_type, classification_type):
    return ['--data_type', data_type, '--classification_type', classification_type, '--ae_folder', 'log/ae', '--attack_pc_idx',
            'log/ae/eval/sel_idx.npy', '--attack_folder', 'attack_res', '--defense_folder', DEFENSE_FOLDER,
            '--output_folder_name', 'classifier_res', '--save_graphs', '0']


def _import_by_path(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _stubs(reference):
    class Configuration(object):
        @staticmethod
        def load(path):
            with open(path + '.json') as f:
                return types.SimpleNamespace(**json.load(f))

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

    for absent in ('seaborn', 'pandas'):
        try:
            __import__(absent)
        except ImportError:
            module(absent, heatmap=refuse, DataFrame=refuse)
    module('src', package=True)
    module('src.autoencoder', Configuration=Configuration)
    module('src.in_out', create_dir=lambda p: (os.makedirs(p, exist_ok=True), p)[1])
    _import_by_path('src.general_utils', osp.join(reference, 'src', 'general_utils.py'))
    _import_by_path('src.adversary_utils', osp.join(reference, 'src', 'adversary_utils.py'))


def run_reference(reference, top, data_type, classification_type):
    script = osp.join(reference, 'classifier', 'evaluate_classifier.py')
    with open(script) as f:
        code = compile(f.read(), script, 'exec')
    argv, path = sys.argv, list(sys.path)
    sys.argv = [script] + cli_args(data_type, classification_type)
    try:
        exec(code, {'__name__': '__main__', '__file__': osp.join(top, 'classifier', 'evaluate_classifier.py')})
    finally:
        sys.argv, sys.path[:] = argv, path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ap.add_argument('--out', default=osp.join(ROOT, 'tests', 'golden', 'classifier_eval.npz'))
    args = ap.parse_args()
    arrays = {'rot_angles': np.array(ROTATION_ANGLES, np.float64)}

    provider = _import_by_path('_reference_provider', osp.join(args.reference, 'classifier', 'provider.py'))
    for (b, n), x in rotation_inputs().items():
        arrays['rot_in__%dx%d' % (b, n)] = x
        for k, angle in enumerate(ROTATION_ANGLES):
            y = provider.rotate_point_cloud_by_angle(x, angle)
            assert y.dtype == np.float32 and y.shape == x.shape
            arrays['rot_out__%dx%d__%d' % (b, n, k)] = y

    t = synthetic_tree()
    for k, v in t.items():
        arrays['tree__' + k] = v
    import matplotlib
    matplotlib.use('Agg')
    _stubs(args.reference)
    for cpo in (0, 1):
        for data_type, ctype in COMBOS:
            with tempfile.TemporaryDirectory() as top:
                att = write_tree(top, t, cpo, full=True)
                run_reference(args.reference, top, data_type, ctype)
                for name in report_names(data_type, ctype):
                    with open(osp.join(report_dir(att, data_type), name)) as f:
                        arrays['text__%d__%s__%s__%s' % (cpo, data_type, ctype, name)] = np.array(f.read())
    np.savez_compressed(args.out, **arrays)
    print('wrote %s (%d bytes)' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
