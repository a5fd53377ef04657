"""Writes tests/golden/evaluate_attack.npz from the REFERENCE's own attacker/evaluate_attack.py (TEST INFRASTRUCTURE; needs a
checkout of the reference project, run on a host that has one -- never on the GPU machines, where the tests only read the
.npz):

    python tools/make_golden_evaluate_attack.py --reference <checkout of the reference project>

The script is read at run time and executed as it is (with plotting off), with `__file__` placed in a temporary top folder
so that its top_out_dir is that folder.  What it imports but this host does not have is replaced by stubs:
  - src.autoencoder.Configuration.load reads <path>.json (the attack configuration, as run_attack writes it),
  - src.in_out.create_dir makes the folder,
  - src.general_utils' plotting functions and matplotlib.pylab refuse to be called (the plots are off),
and src/adversary_utils.py (load_data, get_quantity_for_targeted_untargeted_attack, write_attack_statistics_to_file) is the
reference's own module, imported by path.

The synthetic attack folder: four test-set classes of which three are attacked (num_pc_for_attack 3, num_pc_for_target 2:
12 attacks per class), three distance weights, source Chamfer and target reconstruction error drawn from eighths so that
their sums tie exactly -- across distance weights, inside a target class's window and across target classes -- and the
per-point distances of get_dists_per_point drawn around the outlier threshold, some of them exactly float32(0.05).

Contents: the inputs (class names, attack configuration, per class adversarial_metrics, adversarial_pc_input_dists,
dist_weight), the three index arrays per class and the three text files of over_classes/.
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
PC_CLASSES = ['chair', 'table', 'car', 'lamp']
CLASS_NAMES = ['chair', 'table', 'car']
NUM_PC_FOR_ATTACK, NUM_PC_FOR_TARGET = 3, 2
DIST_WEIGHTS = [0.5, 1.0, 2.0]
N_POINTS = 16
PER_CLASS = 5
TEXTS = ('targeted_attacks.txt', 'untargeted_attacks.txt', 'eval_stats.txt')
INDEX_FILES = ('source_target_norm_min_idx', 'source_target_norm_min_per_target_class_idx',
               'source_target_norm_min_target_all_idx')


def synthetic_inputs(seed=7):
    """-> (conf, {class: (adversarial_metrics [W, n, 5] float32, adversarial_pc_input_dists [W, n, N] float32)})."""
    rng = np.random.default_rng(seed)
    conf = {'class_names': CLASS_NAMES, 'target_pc_idx_type': 'chamfer_nn_complete', 'num_pc_for_attack': NUM_PC_FOR_ATTACK,
            'num_pc_for_target': NUM_PC_FOR_TARGET, 'correct_pred_only': 0, 'dist_weight_list': DIST_WEIGHTS}
    n_att = NUM_PC_FOR_ATTACK * (len(CLASS_NAMES) - 1) * NUM_PC_FOR_TARGET
    out = {}
    for name in CLASS_NAMES:
        m = rng.random((len(DIST_WEIGHTS), n_att, 5)).astype(np.float32)
        m[:, :, 2] = rng.integers(1, 5, (len(DIST_WEIGHTS), n_att)) / np.float32(8)
        m[:, :, 4] = rng.integers(1, 5, (len(DIST_WEIGHTS), n_att)) / np.float32(8)
        m[:, :, 3] = m[:, :, 4] / np.float32(0.25)
        d = (rng.random((len(DIST_WEIGHTS), n_att, N_POINTS)) * 0.1).astype(np.float32)
        d[rng.random(d.shape) < 0.1] = np.float32(0.05)
        out[name] = (m, d)
    return conf, out


def write_attack_folder(top, conf, per_class, full=False):
    """The files evaluate_attack reads under <top>/log/ae/eval (full=True: also the ones only the reference loads)."""
    ev = osp.join(top, 'log', 'ae', 'eval')
    att = osp.join(ev, 'attack_res')
    os.makedirs(att, exist_ok=True)
    n_test = PER_CLASS * len(PC_CLASSES)
    np.save(osp.join(ev, 'pc_classes_4l.npy'), np.array(PC_CLASSES))
    np.save(osp.join(ev, 'ae_loss_test_set_4l.npy'), np.full(n_test, 0.25, np.float32))
    with open(osp.join(att, 'attack_configuration.json'), 'w') as f:
        json.dump(conf, f)
    if full:
        np.save(osp.join(ev, 'slice_idx_test_set_4l.npy'), np.arange(0, n_test + 1, PER_CLASS))
        for base in ('point_clouds_test_set', 'latent_vectors_test_set', 'reconstructions_test_set'):
            np.save(osp.join(ev, base + '_4l.npy'), np.zeros((n_test, 4, 3), np.float32))
        np.save(osp.join(ev, 'chamfer_nn_idx_complete_test_set_4l.npy'), np.zeros((n_test, n_test), np.int16))
        np.save(osp.join(ev, 'sel_idx.npy'), np.tile(np.arange(NUM_PC_FOR_ATTACK), (len(PC_CLASSES), 1)))
    for name, (m, d) in per_class.items():
        os.makedirs(osp.join(att, name), exist_ok=True)
        np.save(osp.join(att, name, 'adversarial_metrics.npy'), m)
        np.save(osp.join(att, name, 'adversarial_pc_input_dists.npy'), d)
        np.save(osp.join(att, name, 'dist_weight.npy'), np.array(conf['dist_weight_list']))
        if full:
            shape = d.shape + (3,)
            np.save(osp.join(att, name, 'adversarial_pc_input.npy'), np.zeros(shape, np.float32))
            np.save(osp.join(att, name, 'adversarial_pc_recon.npy'), np.zeros(shape, np.float32))
    return att


def _stubs(reference):
    class Configuration(object):
        @staticmethod
        def load(path):
            with open(path + '.json') as f:
                return types.SimpleNamespace(**json.load(f))

    def refuse(*args, **kwargs):
        raise RuntimeError('plotting is off in the golden run')

    src = types.ModuleType('src')
    src.__path__ = []
    autoencoder = types.ModuleType('src.autoencoder')
    autoencoder.Configuration = Configuration
    in_out = types.ModuleType('src.in_out')
    in_out.create_dir = lambda p: (os.makedirs(p, exist_ok=True), p)[1]
    general_utils = types.ModuleType('src.general_utils')
    general_utils.plot_3d_point_cloud = general_utils.plot_heatmap_graph = refuse
    mpl = types.ModuleType('matplotlib')
    mpl.__path__ = []
    pylab = types.ModuleType('matplotlib.pylab')
    pylab.figure = pylab.savefig = refuse
    mpl.pylab = pylab
    sys.modules.update({'src': src, 'src.autoencoder': autoencoder, 'src.in_out': in_out, 'src.general_utils': general_utils,
                        'matplotlib': mpl, 'matplotlib.pylab': pylab})
    import importlib.util
    spec = importlib.util.spec_from_file_location('src.adversary_utils', osp.join(reference, 'src', 'adversary_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['src.adversary_utils'] = mod
    spec.loader.exec_module(mod)


def run_reference(reference, top):
    script = osp.join(reference, 'attacker', 'evaluate_attack.py')
    with open(script) as f:
        code = compile(f.read(), script, 'exec')
    argv = sys.argv
    sys.argv = [script, '--ae_folder', 'log/ae', '--attack_pc_idx', 'log/ae/eval/sel_idx.npy', '--output_folder_name',
                'attack_res', '--save_graphs', '0', '--save_pc_plots', '0']
    try:
        exec(code, {'__name__': '__main__', '__file__': osp.join(top, 'attacker', 'evaluate_attack.py')})
    finally:
        sys.argv = argv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ap.add_argument('--out', default=osp.join(ROOT, 'tests', 'golden', 'evaluate_attack.npz'))
    args = ap.parse_args()
    conf, per_class = synthetic_inputs()
    _stubs(args.reference)
    with tempfile.TemporaryDirectory() as top:
        att = write_attack_folder(top, conf, per_class, full=True)
        run_reference(args.reference, top)
        arrays = {'pc_classes': np.array(PC_CLASSES), 'conf_json': np.array(json.dumps(conf))}
        for name, (m, d) in per_class.items():
            arrays['adversarial_metrics__' + name] = m
            arrays['adversarial_pc_input_dists__' + name] = d
            for base in INDEX_FILES:
                arrays[base + '__' + name] = np.load(osp.join(att, name, 'analysis_results', base + '.npy'))
        for t in TEXTS:
            with open(osp.join(att, 'over_classes', t)) as f:
                arrays[t] = np.array(f.read())
    np.savez_compressed(args.out, **arrays)
    print('wrote %s (%d bytes)' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
