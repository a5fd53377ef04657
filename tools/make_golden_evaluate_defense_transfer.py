"""Writes tests/golden/evaluate_defense_transfer.npz from the REFERENCE's own defender/evaluate_defense.py and
transfer/evaluate_transfer.py (TEST INFRASTRUCTURE; needs a checkout of the reference project, run on a host that has one --
never on the GPU machines, where the tests only read the .npz):

    python tools/make_golden_evaluate_defense_transfer.py --reference <checkout of the reference project>

Both scripts are read at run time and executed as they are (with plotting off), the way make_golden_evaluate_attack.py runs
attacker/evaluate_attack.py, with that tool's synthetic attack folder, stubs and runner.  One stub is added: the
Configuration that src.autoencoder.Configuration.load returns also answers exists_and_is_not_none, which evaluate_defense.py
asks of the defense configuration.

The synthetic tree: that tool's attack folder (four test-set classes of which three are attacked, three distance weights,
num_pc_for_attack 3, num_pc_for_target 2: 12 attacks per class), on which the reference's evaluate_attack.py runs first, and
  - the defense folders of DEFENSE_FOLDERS: a surface defense (num_knn_for_defense 2, knn_dist_thresh 0.04 in its
    configuration) whose defense_metrics.npy has leading dimension 1, as this project writes it, the same with leading
    dimension 3 (one entry per distance weight, as a reference-written folder may hold) and a critical defense without those
    two settings, each with its _orig twin holding defense_source_metrics.npy [n_attacks, 4],
  - the transfer folders of TRANSFER_FOLDERS under log/transfer_ae/eval: transfer_metrics.npy with leading dimension 1 and 3.
All metrics are random float32, different for every distance weight, so the weight selection shows in the texts.

Runs: every defense folder x --use_adversarial_data 1 / 0 x --use_params_for_stat_file_name 0 / 1 (over_classes/ is emptied
before each run, so a run's texts are exactly the files it wrote), and both transfer folders.

Contents: the inputs (class names, the attack and defense configurations as JSON strings, per class adversarial_metrics,
adversarial_pc_input_dists, defense_metrics, defense_source_metrics, transfer_metrics) and every written text under
'text__<run>__<file name>', where <run> is defense_run_key(...) or the transfer folder's name.
"""
import argparse
import json
import os
import os.path as osp
import shutil
import sys
import tempfile
import types

import numpy as np

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))
import make_golden_evaluate_attack as A  # noqa: E402

ROOT = A.ROOT
NUM_KNN_FOR_DEFENSE, KNN_DIST_THRESH = 2, 0.04
# folder name -> (leading dimension of defense_metrics, whether the configuration holds the surface defense's settings)
DEFENSE_FOLDERS = {'defense_surface_res': (1, True), 'defense_surface_per_weight_res': (3, True),
                   'defense_critical_res': (1, False)}
# folder name -> leading dimension of transfer_metrics
TRANSFER_FOLDERS = {'attack_res_transfer': 1, 'attack_res_transfer_per_weight': 3}
TRANSFER_AE_FOLDER = 'log/transfer_ae'
BASES = ('targeted_attacks', 'untargeted_attacks', 'eval_stats')
N_CRITICAL = 5


def n_attacks():
    return A.NUM_PC_FOR_ATTACK * (len(A.CLASS_NAMES) - 1) * A.NUM_PC_FOR_TARGET


def defense_conf(conf, surface):
    out = dict(conf)
    if surface:
        out.update(num_knn_for_defense=NUM_KNN_FOR_DEFENSE, knn_dist_thresh=KNN_DIST_THRESH)
    return out


def synthetic_metrics(seed=11):
    """-> (defense, transfer): defense[folder][class] = (defense_metrics [lead, n, 4], defense_source_metrics [n, 4]) and
    transfer[folder][class] = transfer_metrics [lead, n, 4], random float32."""
    rng = np.random.default_rng(seed)
    n = n_attacks()
    draw = lambda *shape: rng.random(shape).astype(np.float32)
    defense = {folder: {name: (draw(lead, n, 4), draw(n, 4)) for name in A.CLASS_NAMES}
               for folder, (lead, _) in DEFENSE_FOLDERS.items()}
    transfer = {folder: {name: draw(lead, n, 4) for name in A.CLASS_NAMES} for folder, lead in TRANSFER_FOLDERS.items()}
    return defense, transfer


def write_defense_folder(att, folder, def_conf, per_class, full=False):
    """<att>/<folder> and <att>/<folder>_orig as the defense commands leave them, with the files evaluate_defense reads
    (full=True: also the ones only the reference loads, for its plots)."""
    for name, (metrics, source_metrics) in per_class.items():
        lead, n = metrics.shape[:2]
        for out, files in ((osp.join(att, folder), {'defense_metrics': metrics}),
                           (osp.join(att, folder + '_orig'), {'defense_source_metrics': source_metrics})):
            os.makedirs(osp.join(out, name), exist_ok=True)
            with open(osp.join(out, 'defense_configuration.json'), 'w') as f:
                json.dump(def_conf, f)
            if full:
                first = (lead, n) if 'defense_metrics' in files else (n,)
                pre, cloud = ('adversarial', 'pc') if 'defense_metrics' in files else ('original', 'source')
                files = dict(files)
                files[pre + ('_critical_points' if pre == 'adversarial' else '_source_critical_points')] = \
                    np.zeros(first + (N_CRITICAL, 3), np.float32)
                files[pre + '_critical_idx'] = np.zeros(first + (N_CRITICAL,), np.int16)
                files[pre + '_critical_num'] = np.zeros(first, np.int16)
                files['defended_%s_input' % cloud] = np.zeros(first + (A.N_POINTS, 3), np.float32)
                files['defended_%s_recon' % cloud] = np.zeros(first + (A.N_POINTS, 3), np.float32)
            for base, a in files.items():
                np.save(osp.join(out, name, base + '.npy'), a)


def write_transfer_folder(top, folder, per_class, full=False):
    """<top>/log/transfer_ae/eval/<folder> as run_transfer leaves it (full=True: also transferred_pc_recon.npy)."""
    out = osp.join(top, TRANSFER_AE_FOLDER, 'eval', folder)
    for name, metrics in per_class.items():
        os.makedirs(osp.join(out, name), exist_ok=True)
        np.save(osp.join(out, name, 'transfer_metrics.npy'), metrics)
        if full:
            np.save(osp.join(out, name, 'transferred_pc_recon.npy'), np.zeros(metrics.shape[:2] + (A.N_POINTS, 3), np.float32))
    return out


def defense_runs():
    """(folder, use_adversarial_data, use_params_for_stat_file_name) of every recorded evaluate_defense run."""
    return [(folder, adv, params) for folder in DEFENSE_FOLDERS for adv in (1, 0) for params in (0, 1)]


def defense_run_key(folder, adv, params):
    return '%s__adv%d__params%d' % (folder, adv, params)


def defense_text_names(folder, params):
    """The file names a run leaves in over_classes/: the surface defense's settings show in them when asked for."""
    suffix = '_k_%d_th_%.2f' % (NUM_KNN_FOR_DEFENSE, KNN_DIST_THRESH) if params and DEFENSE_FOLDERS[folder][1] else ''
    return sorted(base + suffix + '.txt' for base in BASES)


def transfer_text_names():
    return sorted(base + '.txt' for base in BASES)


def defense_argv(folder, adv, params):
    return ['--ae_folder', 'log/ae', '--attack_pc_idx', 'log/ae/eval/sel_idx.npy', '--attack_folder', 'attack_res',
            '--output_folder_name', folder, '--use_adversarial_data', str(adv), '--use_params_for_stat_file_name', str(params)]


def transfer_argv(folder):
    return ['--transfer_ae_folder', TRANSFER_AE_FOLDER, '--ae_folder', 'log/ae', '--attack_pc_idx', 'log/ae/eval/sel_idx.npy',
            '--attack_folder', 'attack_res', '--output_folder_name', folder]


def _configuration_stub():
    """Replaces the Configuration of make_golden_evaluate_attack._stubs by one whose loaded object also answers
    exists_and_is_not_none."""
    class Loaded(types.SimpleNamespace):
        def exists_and_is_not_none(self, attribute):
            return getattr(self, attribute, None) is not None

    class Configuration(object):
        @staticmethod
        def load(path):
            with open(path + '.json') as f:
                return Loaded(**json.load(f))

    sys.modules['src.autoencoder'].Configuration = Configuration


def run_script(reference, top, relative, args):
    """Executes <reference>/<relative> as __main__ with `args`, its __file__ placed under `top` so that its top_out_dir is `top`."""
    script = osp.join(reference, relative)
    with open(script) as f:
        code = compile(f.read(), script, 'exec')
    argv = sys.argv
    sys.argv = [script] + list(args) + ['--save_graphs', '0', '--save_pc_plots', '0']
    try:
        exec(code, {'__name__': '__main__', '__file__': osp.join(top, relative)})
    finally:
        sys.argv = argv


def _texts(over_classes, run, want_names):
    got = sorted(os.listdir(over_classes))
    assert got == want_names, (run, got, want_names)
    out = {}
    for t in got:
        with open(osp.join(over_classes, t)) as f:
            out['text__%s__%s' % (run, t)] = np.array(f.read())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ap.add_argument('--out', default=osp.join(ROOT, 'tests', 'golden', 'evaluate_defense_transfer.npz'))
    args = ap.parse_args()
    conf, per_class = A.synthetic_inputs()
    defense, transfer = synthetic_metrics()
    A._stubs(args.reference)
    _configuration_stub()
    arrays = {'pc_classes': np.array(A.PC_CLASSES), 'conf_json': np.array(json.dumps(conf))}
    for name, (m, d) in per_class.items():
        arrays['adversarial_metrics__' + name] = m
        arrays['adversarial_pc_input_dists__' + name] = d
    with tempfile.TemporaryDirectory() as top:
        att = A.write_attack_folder(top, conf, per_class, full=True)
        A.run_reference(args.reference, top)
        for folder, (_, surface) in DEFENSE_FOLDERS.items():
            def_conf = defense_conf(conf, surface)
            arrays['defense_conf_json__' + folder] = np.array(json.dumps(def_conf))
            write_defense_folder(att, folder, def_conf, defense[folder], full=True)
            for name, (metrics, source_metrics) in defense[folder].items():
                arrays['defense_metrics__%s__%s' % (folder, name)] = metrics
                arrays['defense_source_metrics__%s__%s' % (folder, name)] = source_metrics
        for folder, adv, params in defense_runs():
            over_classes = osp.join(att, folder + ('' if adv else '_orig'), 'over_classes')
            shutil.rmtree(over_classes, ignore_errors=True)
            run_script(args.reference, top, osp.join('defender', 'evaluate_defense.py'), defense_argv(folder, adv, params))
            arrays.update(_texts(over_classes, defense_run_key(folder, adv, params), defense_text_names(folder, params)))
        for folder in TRANSFER_FOLDERS:
            out = write_transfer_folder(top, folder, transfer[folder], full=True)
            for name, metrics in transfer[folder].items():
                arrays['transfer_metrics__%s__%s' % (folder, name)] = metrics
            run_script(args.reference, top, osp.join('transfer', 'evaluate_transfer.py'), transfer_argv(folder))
            arrays.update(_texts(osp.join(out, 'over_classes'), folder, transfer_text_names()))
    np.savez_compressed(args.out, **arrays)
    print('wrote %s (%d bytes)' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
