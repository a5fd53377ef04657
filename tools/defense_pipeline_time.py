"""Wall time of the defense stage at full size on one GPU: evaluate_attack, get_knn_dists_per_point, run_defense_surface,
run_defense_critical and run_classifier (source, before_defense, after_defense) on a synthetic eval folder of 13 classes x
1500 attacks x 2048 points (num_pc_for_attack 25, num_pc_for_target 5, two distance weights), and the share of it spent in
np.load / np.save.

    python tools/defense_pipeline_time.py [--work DIR] [--out result.json]

The test-set clouds are noisy sphere shells (about 0.02 between neighbours, like ShapeNet shapes at 2048 points); an attack's
adversarial cloud is its source plus small noise with 20 of its points pushed off the surface.  The victim and the classifier
carry the repository's synthetic weights.  Writing the folder (about 2 GB) is not timed; the files it writes are still in the
page cache when the commands read them, so the I/O share is that of a warm cache.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_CLASSES, PER_CLASS, N = 13, 30, 2048
NUM_PC_FOR_ATTACK, NUM_PC_FOR_TARGET = 25, 5
DIST_WEIGHTS = [0.5, 1.0]


def _shells(rng, count):
    v = rng.standard_normal((count, N, 3)).astype(np.float32)
    v *= np.float32(0.45) / np.linalg.norm(v, axis=2, keepdims=True)
    return (v + rng.normal(0, 0.003, v.shape)).astype(np.float32)


def make_folder(top):
    from geometric_adv_amd import cls_weights as CW, weights as W
    from geometric_adv_amd.attack_data import prepare_data_for_attack
    from geometric_adv_amd.autoencoder import PointNetAE
    rng = np.random.default_rng(0)
    ev = os.path.join(top, 'log', 'ae', 'eval')
    att = os.path.join(ev, 'attack_res')
    os.makedirs(att)
    classes = np.array(['class%02d' % c for c in range(N_CLASSES)])
    slice_idx = np.arange(0, N_CLASSES * PER_CLASS + 1, PER_CLASS)
    pcs = _shells(rng, N_CLASSES * PER_CLASS)
    w = W.synthetic_weights(N)
    W.save_npz(os.path.join(top, 'log', 'ae', 'weights.npz'), w)
    ae = PointNetAE(w, N)
    nn_idx = np.stack([np.concatenate([rng.permutation(PER_CLASS) for _ in range(N_CLASSES)]) for _ in range(len(pcs))])
    attack_idx = np.stack([rng.permutation(PER_CLASS)[:NUM_PC_FOR_ATTACK] for _ in range(N_CLASSES)])
    for base, a in (('point_clouds_test_set', pcs), ('latent_vectors_test_set', ae.transform(pcs)),
                    ('reconstructions_test_set', ae.get_reconstructions(pcs)), ('ae_loss_test_set', ae.get_loss_per_pc(pcs)),
                    ('pc_classes', classes), ('slice_idx_test_set', slice_idx),
                    ('chamfer_nn_idx_complete_test_set', nn_idx.astype(np.int16)), ('sel_idx', attack_idx)):
        np.save(os.path.join(ev, base + '_13l.npy'), a)
    with open(os.path.join(att, 'attack_configuration.json'), 'w') as f:
        json.dump({'class_names': classes.tolist(), 'target_pc_idx_type': 'chamfer_nn_complete',
                   'num_pc_for_attack': NUM_PC_FOR_ATTACK, 'num_pc_for_target': NUM_PC_FOR_TARGET, 'correct_pred_only': 0,
                   'dist_weight_list': DIST_WEIGHTS, 'restore_epoch': 500}, f)
    for name in classes:
        d = os.path.join(att, name)
        os.makedirs(d)
        src, _ = prepare_data_for_attack(classes, [name], classes, pcs, slice_idx, attack_idx, NUM_PC_FOR_TARGET, nn_idx, None)
        adv = np.repeat(src[None], len(DIST_WEIGHTS), axis=0)
        adv += rng.normal(0, 0.002, adv.shape).astype(np.float32)
        adv[:, :, :20] *= np.float32(1.3)
        m = len(src)
        metrics = rng.random((len(DIST_WEIGHTS), m, 5)).astype(np.float32)
        np.save(os.path.join(d, 'adversarial_pc_input.npy'), adv)
        np.save(os.path.join(d, 'adversarial_pc_recon.npy'), adv)
        np.save(os.path.join(d, 'adversarial_metrics.npy'), metrics)
        np.save(os.path.join(d, 'adversarial_pc_input_dists.npy'), (rng.random((len(DIST_WEIGHTS), m, N)) * 0.06).astype(np.float32))
        np.save(os.path.join(d, 'dist_weight.npy'), np.array(DIST_WEIGHTS))
    cdir = os.path.join(top, 'log', 'pointnet')
    os.makedirs(cdir)
    CW.save_npz(os.path.join(cdir, 'weights.npz'), CW.synthetic_weights(13, seed=13))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--work', default=None, help='folder for the synthetic data (default: a temporary folder, removed)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from geometric_adv_amd import (evaluate_attack, get_knn_dists_per_point, run_classifier, run_defense_critical,
                                   run_defense_surface)
    top = tempfile.mkdtemp(dir=args.work)
    try:
        t0 = time.perf_counter()
        make_folder(top)
        setup_s = time.perf_counter() - t0
        io = {'s': 0.0}

        def timed_io(f):
            def g(*a, **k):
                t = time.perf_counter()
                try:
                    return f(*a, **k)
                finally:
                    io['s'] += time.perf_counter() - t
            return g
        np.load, np.save = timed_io(np.load), timed_io(np.save)
        base = ['--top_dir', top, '--ae_folder', 'log/ae', '--attack_pc_idx', 'log/ae/eval/sel_idx_13l.npy']
        cls = base + ['--classifier_folder', 'log/pointnet', '--num_points', str(N)]
        steps = [('evaluate_attack', evaluate_attack.main, base),
                 ('get_knn_dists_per_point', get_knn_dists_per_point.main, base),
                 ('run_defense_surface', run_defense_surface.main, base),
                 ('run_defense_critical', run_defense_critical.main, base),
                 ('run_classifier_source', run_classifier.main, cls + ['--data_type', 'source', '--defense_folder', 'defense_surface_res']),
                 ('run_classifier_before_defense', run_classifier.main,
                  cls + ['--data_type', 'before_defense', '--defense_folder', 'defense_surface_res']),
                 ('run_classifier_after_defense', run_classifier.main,
                  cls + ['--data_type', 'after_defense', '--defense_folder', 'defense_surface_res'])]
        res = {'classes': N_CLASSES, 'attacks_per_class': NUM_PC_FOR_ATTACK * (N_CLASSES - 1) * NUM_PC_FOR_TARGET, 'n_points': N,
               'dist_weights': len(DIST_WEIGHTS), 'setup_s': round(setup_s, 2), 'steps': {}}
        total = io_total = 0.0
        for name, f, argv in steps:
            io['s'] = 0.0
            t = time.perf_counter()
            f(argv)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            res['steps'][name] = {'wall_s': round(dt, 3), 'npy_io_s': round(io['s'], 3)}
            total += dt
            io_total += io['s']
        res.update(total_wall_s=round(total, 2), total_npy_io_s=round(io_total, 2), npy_io_share=round(io_total / total, 3))
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write(line + '\n')
    finally:
        shutil.rmtree(top, ignore_errors=True)


if __name__ == '__main__':
    main()
