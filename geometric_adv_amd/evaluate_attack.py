"""attacker/evaluate_attack.py on MI355X, without its plots: per attacked class, the distance weight of every attack that
minimises source_chamfer_dist + target_recon_error, the best target instance per target class (targeted attack) and the
best target class (untargeted attack), and the reference's text reports over all classes.

    python -m geometric_adv_amd.evaluate_attack --ae_folder log/autoencoder_victim --output_folder_name attack_res

Reads, per class under <eval>/<output_folder_name>/<class>/: adversarial_metrics.npy, adversarial_pc_input_dists.npy (written
by get_dists_per_point) and dist_weight.npy.  Writes, per class under .../<class>/analysis_results/:
  - source_target_norm_min_idx.npy                    [n_attacks] int64, the selected distance weight of every attack,
  - source_target_norm_min_per_target_class_idx.npy   [num_pc_for_attack, n_target_classes] int16,
  - source_target_norm_min_target_all_idx.npy         [num_pc_for_attack] int64,
and under <output_folder_name>/over_classes/: targeted_attacks.txt, untargeted_attacks.txt, eval_stats.txt in the reference's
line formats (src/adversary_utils.py:181-219 for the statistics).  The selection uses numpy's min / argmin on the same
dtypes as the reference, so ties go to the first index (the smaller distance weight, the earlier target).  A point is an
off-surface point ("#OS") when its distance to the source cloud exceeds 0.05, as in the reference.  numpy only: no GPU.

Differences forced by the environment:
  - the attack's settings come from <output_folder_name>/attack_configuration.json, written by run_attack (the reference
    unpickles a Configuration, which needs tflearn),
  - --save_graphs 1 and --save_pc_plots 1 are refused: they draw with matplotlib and seaborn, which this project does not use,
  - adversarial_pc_input.npy, adversarial_pc_recon.npy and the test-set clouds, which the reference loads for its plots
    only, are not read.
"""
import argparse
import json
import os
import os.path as osp
import time

import numpy as np

OUTLIER_THRESH = 0.05       # evaluate_attack.py:47


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--output_folder_name', type=str, default='attack_res')
    p.add_argument('--save_graphs', type=int, default=0)
    p.add_argument('--save_pc_plots', type=int, default=0)
    p.add_argument('--top_dir', type=str, default='.', help='root that --ae_folder / --attack_pc_idx are relative to')
    return p


def quantity_for_targeted_untargeted_attack(quantity, dist_weight_idx, targeted_idx, untargeted_idx):
    """src/adversary_utils.py:101-146: quantity [W, n_attacks] at the selected distance weight of every attack, reshaped to
    [num_pc_for_attack, n_attacks_per_instance]; at the best target per target class; at the best target class."""
    num_instance, num_target_classes = targeted_idx.shape
    per_instance = quantity.shape[1] // num_instance
    per_target = per_instance // num_target_classes
    at_weight = quantity[np.asarray(dist_weight_idx), np.arange(quantity.shape[1])].reshape(num_instance, per_instance)
    rows = np.arange(num_instance)[:, None]
    cols = np.arange(num_target_classes)[None, :] * per_target + targeted_idx
    targeted = at_weight[rows, cols]
    untargeted = at_weight[np.arange(num_instance), untargeted_idx * per_target + targeted_idx[np.arange(num_instance), untargeted_idx]]
    return at_weight, targeted, untargeted


def attack_line(attack_name, n_outlier, s_chamfer, t_chamfer, t_nre):
    spaces = ' ' * (40 - len(attack_name))
    return '%s%s#OS: %03d   S-CD: %.5f   T-RE: %.5f   T-NRE: %.2f\n' % (attack_name, spaces, n_outlier, s_chamfer, t_chamfer, t_nre)


def write_attack_statistics(fout, classes, norm_min, num_outlier, source_chamfer, target_chamfer, target_nre):
    """src/adversary_utils.py:181-219: per-class means (the lists are in the order the classes were evaluated, the labels
    in the order of the configuration's class names, as in the reference) and the means over classes."""
    fout.write('Shape\t\tAttack\t\tAdv\t\tAdv\t\tAdv\t\tAdv\n')
    fout.write('Class\t\tScore\t\t#OS\t\tS-CD\t\tT-RE\t\tT-NRE\n')
    fout.write('\n')
    line = '%s%s%.5f\t\t%03d\t\t%.5f\t\t%.5f\t\t%.2f\n'
    for c, name in enumerate(classes):
        fout.write(line % (name, ' ' * (16 - len(name)), norm_min[c].mean(), int(num_outlier[c].mean() + 0.5),
                           source_chamfer[c].mean(), target_chamfer[c].mean(), target_nre[c].mean()))
    fout.write('\n')
    name = 'over classes'
    fout.write(line % (name, ' ' * (16 - len(name)), np.vstack(norm_min).mean(), int(np.vstack(num_outlier).mean() + 0.5),
                       np.vstack(source_chamfer).mean(), np.vstack(target_chamfer).mean(), np.vstack(target_nre).mean()))


def main(argv=None):
    flags = build_parser().parse_args(argv)
    if flags.save_graphs or flags.save_pc_plots:
        raise SystemExit('evaluate_attack: --save_graphs and --save_pc_plots draw with matplotlib and seaborn, which this '
                         'project does not use; run with --save_graphs 0 --save_pc_plots 0')
    print('Evaluate attack flags:', flags)

    from .attack_data import create_dir, load_data

    data_path = osp.join(flags.top_dir, flags.ae_folder, 'eval')
    files = [f for f in os.listdir(data_path) if osp.isfile(osp.join(data_path, f))]
    output_path = create_dir(osp.join(data_path, flags.output_folder_name))
    with open(osp.join(output_path, 'attack_configuration.json')) as f:
        conf = json.load(f)
    pc_classes, ae_loss = load_data(data_path, files, ['pc_classes', 'ae_loss_test_set'])
    assert np.all(ae_loss > 0), 'Note: not all autoencoder loss values are larger than 0 as they should!'

    classes = list(conf['class_names'])
    num_instance = conf['num_pc_for_attack']
    num_pc_for_target = conf['num_pc_for_target']
    over_classes_dir = create_dir(osp.join(output_path, 'over_classes'))
    targeted = {k: [] for k in ('norm', 'os', 'scd', 'tre', 'tnre')}
    untargeted = {k: [] for k in ('norm', 'os', 'scd', 'tre', 'tnre')}
    with open(osp.join(over_classes_dir, 'targeted_attacks.txt'), 'w') as ftar, \
            open(osp.join(over_classes_dir, 'untargeted_attacks.txt'), 'w') as funtar:
        for i in range(len(pc_classes)):
            name = str(pc_classes[i])
            if name not in classes:
                continue
            print('evaluate shape class %s (%d out of %d classes) ' % (name, i + 1, len(pc_classes)))
            start = time.time()
            load_dir = osp.join(output_path, name)
            # adversarial metrics: loss_adv, loss_dist, source_chamfer_dist, target_nre, target_recon_error
            metrics = np.load(osp.join(load_dir, 'adversarial_metrics.npy'))
            dists = np.load(osp.join(load_dir, 'adversarial_pc_input_dists.npy'))
            num_dist_weight = len(np.load(osp.join(load_dir, 'dist_weight.npy')))
            assert metrics.shape[0] == num_dist_weight, 'adversarial_metrics has %d distance weights, dist_weight.npy %d' % (
                metrics.shape[0], num_dist_weight)
            save_dir = create_dir(osp.join(load_dir, 'analysis_results'))

            per_instance = metrics.shape[1] // num_instance
            target_class_name = [c for c in classes if c != name]
            num_target_classes = len(target_class_name)

            source_chamfer_dist = metrics[:, :, 2]
            target_nre = metrics[:, :, 3]
            target_recon_error = metrics[:, :, 4]
            num_outlier = np.sum(dists > OUTLIER_THRESH, axis=-1).astype(np.int16)

            # best distance weight per attack (minimal source Chamfer + target reconstruction error)
            norm = source_chamfer_dist + target_recon_error
            norm_min_val = np.min(norm, axis=0)
            norm_min_idx = np.argmin(norm, axis=0)
            np.save(osp.join(save_dir, 'source_target_norm_min_idx'), norm_min_idx)
            norm_min_reshape = norm_min_val.reshape([num_instance, per_instance])

            # best attack per source instance per target class (targeted attack)
            per_class_val = np.zeros([num_instance, num_target_classes], dtype=np.float32)
            per_class_idx = np.zeros([num_instance, num_target_classes], dtype=np.int16)
            for k in range(num_target_classes):
                window = norm_min_reshape[:, k * num_pc_for_target:(k + 1) * num_pc_for_target]
                per_class_val[:, k] = np.min(window, axis=1)
                per_class_idx[:, k] = np.argmin(window, axis=1)
            np.save(osp.join(save_dir, 'source_target_norm_min_per_target_class_idx'), per_class_idx)

            # best attack per source instance over all target classes (untargeted attack)
            all_val = np.min(per_class_val, axis=1)
            all_idx = np.argmin(per_class_val, axis=1)
            np.save(osp.join(save_dir, 'source_target_norm_min_target_all_idx'), all_idx)

            q = [quantity_for_targeted_untargeted_attack(x, norm_min_idx, per_class_idx, all_idx)
                 for x in (num_outlier, source_chamfer_dist, target_recon_error, target_nre)]
            for d, vals in ((targeted, [per_class_val] + [t[1] for t in q]), (untargeted, [all_val] + [t[2] for t in q])):
                for key, v in zip(('norm', 'os', 'scd', 'tre', 'tnre'), vals):
                    d[key].append(v)

            ftar.write('Shape class: %s\n' % name)
            ftar.write('--------------------------------------\n')
            for j in range(num_instance):
                for k in range(num_target_classes):
                    ftar.write(attack_line('adv_%s_%d_target_%s_%d' % (name, j, target_class_name[k], per_class_idx[j, k]),
                                           q[0][1][j, k], q[1][1][j, k], q[2][1][j, k], q[3][1][j, k]))
            ftar.write('\n')

            funtar.write('Shape class: %s\n' % name)
            funtar.write('--------------------------------------\n')
            for j in range(num_instance):
                c_idx = all_idx[j]
                funtar.write(attack_line('adv_%s_%d_target_%s_%d' % (name, j, target_class_name[c_idx], per_class_idx[j, c_idx]),
                                         q[0][2][j], q[1][2][j], q[2][2][j], q[3][2][j]))
            funtar.write('\n')
            print('Duration (minutes): %.2f' % ((time.time() - start) / 60.0))

    with open(osp.join(over_classes_dir, 'eval_stats.txt'), 'w') as fout:
        fout.write('Statistics for targeted attack\n')
        fout.write('--------------------------------------\n')
        write_attack_statistics(fout, classes, *[targeted[k] for k in ('norm', 'os', 'scd', 'tre', 'tnre')])
        fout.write('\n')
        fout.write('Statistics for untargeted attack\n')
        fout.write('--------------------------------------\n')
        write_attack_statistics(fout, classes, *[untargeted[k] for k in ('norm', 'os', 'scd', 'tre', 'tnre')])


if __name__ == '__main__':
    main()
