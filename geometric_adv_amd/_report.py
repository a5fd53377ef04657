"""What evaluate_defense and evaluate_transfer share: both report four metric columns of every attack -- at the distance
weight, the target instance and the target class that evaluate_attack selected -- as one line per attack in
targeted_attacks.txt / untargeted_attacks.txt and as per-class and over-class means in eval_stats.txt.  numpy only.

Everything is read and every line is formed before the first file is opened for writing, so a refused run writes nothing.
"""
import json
import os
import os.path as osp

import numpy as np

from .evaluate_attack import quantity_for_targeted_untargeted_attack

INDEX_FILES = ('source_target_norm_min_idx', 'source_target_norm_min_per_target_class_idx',
               'source_target_norm_min_target_all_idx')
RULE = '--------------------------------------\n'


def refuse_plots(command, flags):
    """The wording of evaluate_attack's refusal."""
    if flags.save_graphs or flags.save_pc_plots:
        raise SystemExit('%s: --save_graphs and --save_pc_plots draw with matplotlib and seaborn, which this '
                         'project does not use; run with --save_graphs 0 --save_pc_plots 0' % command)


def load_attack(top_dir, ae_folder, attack_folder):
    """-> (attack path, attack configuration, class names of the test set); keeps the reference's ae_loss > 0 assertion."""
    from .attack_data import load_data
    data_path = osp.join(top_dir, ae_folder, 'eval')
    files = [f for f in os.listdir(data_path) if osp.isfile(osp.join(data_path, f))]
    attack_path = osp.join(data_path, attack_folder)
    with open(osp.join(attack_path, 'attack_configuration.json')) as f:
        conf = json.load(f)
    pc_classes, ae_loss = load_data(data_path, files, ['pc_classes', 'ae_loss_test_set'])
    assert np.all(ae_loss > 0), 'Note: not all autoencoder loss values are larger than 0 as they should!'
    return attack_path, conf, pc_classes


def over_weights(a, num_dist_weight):
    """evaluate_defense.py:143-148 / evaluate_transfer.py:122-123: an array with fewer leading entries than there are distance
    weights is stacked round(W / len) times ([1, m, 4], as this project writes it, W times; [W, m, 4] once)."""
    return np.vstack([a] * round(num_dist_weight / len(a)))


def metric_line(attack_name, labels, values):
    spaces = ' ' * (40 - len(attack_name))
    return '%s%s%s: %.5f   %s: %.2f   %s: %.5f   %s: %.2f\n' % (
        (attack_name, spaces) + tuple(x for pair in zip(labels, values) for x in pair))


def write_statistics(fout, heading, classes, columns):
    """src/adversary_utils.py:222-257 and :260-295, which differ in the two heading lines only: per-class means (the lists
    are in the order the classes were evaluated, the labels in the order of the configuration's class names, as in the
    reference) and the means over classes, on the arrays' own dtypes."""
    fout.write(heading[0])
    fout.write(heading[1])
    fout.write('\n')
    line = '%s%s%.5f\t\t%.2f\t\t%.5f\t\t%.2f\n'
    for c, name in enumerate(classes):
        fout.write(line % ((name, ' ' * (16 - len(name))) + tuple(col[c].mean() for col in columns)))
    fout.write('\n')
    name = 'over classes'
    fout.write(line % ((name, ' ' * (16 - len(name))) + tuple(np.vstack(col).mean() for col in columns)))


def report(attack_path, conf, pc_classes, metrics_of_class, targeted_line, untargeted_line, heading, over_classes_dir, names):
    """The per-class loop and the three texts.
      - metrics_of_class(name, num_dist_weight) -> [W, n_attacks, 4] metrics of an attacked class,
      - targeted_line / untargeted_line: (index into `names` of the text the lines go to, prefix of the attack's name, the
        four labels),
      - heading: the two heading lines of a statistics table,
      - names: file names of the targeted, untargeted and statistics texts under over_classes_dir."""
    classes = list(conf['class_names'])
    num_instance = conf['num_pc_for_attack']
    texts = ([], [])
    targeted = [[] for _ in range(4)]
    untargeted = [[] for _ in range(4)]
    for i in range(len(pc_classes)):
        name = str(pc_classes[i])
        if name not in classes:
            continue
        print('evaluate shape class %s (%d out of %d classes) ' % (name, i + 1, len(pc_classes)))
        load_dir = osp.join(attack_path, name)
        missing = [b for b in INDEX_FILES if not osp.exists(osp.join(load_dir, 'analysis_results', b + '.npy'))]
        if missing:
            raise SystemExit('%s is missing in %s: run geometric_adv_amd.evaluate_attack on the attack folder first'
                             % (', '.join(b + '.npy' for b in missing), osp.join(load_dir, 'analysis_results')))
        norm_min_idx, per_class_idx, all_idx = [np.load(osp.join(load_dir, 'analysis_results', b + '.npy'))
                                                for b in INDEX_FILES]
        num_dist_weight = len(np.load(osp.join(load_dir, 'dist_weight.npy')))
        metrics = metrics_of_class(name, num_dist_weight)
        target_class_name = [c for c in classes if c != name]
        q = [quantity_for_targeted_untargeted_attack(metrics[:, :, col], norm_min_idx, per_class_idx, all_idx)
             for col in range(4)]
        for col in range(4):
            targeted[col].append(q[col][1])
            untargeted[col].append(q[col][2])

        texts[0].append('Shape class: %s\n' % name)
        texts[0].append(RULE)
        where, prefix, labels = targeted_line
        for j in range(num_instance):
            for k in range(len(target_class_name)):
                attack_name = '%s_%s_%d_target_%s_%d' % (prefix, name, j, target_class_name[k], per_class_idx[j, k])
                texts[where].append(metric_line(attack_name, labels, [t[1][j, k] for t in q]))
        texts[0].append('\n')

        texts[1].append('Shape class: %s\n' % name)
        texts[1].append(RULE)
        where, prefix, labels = untargeted_line
        for j in range(num_instance):
            c_idx = all_idx[j]
            attack_name = '%s_%s_%d_target_%s_%d' % (prefix, name, j, target_class_name[c_idx], per_class_idx[j, c_idx])
            texts[where].append(metric_line(attack_name, labels, [t[2][j] for t in q]))
        texts[1].append('\n')

    os.makedirs(over_classes_dir, exist_ok=True)
    for text, file_name in zip(texts, names[:2]):
        with open(osp.join(over_classes_dir, file_name), 'w') as f:
            f.write(''.join(text))
    with open(osp.join(over_classes_dir, names[2]), 'w') as fout:
        fout.write('Statistics for targeted attack\n')
        fout.write(RULE)
        write_statistics(fout, heading, classes, targeted)
        fout.write('\n')
        fout.write('Statistics for untargeted attack\n')
        fout.write(RULE)
        write_statistics(fout, heading, classes, untargeted)
