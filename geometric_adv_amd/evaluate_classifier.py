"""classifier/evaluate_classifier.py on MI355X, without its plots: the accuracy tables of the semantic evaluation from the
*_pc_recon_pred.npy files run_classifier wrote -- per attacked class the classification correctness of every attack at its
selected distance weight, at the best target per target class (targeted attack) and at the best target class (untargeted
attack), and the reference's text reports over all classes.

    python -m geometric_adv_amd.evaluate_classifier --data_type adversarial --classification_type hit_target \
        --ae_folder log/autoencoder_victim --attack_folder attack_res --output_folder_name classifier_res

--data_type (folders as in run_classifier, under <eval>/<attack_folder>):
  - target:          <output_folder_name>_orig/<class>/target_pc_recon_pred.npy,
  - adversarial:     <output_folder_name>/<class>/adversarial_pc_recon_pred.npy,
  - source:          <defense_folder>/<output_folder_name>_orig/<class>/source_pc_recon_pred.npy,
  - before_defense:  <output_folder_name>/<class>/adversarial_pc_recon_pred.npy, reported under <defense_folder>/<output_folder_name>,
  - after_defense:   <defense_folder>/<output_folder_name>/<class>/defended_pc_recon_pred.npy when it exists, else
                     defended_source_recon_pred.npy.
--classification_type hit_target counts a prediction equal to the target's label, avoid_source one different from the
source's label (target and adversarial only; the defense types count predictions equal to the source's label).

Writes under <that folder>/over_classes/: targeted_attacks_*.txt, untargeted_attacks_*.txt and eval_stats_*.txt, named and
formatted as the reference's (src/adversary_utils.py:298-329 for the statistics).  numpy only: no GPU.

Differences forced by the environment:
  - the attack's settings come from <attack_folder>/attack_configuration.json, written by run_attack (the reference unpickles a
    Configuration, which needs tflearn),
  - --save_graphs 1 is refused: it draws with matplotlib and seaborn, which this project does not use,
  - the clouds, latent vectors, reconstructions and adversarial inputs, which the reference loads for its plots only, are not
    read.
"""
import argparse
import json
import os
import os.path as osp
import time

import numpy as np

DATA_TYPES = ('target', 'adversarial', 'source', 'before_defense', 'after_defense')
STATS_HEADER = {'target': ('Orig target recon', 'Target accuracy'), 'adversarial': ('Adv recon', 'Target accuracy'),
                'source': ('Orig source recon', 'Source accuracy'), 'before_defense': ('Adv recon', 'Source accuracy'),
                'after_defense': ('Def recon', 'Source accuracy')}


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--data_type', type=str, default='adversarial')
    p.add_argument('--classification_type', type=str, default='hit_target')
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--defense_folder', type=str, default='defense_critical_res')
    p.add_argument('--output_folder_name', type=str, default='classifier_res')
    p.add_argument('--save_graphs', type=int, default=0)
    p.add_argument('--top_dir', type=str, default='.', help='root that --ae_folder / --attack_pc_idx are relative to')
    return p


def file_suffix(data_type, classification_type):
    """evaluate_classifier.py:88-99, 287-294: what follows targeted_attacks / untargeted_attacks / eval_stats."""
    if data_type in ('before_defense', 'after_defense'):
        return '_' + data_type
    return '' if data_type == 'source' else '_' + classification_type


def write_classification_statistics(fout, classes, recon_cls_list, data_type):
    """src/adversary_utils.py:298-329: per-class mean accuracy (the list is in the order the classes were evaluated, the
    labels in the order of the configuration's class names, as in the reference) and the mean over classes."""
    fout.write('Shape\t\t%s\n' % STATS_HEADER[data_type][0])
    fout.write('Shape\t\t%s\n' % STATS_HEADER[data_type][1])
    fout.write('\n')
    for c, name in enumerate(classes):
        fout.write('%s%s%.4f\n' % (name, ' ' * (16 - len(name)), recon_cls_list[c].mean()))
    fout.write('\n')
    name = 'over classes'
    fout.write('%s%s%.4f\n' % (name, ' ' * (16 - len(name)), np.vstack(recon_cls_list).mean()))


def main(argv=None):
    flags = build_parser().parse_args(argv)
    if flags.save_graphs:
        raise SystemExit('evaluate_classifier: --save_graphs draws with matplotlib and seaborn, which this project does not '
                         'use; run with --save_graphs 0')
    print('Evaluate classifier flags:', flags)
    assert flags.data_type in DATA_TYPES, 'wrong data_type: %s.' % flags.data_type
    assert flags.classification_type in ['hit_target', 'avoid_source'], 'wrong classification_type: %s.' % flags.classification_type

    from .attack_data import create_dir, load_data, prepare_data_for_attack
    from .evaluate_attack import quantity_for_targeted_untargeted_attack

    data_path = osp.join(flags.top_dir, flags.ae_folder, 'eval')
    files = [f for f in os.listdir(data_path) if osp.isfile(osp.join(data_path, f))]
    attack_path = create_dir(osp.join(data_path, flags.attack_folder))
    adversarial_data_path = None
    if flags.data_type == 'target':
        output_path = create_dir(osp.join(attack_path, flags.output_folder_name + '_orig'))
    elif flags.data_type == 'adversarial':
        output_path = create_dir(osp.join(attack_path, flags.output_folder_name))
    elif flags.data_type == 'source':
        output_path = create_dir(osp.join(attack_path, flags.defense_folder, flags.output_folder_name + '_orig'))
    else:
        if flags.data_type == 'before_defense':
            adversarial_data_path = create_dir(osp.join(attack_path, flags.output_folder_name))
        output_path = create_dir(osp.join(attack_path, flags.defense_folder, flags.output_folder_name))

    with open(osp.join(attack_path, 'attack_configuration.json')) as f:
        conf = json.load(f)
    pc_classes, slice_idx, pc_labels = load_data(data_path, files, ['pc_classes', 'slice_idx_test_set', 'pc_label_test_set'])
    nn_idx_dict = {'latent_nn': 'latent_nn_idx_test_set', 'chamfer_nn_complete': 'chamfer_nn_idx_complete_test_set'}
    nn_idx = load_data(data_path, files, [nn_idx_dict[conf['target_pc_idx_type']]])
    correct_pred = None
    if conf['correct_pred_only']:
        pc_pred_labels = load_data(data_path, files, ['pc_pred_labels_test_set'])
        correct_pred = (pc_labels == pc_pred_labels)
    attack_pc_idx = np.load(osp.join(flags.top_dir, flags.attack_pc_idx))[:, :conf['num_pc_for_attack']]

    classes = list(conf['class_names'])
    suffix = file_suffix(flags.data_type, flags.classification_type)
    over_classes_dir = create_dir(osp.join(output_path, 'over_classes'))
    per_target_class_list, best_target_class_list = [], []
    with open(osp.join(over_classes_dir, 'targeted_attacks%s.txt' % suffix), 'w') as ftar, \
            open(osp.join(over_classes_dir, 'untargeted_attacks%s.txt' % suffix), 'w') as funtar:
        for i in range(len(pc_classes)):
            name = str(pc_classes[i])
            if name not in classes:
                continue
            print('evaluate shape class %s (%d out of %d classes) ' % (name, i + 1, len(pc_classes)))
            start = time.time()
            load_dir_attack = osp.join(attack_path, name)
            num_dist_weight = len(np.load(osp.join(load_dir_attack, 'dist_weight.npy')))
            analysis = osp.join(load_dir_attack, 'analysis_results')
            norm_min_idx = np.load(osp.join(analysis, 'source_target_norm_min_idx.npy'))
            per_class_idx = np.load(osp.join(analysis, 'source_target_norm_min_per_target_class_idx.npy'))
            all_idx = np.load(osp.join(analysis, 'source_target_norm_min_target_all_idx.npy'))

            source_pc_labels, target_pc_labels = prepare_data_for_attack(pc_classes, [pc_classes[i]], classes, pc_labels, slice_idx,
                                                                         attack_pc_idx, conf['num_pc_for_target'], nn_idx, correct_pred)
            source_pc_labels = source_pc_labels.reshape(-1)
            target_pc_labels = target_pc_labels.reshape(-1)
            load_dir = osp.join(output_path, name)

            if flags.data_type == 'target':
                pred = np.load(osp.join(load_dir, 'target_pc_recon_pred.npy'))
                if flags.classification_type == 'hit_target':
                    correct = np.equal(pred, target_pc_labels)
                else:
                    correct = np.not_equal(pred, source_pc_labels)
                correct = np.vstack([correct] * num_dist_weight)
            elif flags.data_type == 'adversarial':
                pred = np.load(osp.join(load_dir, 'adversarial_pc_recon_pred.npy'))
                if flags.classification_type == 'hit_target':
                    correct = np.equal(pred, np.vstack([target_pc_labels] * len(pred)))
                else:
                    correct = np.not_equal(pred, np.vstack([source_pc_labels] * len(pred)))
                correct = np.vstack([correct] * int(num_dist_weight / len(correct)))
            elif flags.data_type == 'source':
                pred = np.load(osp.join(load_dir, 'source_pc_recon_pred.npy'))
                correct = np.vstack([np.equal(pred, source_pc_labels)] * num_dist_weight)
            else:
                if flags.data_type == 'before_defense':
                    pred = np.load(osp.join(adversarial_data_path, name, 'adversarial_pc_recon_pred.npy'))
                elif osp.exists(osp.join(load_dir, 'defended_pc_recon_pred.npy')):
                    pred = np.load(osp.join(load_dir, 'defended_pc_recon_pred.npy'))             # defense on adversarial input
                else:
                    pred = np.expand_dims(np.load(osp.join(load_dir, 'defended_source_recon_pred.npy')), axis=0)   # on clean input
                correct = np.equal(pred, np.vstack([source_pc_labels] * len(pred)))
                correct = np.vstack([correct] * int(num_dist_weight / len(correct)))

            num_instance = conf['num_pc_for_attack']
            target_class_name = [c for c in classes if c != name]
            _, per_target_class, best = quantity_for_targeted_untargeted_attack(correct, norm_min_idx, per_class_idx, all_idx)
            per_target_class_list.append(per_target_class)
            best_target_class_list.append(best)

            ftar.write('Shape class: %s\n' % name)
            ftar.write('--------------------------------------\n')
            for j in range(num_instance):
                for k in range(len(target_class_name)):
                    attack_name = 'cls_%s_%d_target_%s_%d' % (name, j, target_class_name[k], per_class_idx[j, k])
                    ftar.write('%s%saccuracy: %.4f\n' % (attack_name, ' ' * (40 - len(attack_name)), per_target_class[j, k]))
            ftar.write('\n')

            funtar.write('Shape class: %s\n' % name)
            funtar.write('--------------------------------------\n')
            for j in range(num_instance):
                c_idx = all_idx[j]
                attack_name = 'cls_%s_%d_target_%s_%d' % (name, j, target_class_name[c_idx], per_class_idx[j, c_idx])
                funtar.write('%s%saccuracy: %.4f\n' % (attack_name, ' ' * (40 - len(attack_name)), best[j]))
            funtar.write('\n')
            print('Duration (minutes): %.2f' % ((time.time() - start) / 60.0))

    with open(osp.join(over_classes_dir, 'eval_stats%s.txt' % suffix), 'w') as fout:
        fout.write('Statistics for targeted attack\n')
        fout.write('--------------------------------------\n')
        write_classification_statistics(fout, classes, per_target_class_list, flags.data_type)
        fout.write('\n')
        fout.write('Statistics for untargeted attack\n')
        fout.write('--------------------------------------\n')
        write_classification_statistics(fout, classes, best_target_class_list, flags.data_type)


if __name__ == '__main__':
    main()
