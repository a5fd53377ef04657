"""classifier/run_classifier.py on MI355X: the reference's flags and per-class output files for every --data_type, with the
PointNet classifier running as HIP kernels (classifier.py).

    python -m geometric_adv_amd.run_classifier --data_type adversarial --ae_folder log/autoencoder_victim ...

--data_type (the folders are those of the reference, under <eval>/<attack_folder>):
  - target:          the targets' reconstructions (reconstructions_test_set) -> <output_folder_name>_orig/<class>/target_pc_recon_pred.npy,
  - adversarial:     adversarial_pc_recon at the selected distance weight -> <output_folder_name>/<class>/adversarial_pc_recon_pred.npy,
  - source:          the sources' reconstructions -> <defense_folder>/<output_folder_name>_orig/<class>/source_pc_recon_pred.npy,
  - before_defense:  as adversarial, written under <defense_folder>/<output_folder_name>,
  - after_defense:   <defense_folder>/<class>/defended_pc_recon.npy when it exists (defended_pc_recon_pred.npy [1, n]), else
                     defended_source_recon.npy (defended_source_recon_pred.npy [n]) -- so --defense_folder may name a defense
                     output folder or its _orig twin; both are written by run_defense_surface / run_defense_critical.

Differences forced by the environment:
  - configurations are JSON: the attack's is read from <eval>/<attack_folder>/attack_configuration.json (written by run_attack),
    a defense's from defense_configuration.json where the reference reads its pickle (written by run_defense_surface and
    run_defense_critical; a missing one ends the run with a message naming the command), and the classifier's is written as
    classifier_configuration.json next to the outputs,
  - the classifier's weights are read from <classifier_folder>/model-%03d.ckpt by the TF-free checkpoint reader
    (<classifier_folder>/weights.npz with the same variable names is the fallback),
  - adversarial and before_defense take the distance weight of every attack from analysis_results/source_target_norm_min_idx.npy
    (written by evaluate_attack) when it exists; without it, an attack run with a single distance weight uses weight 0 (what
    that file would hold), and one with several is refused.
"""
import argparse
import json
import os
import os.path as osp
import time

import numpy as np

DEFENSE_TYPES = ('source', 'before_defense', 'after_defense')


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--classifier_folder', type=str, default='log/pointnet')
    p.add_argument('--classifier_restore_epoch', type=int, default=150)
    p.add_argument('--data_type', type=str, default='adversarial')
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--num_points', type=int, default=2048)
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--defense_folder', type=str, default='defense_critical_res')
    p.add_argument('--output_folder_name', type=str, default='classifier_res')
    p.add_argument('--num_classes', type=int, default=13)
    p.add_argument('--top_dir', type=str, default='.', help='root that the folder flags are relative to')
    return p


def classifier_weights_path(classifier_path, restore_epoch):
    """<classifier_path>/model-%03d.ckpt when it exists, else <classifier_path>/weights.npz."""
    from .cls_weights import checkpoint_prefix
    prefix = checkpoint_prefix(classifier_path, restore_epoch)
    return prefix if osp.exists(prefix + '.index') else osp.join(classifier_path, 'weights.npz')


def _paths(flags, attack_path):
    """(classifier_data_path, output folder, configuration file) of every data type (run_classifier.py:49-83)."""
    defense_path = osp.join(attack_path, flags.defense_folder)
    return {'target': (attack_path, flags.output_folder_name + '_orig', 'attack_configuration.json'),
            'adversarial': (attack_path, flags.output_folder_name, 'attack_configuration.json'),
            'source': (defense_path, flags.output_folder_name + '_orig', 'defense_configuration.json'),
            'before_defense': (attack_path, osp.join(flags.defense_folder, flags.output_folder_name),
                               osp.join(flags.defense_folder, 'defense_configuration.json')),
            'after_defense': (defense_path, flags.output_folder_name, 'defense_configuration.json')}[flags.data_type]


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Run classifier flags:', flags)
    assert flags.data_type in ('target', 'adversarial') + DEFENSE_TYPES, 'wrong data_type: %s.' % flags.data_type

    from .attack_data import create_dir, get_quantity_at_index, load_data, prepare_data_for_attack, select_dist_weight
    from .classifier import PointNetClassifier

    data_path = osp.join(flags.top_dir, flags.ae_folder, 'eval')
    files = [f for f in os.listdir(data_path) if osp.isfile(osp.join(data_path, f))]
    classifier_path = osp.join(flags.top_dir, flags.classifier_folder)
    classifier_data_path, output_folder, conf_file = _paths(flags, osp.join(data_path, flags.attack_folder))
    conf_path = osp.join(classifier_data_path, conf_file)
    if not osp.exists(conf_path):
        if flags.data_type in DEFENSE_TYPES:
            raise SystemExit('run_classifier: --data_type %s reads %s, which is missing: run geometric_adv_amd.run_defense_surface '
                             'or run_defense_critical with --output_folder_name %s first'
                             % (flags.data_type, conf_path, flags.defense_folder.rsplit('_orig', 1)[0]))
        raise FileNotFoundError('%s is missing: run geometric_adv_amd.run_attack first' % conf_path)
    output_path = create_dir(osp.join(classifier_data_path, output_folder))

    with open(conf_path) as f:
        conf = json.load(f)
    conf.update(classifier_path=classifier_path, classifier_restore_epoch=flags.classifier_restore_epoch,
                classifier_data_path=classifier_data_path)
    with open(osp.join(output_path, 'classifier_configuration.json'), 'w') as f:
        json.dump(conf, f)

    pc_classes, slice_idx, reconstructions = load_data(data_path, files, ['pc_classes', 'slice_idx_test_set',
                                                                          'reconstructions_test_set'])
    nn_idx_dict = {'latent_nn': 'latent_nn_idx_test_set', 'chamfer_nn_complete': 'chamfer_nn_idx_complete_test_set'}
    nn_idx = load_data(data_path, files, [nn_idx_dict[conf['target_pc_idx_type']]])
    correct_pred = None
    if conf['correct_pred_only']:
        pc_labels, pc_pred_labels = load_data(data_path, files, ['pc_label_test_set', 'pc_pred_labels_test_set'])
        correct_pred = (pc_labels == pc_pred_labels)
    attack_pc_idx = np.load(osp.join(flags.top_dir, flags.attack_pc_idx))[:, :conf['num_pc_for_attack']]

    classifier = PointNetClassifier(classifier_path, flags.classifier_restore_epoch, num_points=flags.num_points, batch_size=10,
                                    num_classes=flags.num_classes,
                                    weights=classifier_weights_path(classifier_path, flags.classifier_restore_epoch))
    classes = conf['class_names']
    n_weights = len(conf.get('dist_weight_list', [1.0]))
    for i in range(len(pc_classes)):
        name = str(pc_classes[i])
        if name not in classes:
            continue
        save_dir = create_dir(osp.join(output_path, name))
        print('Classify shape class %s (%d out of %d classes) ' % (name, i + 1, len(pc_classes)))
        start = time.time()
        source_recon_ref, target_recon_ref = prepare_data_for_attack(pc_classes, [pc_classes[i]], classes, reconstructions, slice_idx,
                                                                     attack_pc_idx, conf['num_pc_for_target'], nn_idx, correct_pred)
        load_dir = osp.join(classifier_data_path, name)
        defense_on_adv = False
        if flags.data_type == 'target':
            pc_recon = np.expand_dims(target_recon_ref, axis=0)
        elif flags.data_type in ('adversarial', 'before_defense'):
            adversarial_pc_recon = np.load(osp.join(load_dir, 'adversarial_pc_recon.npy'))
            sel = select_dist_weight(load_dir, adversarial_pc_recon.shape[1], n_weights)
            pc_recon = np.expand_dims(get_quantity_at_index([adversarial_pc_recon], sel), axis=0)
        elif flags.data_type == 'source':
            pc_recon = np.expand_dims(source_recon_ref, axis=0)
        else:
            defense_on_adv = osp.exists(osp.join(load_dir, 'defended_pc_recon.npy'))
            if defense_on_adv:
                pc_recon = np.load(osp.join(load_dir, 'defended_pc_recon.npy'))          # defense on adversarial input
            else:
                pc_recon = np.expand_dims(np.load(osp.join(load_dir, 'defended_source_recon.npy')), axis=0)   # on clean input
        num_dist_weight, num_pc = pc_recon.shape[:2]
        pc_recon_pred = np.zeros([num_dist_weight, num_pc], dtype=np.int8)
        for j in range(num_dist_weight):
            pc_recon_pred[j] = classifier.classify(pc_recon[j])
        if flags.data_type == 'after_defense':
            out_name = 'defended_pc_recon_pred' if defense_on_adv else 'defended_source_recon_pred'
            if not defense_on_adv:
                pc_recon_pred = np.squeeze(pc_recon_pred, axis=0)
        else:
            out_name = {'target': 'target_pc_recon_pred', 'adversarial': 'adversarial_pc_recon_pred',
                        'before_defense': 'adversarial_pc_recon_pred', 'source': 'source_pc_recon_pred'}[flags.data_type]
        np.save(osp.join(save_dir, out_name), pc_recon_pred)
        print('Duration (minutes): %.2f' % ((time.time() - start) / 60.0))


if __name__ == '__main__':
    main()
