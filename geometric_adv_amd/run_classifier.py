"""classifier/run_classifier.py on MI355X: the reference's flags and per-class output files for --data_type target and
adversarial, with the PointNet classifier running as HIP kernels (classifier.py).

    python -m geometric_adv_amd.run_classifier --data_type adversarial --ae_folder log/autoencoder_victim ...

Differences forced by the environment:
  - the attack's configuration is read from <eval>/<attack_folder>/attack_configuration.json, which this project's
    run_attack writes in place of the pickled Configuration (which needs tflearn to unpickle); the classifier's
    configuration is written as classifier_configuration.json next to the outputs,
  - the classifier's weights are read from <classifier_folder>/model-%03d.ckpt by the TF-free checkpoint reader
    (<classifier_folder>/weights.npz with the same variable names is the fallback),
  - --data_type adversarial takes the distance weight of every attack from analysis_results/source_target_norm_min_idx.npy
    when it exists; without it, an attack run with a single distance weight uses weight 0 (what that file would hold),
  - source, before_defense and after_defense read defense outputs that no command of this project writes yet: refused.
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


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Run classifier flags:', flags)
    assert flags.data_type in ('target', 'adversarial') + DEFENSE_TYPES, 'wrong data_type: %s.' % flags.data_type
    if flags.data_type in DEFENSE_TYPES:
        raise SystemExit('run_classifier: --data_type %s classifies defense outputs (defense_configuration, defended_*.npy), '
                         'which no command of this project writes; only target and adversarial are supported' % flags.data_type)

    from .attack_data import create_dir, get_quantity_at_index, load_data, prepare_data_for_attack
    from .classifier import PointNetClassifier

    data_path = osp.join(flags.top_dir, flags.ae_folder, 'eval')
    files = [f for f in os.listdir(data_path) if osp.isfile(osp.join(data_path, f))]
    classifier_path = osp.join(flags.top_dir, flags.classifier_folder)
    classifier_data_path = osp.join(data_path, flags.attack_folder)
    suffix = '_orig' if flags.data_type == 'target' else ''
    output_path = create_dir(osp.join(classifier_data_path, flags.output_folder_name + suffix))

    with open(osp.join(classifier_data_path, 'attack_configuration.json')) as f:
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
        _, target_recon_ref = prepare_data_for_attack(pc_classes, [pc_classes[i]], classes, reconstructions, slice_idx,
                                                      attack_pc_idx, conf['num_pc_for_target'], nn_idx, correct_pred)
        load_dir = osp.join(classifier_data_path, name)
        if flags.data_type == 'target':
            pc_recon = np.expand_dims(target_recon_ref, axis=0)
        else:
            adversarial_pc_recon = np.load(osp.join(load_dir, 'adversarial_pc_recon.npy'))
            idx_file = osp.join(load_dir, 'analysis_results', 'source_target_norm_min_idx.npy')
            if osp.exists(idx_file):
                sel = np.load(idx_file)
            elif n_weights == 1:
                sel = np.zeros(adversarial_pc_recon.shape[1], dtype=np.int64)
            else:
                raise FileNotFoundError('%s is missing: the attack used %d distance weights, and that file selects one per '
                                        'attack' % (idx_file, n_weights))
            pc_recon = np.expand_dims(get_quantity_at_index([adversarial_pc_recon], sel), axis=0)
        num_dist_weight, num_pc = pc_recon.shape[:2]
        pc_recon_pred = np.zeros([num_dist_weight, num_pc], dtype=np.int8)
        for j in range(num_dist_weight):
            pc_recon_pred[j] = classifier.classify(pc_recon[j])
        out_name = 'target_pc_recon_pred' if flags.data_type == 'target' else 'adversarial_pc_recon_pred'
        np.save(osp.join(save_dir, out_name), pc_recon_pred)
        print('Duration (minutes): %.2f' % ((time.time() - start) / 60.0))


if __name__ == '__main__':
    main()
