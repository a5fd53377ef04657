"""autoencoder/tst_ae.py on MI355X: evaluates a trained victim auto-encoder on one split of the ShapeNet PLY folder and
writes the folder every later stage reads (run_attack, prepare_indices_for_attack, get_dists_per_point, the defenses,
run_classifier, run_transfer, train_classifier): <train_folder>/<output_folder_name>/ with, for <set> = --set_type and
<oc> = '_'.join(object_class),

    pc_classes_<oc>.npy            the class names
    pc_label_<set>_<oc>.npy        class index of every cloud, int8
    slice_idx_<set>_<oc>.npy       start of every class in the cloud array, and the total
    point_clouds_<set>_<oc>.npy    the clouds (axes sorted if the configuration says so), float32 (N, n, 3)
    latent_vectors_<set>_<oc>.npy  float32 (N, 128)
    reconstructions_<set>_<oc>.npy float32 (N, n, 3)
    ae_loss_<set>_<oc>.npy         Chamfer reconstruction error per cloud, float32 (N,)
    eval_stats_<set>_<oc>.txt      `Mean ae loss: %.9f`

-- the reference's names and dtypes.  The run reads <train_folder>/configuration.json (written by train_ae: JSON where the
reference pickles), loads the split with in_out.load_dataset (files sorted by full path: in_out's file-order decision), sorts
the axes on the device (ops.sort_axes), restores models.ckpt-<restore_epoch> and takes the three arrays from ONE forward per
chunk (PointNetAE.evaluate; the reference runs three).

    python -m geometric_adv_amd.tst_ae --train_folder log/autoencoder_victim --restore_epoch 500 --set_type test_set
"""
import argparse
import os.path as osp

import numpy as np

SET_TYPES = ('train_set', 'val_set', 'test_set')
ARRAYS = ('pc_label', 'slice_idx', 'point_clouds', 'latent_vectors', 'reconstructions', 'ae_loss')


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--restore_epoch', type=int, default=500, help='Restore epoch of a trained autoencoder [default: 500]')
    p.add_argument('--set_type', type=str, default='test_set', help='Set for evaluation of the autoencoder [default: test_set]')
    p.add_argument('--train_folder', type=str, default='log/autoencoder_victim',
                   help='Folder for saved data form the training phase [default: log/autoencoder_victim]')
    p.add_argument('--output_folder_name', type=str, default='eval', help="Output folder name")
    p.add_argument('--top_dir', type=str, default='.', help='root that --train_folder is relative to')
    p.add_argument('--data_dir', type=str, default=None,
                   help='ShapeNet PLY folder [default: <top_dir>/data/shape_net_core_uniform_samples_2048]')
    return p


def eval_file_names(set_type, object_class):
    """{'pc_classes': ..., 'pc_label': ..., ..., 'eval_stats': ...}: the eight file names of tst_ae.py:75-121."""
    names = {'pc_classes': '_'.join(['pc_classes'] + list(object_class)) + '.npy'}
    for base in ARRAYS:
        names[base] = '_'.join([base, set_type] + list(object_class)) + '.npy'
    names['eval_stats'] = '_'.join(['eval_stats', set_type] + list(object_class)) + '.txt'
    return names


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Test autoencoder flags:', flags)
    if flags.set_type not in SET_TYPES:
        raise ValueError('--set_type must be one of %s, not %r' % (SET_TYPES, flags.set_type))
    import torch
    from . import dist as gdist, in_out, tf_checkpoint
    from .autoencoder import PointNetAE
    from .train_ae import load_configuration, sort_axes_on_device
    data_dir = flags.data_dir if flags.data_dir is not None else osp.join(flags.top_dir, 'data', 'shape_net_core_uniform_samples_2048')
    train_dir = osp.join(flags.top_dir, flags.train_folder)
    conf = load_configuration(train_dir)
    if conf['data_source'] != 'data_dir':
        raise ValueError('%s was trained on a .npy of clouds (train_ae --train_data): its configuration names no classes to '
                         'read from the PLY folder' % train_dir)
    object_class, class_names = conf['object_class'], conf['class_names']

    pc_data, slice_idx, pc_label = in_out.load_dataset(class_names, flags.set_type, data_dir)
    point_clouds = pc_data.point_clouds.copy()
    if len(point_clouds) == 0:
        raise ValueError('the %s of %s under %s is empty' % (flags.set_type, class_names, data_dir))
    if tuple(point_clouds.shape[1:]) != tuple(conf['n_input']):
        raise ValueError('the clouds under %s are %s, the model was trained on %s' % (data_dir, point_clouds.shape[1:], conf['n_input']))
    device = torch.device('cuda', gdist.env_rank()[2])          # the local rank's GPU, as the other commands
    if conf['sort_axes']:
        point_clouds = sort_axes_on_device(point_clouds, device)

    weights = tf_checkpoint.restore_ae_weights(train_dir, flags.restore_epoch, conf['experiment_name'])
    ae = PointNetAE(weights, point_clouds.shape[1], ae_name=conf['experiment_name'], device=device)
    latent_vectors, reconstructions, loss_per_pc = ae.evaluate(point_clouds)

    eval_dir = in_out.create_dir(osp.join(train_dir, flags.output_folder_name))
    names = eval_file_names(flags.set_type, object_class)
    np.save(osp.join(eval_dir, names['pc_classes']), np.array(class_names))
    np.save(osp.join(eval_dir, names['pc_label']), np.array(pc_label).astype(np.int8))
    np.save(osp.join(eval_dir, names['slice_idx']), np.array(slice_idx))
    np.save(osp.join(eval_dir, names['point_clouds']), point_clouds)
    np.save(osp.join(eval_dir, names['latent_vectors']), latent_vectors)
    np.save(osp.join(eval_dir, names['reconstructions']), reconstructions)
    np.save(osp.join(eval_dir, names['ae_loss']), loss_per_pc)
    with open(osp.join(eval_dir, names['eval_stats']), 'w', 1) as log_file:
        log_file.write('Mean ae loss: %.9f\n' % loss_per_pc.mean())
    return eval_dir


if __name__ == '__main__':
    main()
