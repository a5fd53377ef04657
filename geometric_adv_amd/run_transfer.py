"""transfer/run_transfer.py on MI355X: feeds the adversarial clouds run_attack wrote to another auto-encoder and measures
how well it reconstructs the attack's TARGET shapes, with the reference's flags and output files.

    python -m geometric_adv_amd.run_transfer --transfer_ae_type AtlasNet --transfer_ae_folder log/atlasnet_ae ...

--transfer_ae_type:
  - PointNet: this project's PointNetAE (the victim's architecture, other weights) from
    <transfer_ae_folder>/models.ckpt-<transfer_ae_restore_epoch> (or weights.npz),
  - AtlasNet: atlasnet.AtlasNetAE from <transfer_ae_folder>/network.pth and options.json,
  - FoldingNet: foldingnet.FoldingNetAE from <transfer_ae_folder>/checkpoint_<transfer_ae_restore_epoch>.pth.  Its
    Graph_Pooling draws neighbours with np.random.choice (transfer/foldingnet/foldingnet.py:36-39), which the reference
    never seeds, so not even the reference reproduces its own output.  Here --graph_seed is required (without it
    FoldingNet is refused before any file is read), and --graph_sampling picks how it is used: 'device' (default) draws on
    the GPU from (seed, cloud ordinal, pool layer, point); 'reference' draws with np.random.RandomState(seed).choice on
    the host in the reference's order, reproducing a reference run that called np.random.seed(seed) first (13 to 36 ms of
    host time per cloud).

Differences forced by the environment, as in run_classifier:
  - the attack's configuration is read from <eval>/<attack_folder>/attack_configuration.json (run_attack writes it in place of
    the pickled Configuration); the transfer configuration is written as transfer_configuration.json,
  - the distance weight of every attack comes from analysis_results/source_target_norm_min_idx.npy; without it, an attack run
    with a single distance weight uses weight 0 (what that file would hold),
  - AtlasNet's reconstruction has nb_primitives * g * g points, whatever that is (the reference's buffer fixes 2500),
  - FoldingNet takes clouds of any 17 ... 16384 points (the reference's covariance buffer fixes 2048); its reconstruction
    has 2025 points.
Outputs (only when the transfer folder differs from the victim's, as in the reference, :220-222), per class under
<transfer_ae_folder>/eval/<output_folder_name>/<class>/: transferred_pc_recon.npy [1, n, P, 3] and transfer_metrics.npy
[1, n, 4] (transferred target recon error, transferred target NRE, the attack's target recon error and NRE).
"""
import argparse
import json
import os
import os.path as osp
import time

import numpy as np

AE_TYPES = ('PointNet', 'AtlasNet', 'FoldingNet')


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--transfer_ae_folder', type=str, default='log/autoencoder_for_transfer')
    p.add_argument('--transfer_ae_restore_epoch', type=int, default=500)
    p.add_argument('--transfer_ae_type', type=str, default='PointNet')
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--do_sanity_checks', type=int, default=0)
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--output_folder_name', type=str, default='attack_res_transfer')
    p.add_argument('--top_dir', type=str, default='.', help='root that the folder flags are relative to')
    p.add_argument('--graph_seed', type=int, default=None,
                   help="FoldingNet: seed of the graph pooling's neighbour draws (required for FoldingNet)")
    p.add_argument('--graph_sampling', type=str, default='device', choices=['device', 'reference'],
                   help="FoldingNet: 'device' draws on the GPU; 'reference' reproduces np.random.seed(graph_seed) followed "
                        "by the reference's np.random.choice calls")
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    assert flags.transfer_ae_type in AE_TYPES, 'wrong ae_type: %s.' % flags.transfer_ae_type
    if flags.transfer_ae_type == 'FoldingNet' and flags.graph_seed is None:
        raise SystemExit('run_transfer: --transfer_ae_type FoldingNet needs --graph_seed: its Graph_Pooling draws neighbours '
                         'with an unseeded np.random.choice (foldingnet.py:36-39), so without a seed its reconstructions '
                         'are not reproducible, not even by the reference')
    print('Run transfer flags:', flags)

    from .attack_data import create_dir, get_quantity_at_index, load_data, prepare_data_for_attack, select_dist_weight

    data_path = osp.join(flags.top_dir, flags.ae_folder, 'eval')
    files = [f for f in os.listdir(data_path) if osp.isfile(osp.join(data_path, f))]
    attack_path = osp.join(data_path, flags.attack_folder)
    transfer_ae_dir = osp.join(flags.top_dir, flags.transfer_ae_folder)
    output_path = create_dir(osp.join(transfer_ae_dir, 'eval', flags.output_folder_name))

    with open(osp.join(attack_path, 'attack_configuration.json')) as f:
        conf = json.load(f)
    conf.update(attack_path=attack_path, transfer_ae_restore_epoch=flags.transfer_ae_restore_epoch,
                transfer_ae_type=flags.transfer_ae_type, transfer_ae_folder=flags.transfer_ae_folder,
                graph_seed=flags.graph_seed, graph_sampling=flags.graph_sampling)
    with open(osp.join(output_path, 'transfer_configuration.json'), 'w') as f:
        json.dump(conf, f)

    point_clouds, pc_classes, slice_idx, ae_loss, reconstructions = load_data(
        data_path, files, ['point_clouds_test_set', 'pc_classes', 'slice_idx_test_set', 'ae_loss_test_set',
                           'reconstructions_test_set'])
    assert np.all(ae_loss > 0), 'Note: not all autoencoder loss values are larger than 0 as they should!'
    nn_idx_dict = {'latent_nn': 'latent_nn_idx_test_set', 'chamfer_nn_complete': 'chamfer_nn_idx_complete_test_set'}
    nn_idx = load_data(data_path, files, [nn_idx_dict[conf['target_pc_idx_type']]])
    correct_pred = None
    if conf['correct_pred_only']:
        pc_labels, pc_pred_labels = load_data(data_path, files, ['pc_label_test_set', 'pc_pred_labels_test_set'])
        correct_pred = (pc_labels == pc_pred_labels)
    attack_pc_idx = np.load(osp.join(flags.top_dir, flags.attack_pc_idx))[:, :conf['num_pc_for_attack']]

    if flags.transfer_ae_type == 'AtlasNet':
        from .atlasnet import AtlasNetAE
        ae = AtlasNetAE(transfer_ae_dir)
    elif flags.transfer_ae_type == 'FoldingNet':
        from .foldingnet import FoldingNetAE
        ae = FoldingNetAE(transfer_ae_dir, epoch=flags.transfer_ae_restore_epoch, seed=flags.graph_seed,
                          sampling=flags.graph_sampling)
    else:
        from .autoencoder import PointNetAE
        from .run_attack import victim_weights_path
        ae = PointNetAE(victim_weights_path(transfer_ae_dir, flags.transfer_ae_restore_epoch), int(point_clouds.shape[1]))

    classes = conf['class_names']
    n_weights = len(conf.get('dist_weight_list', [1.0]))
    sanity = (flags.transfer_ae_folder == flags.ae_folder and flags.transfer_ae_restore_epoch == conf.get('restore_epoch')
              and flags.do_sanity_checks)
    for i in range(len(pc_classes)):
        name = str(pc_classes[i])
        if name not in classes:
            continue
        save_dir = create_dir(osp.join(output_path, name))
        print('transfer shape class %s (%d out of %d classes) ' % (name, i + 1, len(pc_classes)))
        start = time.time()
        prep = lambda data: prepare_data_for_attack(pc_classes, [pc_classes[i]], classes, data, slice_idx, attack_pc_idx,
                                                     conf['num_pc_for_target'], nn_idx, correct_pred)
        _, target_pc = prep(point_clouds)
        _, target_ae_loss_ref = prep(ae_loss)
        _, target_recon_ref = prep(reconstructions)
        target_ae_loss_ref = target_ae_loss_ref.reshape(-1)

        load_dir = osp.join(attack_path, name)
        adversarial_pc_input = np.load(osp.join(load_dir, 'adversarial_pc_input.npy'))
        adversarial_pc_recon = np.load(osp.join(load_dir, 'adversarial_pc_recon.npy'))
        adversarial_metrics = np.load(osp.join(load_dir, 'adversarial_metrics.npy'))
        sel = select_dist_weight(load_dir, adversarial_pc_input.shape[1], n_weights)
        adversarial_pc_input, adversarial_pc_recon, adversarial_metrics = [
            np.expand_dims(q, axis=0) for q in
            get_quantity_at_index([adversarial_pc_input, adversarial_pc_recon, adversarial_metrics], sel)]
        num_dist_weight, num_pc = adversarial_pc_input.shape[:2]

        if flags.transfer_ae_type == 'PointNet':
            transferred_pc_recon = np.zeros_like(adversarial_pc_recon)
        else:
            transferred_pc_recon = np.zeros([1, num_pc, ae.num_points, 3], dtype=adversarial_pc_recon.dtype)
        transferred_target_recon_error = np.zeros([num_dist_weight, num_pc], dtype=adversarial_metrics.dtype)
        transferred_target_nre = np.zeros([num_dist_weight, num_pc], dtype=adversarial_metrics.dtype)
        for j in range(num_dist_weight):
            pc_input = adversarial_pc_input[j]
            pc_recon = ae.get_reconstructions(pc_input)
            transferred_pc_recon[j] = pc_recon
            if flags.transfer_ae_type == 'PointNet':
                err = ae.get_loss_per_pc(pc_input, target_pc)          # reconstructs pc_input itself
            else:
                err = ae.get_loss_per_pc(pc_recon, target_pc)
            transferred_target_recon_error[j] = err.astype(adversarial_metrics.dtype)
            transferred_target_nre[j] = np.divide(transferred_target_recon_error[j], target_ae_loss_ref)
        adversarial_target_recon_error = adversarial_metrics[:, :, 4]
        adversarial_target_nre = adversarial_metrics[:, :, 3]

        if sanity:     # run_transfer.py:180-204, the same tolerances
            assert flags.transfer_ae_type == 'PointNet', \
                'the sanity checks are for transfer_ae_type "PointNet" (got "%s")' % flags.transfer_ae_type
            target_recon = ae.get_reconstructions(target_pc)
            target_ae_loss = ae.get_loss_per_pc(target_pc)
            assert np.abs(target_recon - target_recon_ref).max() < 1e-06, \
                'when transfer_ae_folder and ae_folder are the same, the ae target reconstructions should also be the same!'
            assert np.abs(target_ae_loss - target_ae_loss_ref).max() < 1e-08, \
                'when transfer_ae_folder and ae_folder are the same, the ae target loss should also be the same!'
            assert np.abs(transferred_pc_recon - adversarial_pc_recon).max() < 1e-06, \
                'when transfer_ae_folder and ae_folder are the same, the ae adversarial reconstructions should also be the same!'
            assert np.abs(transferred_target_recon_error - adversarial_target_recon_error).max() < 1e-08, \
                'when transfer_ae_folder and ae_folder are the same, the ae target recon error should also be the same!'
            assert np.abs(transferred_target_nre - adversarial_target_nre).max() < 1e-04, \
                'when transfer_ae_folder and ae_folder are the same, the ae target normalized recon error should also be the same!'

        transfer_metrics = np.concatenate([np.expand_dims(m, axis=-1) for m in
                                           [transferred_target_recon_error, transferred_target_nre,
                                            adversarial_target_recon_error, adversarial_target_nre]], axis=-1)
        if flags.transfer_ae_folder != flags.ae_folder:
            np.save(osp.join(save_dir, 'transferred_pc_recon'), transferred_pc_recon)
            np.save(osp.join(save_dir, 'transfer_metrics'), transfer_metrics)
        print('Duration (minutes): %.2f' % ((time.time() - start) / 60.0))


if __name__ == '__main__':
    main()
