"""What get_knn_dists_per_point, run_defense_surface and run_defense_critical share: the attack folder's settings and test-set
arrays, the (source, target) pairs of a class, the adversarial arrays at the selected distance weight, and the per-class loop
of the two defenses (defender/run_defense_surface.py:96-271, run_defense_critical.py:95-266).

Every array of a class goes to the GPU once; the kNN file, the outlier / critical-point packing, the victim AE and the
Chamfer scores run on device tensors, and the results come back once, for np.save.
"""
import json
import os
import os.path as osp
import time

import numpy as np

from .attack_data import create_dir, get_quantity_at_index, load_data, prepare_data_for_attack, select_dist_weight


class AttackFolder:
    """<top_dir>/<ae_folder>/eval and its <attack_folder>: attack_configuration.json (written by run_attack in place of the
    reference's pickled Configuration) and the test-set arrays named by `bases`."""

    def __init__(self, top_dir, ae_folder, attack_folder, attack_pc_idx, bases):
        self.data_path = osp.join(top_dir, ae_folder, 'eval')
        self.files = [f for f in os.listdir(self.data_path) if osp.isfile(osp.join(self.data_path, f))]
        self.attack_dir = osp.join(self.data_path, attack_folder)
        with open(osp.join(self.attack_dir, 'attack_configuration.json')) as f:
            self.conf = json.load(f)
        self.pc_classes, self.slice_idx = load_data(self.data_path, self.files, ['pc_classes', 'slice_idx_test_set'])
        arrays = load_data(self.data_path, self.files, list(bases))
        self.arrays = dict(zip(bases, arrays if len(bases) > 1 else [arrays]))
        nn_idx_dict = {'latent_nn': 'latent_nn_idx_test_set', 'chamfer_nn_complete': 'chamfer_nn_idx_complete_test_set'}
        self.nn_idx = load_data(self.data_path, self.files, [nn_idx_dict[self.conf['target_pc_idx_type']]])
        self.correct_pred = None
        if self.conf['correct_pred_only']:
            pc_labels, pc_pred_labels = load_data(self.data_path, self.files, ['pc_label_test_set', 'pc_pred_labels_test_set'])
            self.correct_pred = (pc_labels == pc_pred_labels)
        self.attack_pc_idx = np.load(osp.join(top_dir, attack_pc_idx))[:, :self.conf['num_pc_for_attack']]
        self.classes = self.conf['class_names']
        self.n_weights = len(self.conf.get('dist_weight_list', [1.0]))

    def attacked(self):
        """(position in pc_classes, name) of every attacked class, in the order of pc_classes."""
        return [(i, str(c)) for i, c in enumerate(self.pc_classes) if str(c) in self.classes]

    def prep(self, i, base):
        """(source, target) of class i for the test-set array `base` (adversary_utils.prepare_data_for_attack)."""
        return prepare_data_for_attack(self.pc_classes, [self.pc_classes[i]], self.classes, self.arrays[base], self.slice_idx,
                                       self.attack_pc_idx, self.conf['num_pc_for_target'], self.nn_idx, self.correct_pred)

    def selected(self, name, files):
        """The attack's arrays `files` of class `name` at the selected distance weight of every attack, as [1, n, ...]."""
        load_dir = osp.join(self.attack_dir, name)
        arrays = [np.load(osp.join(load_dir, f + '.npy')) for f in files]
        sel = select_dist_weight(load_dir, arrays[0].shape[1], self.n_weights)
        return [np.expand_dims(get_quantity_at_index([a], sel), axis=0) for a in arrays]


def write_defense_configuration(folder, output_path, output_path_orig, defense_args):
    """run_defense_*.py:70-76: the attack's configuration plus the defense's flags, in both output folders (JSON in place of
    the pickled Configuration)."""
    conf = dict(folder.conf, ae_dir=osp.dirname(folder.data_path), **defense_args)
    for path in (output_path, output_path_orig):
        with open(osp.join(path, 'defense_configuration.json'), 'w') as f:
            json.dump(dict(conf, train_dir=path), f)


def run_defense(flags, kind):
    """The per-class loop of run_defense_surface.py (kind 'surface') or run_defense_critical.py (kind 'critical'), and of the
    two defenses the reference does not have: statistical outlier removal (kind 'sor': ops.sor_filter on kNN distances computed
    on the device, no kNN files) and simple random sampling (kind 'srs': ops.random_drop with counter = the class's position in
    pc_classes, slot = row for the adversarial half and number of rows + row for the _orig half, so a rerun reproduces the
    files).  Both write the surface defense's files; adversarial_critical_* / original_*critical* hold the removed points."""
    import torch
    from . import ops
    from .autoencoder import PointNetAE
    from .run_attack import victim_weights_path

    folder = AttackFolder(flags.top_dir, flags.ae_folder, flags.attack_folder, flags.attack_pc_idx,
                          ['point_clouds_test_set', 'latent_vectors_test_set', 'ae_loss_test_set', 'reconstructions_test_set'])
    assert np.all(folder.arrays['ae_loss_test_set'] > 0), 'Note: not all autoencoder loss values are larger than 0 as they should!'
    bottleneck_size = folder.arrays['latent_vectors_test_set'].shape[1]
    if kind == 'srs' and not 0 <= flags.drop_num < folder.arrays['point_clouds_test_set'].shape[1]:
        raise ValueError('--drop_num must be in [0, %d), the number of points of a cloud (got %d)'
                         % (folder.arrays['point_clouds_test_set'].shape[1], flags.drop_num))
    output_path = create_dir(osp.join(folder.attack_dir, flags.output_folder_name))
    output_path_orig = create_dir(osp.join(folder.attack_dir, flags.output_folder_name + '_orig'))
    defense_args = {}
    if kind == 'surface':
        defense_args = dict(num_knn_for_defense=flags.num_knn_for_defense, knn_dist_thresh=flags.knn_dist_thresh)
    elif kind == 'sor':
        defense_args = dict(num_knn_for_defense=flags.num_knn_for_defense, sor_alpha=flags.sor_alpha)
    elif kind == 'srs':
        defense_args = dict(drop_num=flags.drop_num, seed=flags.seed)
    write_defense_configuration(folder, output_path, output_path_orig, defense_args)

    point_clouds = folder.arrays['point_clouds_test_set']
    ae = PointNetAE(victim_weights_path(osp.join(flags.top_dir, flags.ae_folder), folder.conf.get('restore_epoch', 500)),
                    int(point_clouds.shape[1]))
    assert ae.bneck == bottleneck_size, 'the victim has a %d-channel bottleneck, latent_vectors_test_set %d' % (ae.bneck,
                                                                                                              bottleneck_size)
    for i, name in folder.attacked():
        save_dir = create_dir(osp.join(output_path, name))
        save_dir_orig = create_dir(osp.join(output_path_orig, name))
        print('defend shape class %s (%d out of %d classes) ' % (name, i + 1, len(folder.pc_classes)))
        start = time.time()
        if kind == 'surface':       # (before anything is computed: the kNN files are this defense's input)
            knn_files = [osp.join(save_dir, 'knn_dists_adversarial_pc_input.npy'), osp.join(save_dir_orig, 'knn_dists_source_pc.npy')]
            missing = [f for f in knn_files if not osp.exists(f)]
            if missing:
                raise FileNotFoundError('%s: missing; run geometric_adv_amd.get_knn_dists_per_point with --output_folder_name %s '
                                        'first' % (', '.join(missing), flags.output_folder_name))
        source_pc, target_pc = folder.prep(i, 'point_clouds_test_set')
        source_ae_loss_ref, target_ae_loss_ref = folder.prep(i, 'ae_loss_test_set')
        source_recon_ref, _ = folder.prep(i, 'reconstructions_test_set')
        source_ae_loss_ref, target_ae_loss_ref = source_ae_loss_ref.reshape(-1), target_ae_loss_ref.reshape(-1)
        adversarial_pc_input, adversarial_pc_recon, adversarial_metrics = folder.selected(
            name, ['adversarial_pc_input', 'adversarial_pc_recon', 'adversarial_metrics'])
        dtype = adversarial_metrics.dtype
        src = ae._as_dev(source_pc)
        adv = ae._as_dev(adversarial_pc_input[0])

        # the victim on the adversarial clouds (the adversarial score; and the sanity checks', with the clean sources)
        adv_recon, _ = ae.forward(adv)
        src_recon = ae.forward(src)[0] if flags.do_sanity_checks else None
        adv_source_err = ae.loss_per_pc_tensor(adv_recon, src)
        if kind == 'surface':
            knn_adv = torch.from_numpy(np.load(knn_files[0])[0]).to(ae.device)
            knn_src = torch.from_numpy(np.load(knn_files[1])).to(ae.device)
            a_pts, a_idx, a_num, a_def = ops.outlier_filter(adv, knn_adv, flags.knn_dist_thresh, top_k=flags.num_knn_for_defense)
            s_pts, s_idx, s_num, s_def = ops.outlier_filter(src, knn_src, flags.knn_dist_thresh, top_k=flags.num_knn_for_defense)
        elif kind == 'sor':
            a_pts, a_idx, a_num, a_def = ops.sor_filter(adv, None, k=flags.num_knn_for_defense, alpha=flags.sor_alpha)
            s_pts, s_idx, s_num, s_def = ops.sor_filter(src, None, k=flags.num_knn_for_defense, alpha=flags.sor_alpha)
        elif kind == 'srs':
            rows = int(adv.shape[0])
            a_def, a_idx = ops.random_drop(adv, flags.drop_num, flags.seed, counter=i, slot_offset=0, return_idx=True)
            s_def, s_idx = ops.random_drop(src, flags.drop_num, flags.seed, counter=i, slot_offset=rows, return_idx=True)
            a_pts = torch.gather(adv, 1, a_idx.long().unsqueeze(-1).expand(-1, -1, 3))
            s_pts = torch.gather(src, 1, s_idx.long().unsqueeze(-1).expand(-1, -1, 3))
            a_idx, s_idx = a_idx.to(torch.int16), s_idx.to(torch.int16)           # (n <= 32767: the other defenses' dtype)
            a_num = torch.full((rows,), flags.drop_num, dtype=torch.int16, device=adv.device)
            s_num = torch.full((int(src.shape[0]),), flags.drop_num, dtype=torch.int16, device=src.device)
        else:
            mv, mi = ae.max_and_argmax(adv)
            a_pts, a_idx, a_num, a_crit, a_def = ops.critical_split(adv, mv, mi)
            mv, mi = ae.max_and_argmax(src)
            s_pts, s_idx, s_num, s_crit, s_def = ops.critical_split(src, mv, mi)
        a_def_recon, _ = ae.forward(a_def)
        a_def_err = ae.loss_per_pc_tensor(a_def_recon, src)
        s_def_recon, _ = ae.forward(s_def)
        s_def_err = ae.loss_per_pc_tensor(s_def_recon, src)
        if kind == 'critical' and flags.do_sanity_checks:
            a_crit_recon, _ = ae.forward(a_crit)
            s_crit_recon, _ = ae.forward(s_crit)
        ae.status()                        # (the f16x2 encoder's range guard: raises instead of returning +inf-born numbers)

        if flags.do_sanity_checks:         # run_defense_*.py, the reference's tolerances
            source_recon = src_recon.cpu().numpy()
            source_ae_loss = ae.loss_per_pc_tensor(src_recon, src).cpu().numpy()
            assert np.abs(source_recon - source_recon_ref).max() < 1e-06, \
                'The ae source reconstructions should also be the same! (up to precision errors)'
            assert np.abs(source_ae_loss - source_ae_loss_ref).max() < 1e-08, \
                'the ae source loss should also be the same! (up to precision errors)'
            target_recon_error = ae.loss_per_pc_tensor(adv_recon, ae._as_dev(target_pc)).cpu().numpy().astype(dtype)
            target_nre = np.divide(target_recon_error, target_ae_loss_ref)
            assert np.abs(adversarial_pc_recon[0] - adv_recon.cpu().numpy()).max() < 1e-06, \
                'Reconstructions from the attack and reconstructions when running the adversarial point clouds through the AE ' \
                'should also be the same! (up to precision errors)'
            assert np.abs(target_recon_error - adversarial_metrics[0, :, 4]).max() < 1e-08, \
                'The target recon error from the AE and from the attack should be the same! (up to precision errors)'
            assert np.abs(target_nre - adversarial_metrics[0, :, 3]).max() < 1e-04, \
                'The target normalized recon error from the AE and from the attack should be the same! (up to precision errors)'
            if kind == 'critical':
                assert torch.equal(adv_recon, a_crit_recon), \
                    'Reconstructions of adversarial point clouds and of adversarial critical points should be equal!'
                assert np.abs(source_recon_ref - s_crit_recon.cpu().numpy()).max() < 1e-06, \
                    'Reconstructions of source point clouds and of source critical points should also be the same! ' \
                    '(up to precision errors)'

        a_pts, a_idx, a_num, a_def, a_def_recon, a_def_err, adv_source_err = [
            t.cpu().numpy() for t in (a_pts, a_idx, a_num, a_def, a_def_recon, a_def_err, adv_source_err)]
        s_pts, s_idx, s_num, s_def, s_def_recon, s_def_err = [t.cpu().numpy() for t in (s_pts, s_idx, s_num, s_def, s_def_recon, s_def_err)]
        a_def_err, adv_source_err, s_def_err = a_def_err.astype(dtype), adv_source_err.astype(dtype), s_def_err.astype(dtype)
        defense_metrics = np.stack([a_def_err, np.divide(a_def_err, source_ae_loss_ref).astype(dtype),
                                    adv_source_err, np.divide(adv_source_err, source_ae_loss_ref).astype(dtype)], axis=-1)[None]
        defense_source_metrics = np.stack([s_def_err, np.divide(s_def_err, source_ae_loss_ref),
                                           source_ae_loss_ref, np.ones_like(source_ae_loss_ref)], axis=-1)
        if kind in ('surface', 'sor'):   # data above the class's max number of outliers can be discarded (run_defense_surface.py:216-220)
            a_max, s_max = int(a_num.max(initial=0)), int(s_num.max(initial=0))
            a_pts, a_idx = a_pts[:, :a_max], a_idx[:, :a_max]
            s_pts, s_idx = s_pts[:, :s_max], s_idx[:, :s_max]

        # the reference's names: adversarial_critical_* / original_*critical* are the OUTLIERS of the surface defense
        np.save(osp.join(save_dir, 'adversarial_critical_points'), a_pts[None])
        np.save(osp.join(save_dir, 'adversarial_critical_idx'), a_idx[None])
        np.save(osp.join(save_dir, 'adversarial_critical_num'), a_num[None])
        np.save(osp.join(save_dir, 'defended_pc_input'), a_def[None])
        np.save(osp.join(save_dir, 'defended_pc_recon'), a_def_recon[None])
        np.save(osp.join(save_dir, 'defense_metrics'), defense_metrics)
        np.save(osp.join(save_dir_orig, 'original_source_critical_points'), s_pts)
        np.save(osp.join(save_dir_orig, 'original_critical_idx'), s_idx)
        np.save(osp.join(save_dir_orig, 'original_critical_num'), s_num)
        np.save(osp.join(save_dir_orig, 'defended_source_input'), s_def)
        np.save(osp.join(save_dir_orig, 'defended_source_recon'), s_def_recon)
        np.save(osp.join(save_dir_orig, 'defense_source_metrics'), defense_source_metrics)
        print('Duration (minutes): %.2f' % ((time.time() - start) / 60.0))
