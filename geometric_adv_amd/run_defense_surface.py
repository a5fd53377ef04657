"""defender/run_defense_surface.py on MI355X: the off-surface defense.  For every attacked class, the points of each
adversarial cloud (at the selected distance weight) whose mean distance to its num_knn_for_defense nearest neighbours exceeds
knn_dist_thresh are dropped, the victim AE reconstructs what is left, and the reconstruction is scored against the clean
source; the same runs on the clean sources (the _orig half), to show what the defense costs them.

    python -m geometric_adv_amd.get_knn_dists_per_point --ae_folder log/autoencoder_victim
    python -m geometric_adv_amd.run_defense_surface --ae_folder log/autoencoder_victim --do_sanity_checks 1

Reads the kNN distances get_knn_dists_per_point wrote (refused with a message naming it when they are missing).  Everything
of a class runs on the GPU from load to download: the outlier filter on the loaded distances (ops.outlier_filter, which forms
numpy's float32 mean of the first num_knn_for_defense distances itself), the victim AE (autoencoder.PointNetAE) and Chamfer.

Writes the reference's file names, in which adversarial_critical_* and original_*critical* hold the OUTLIERS:
  <output_folder_name>/<class>/: adversarial_critical_points [1, n, M, 3] / adversarial_critical_idx [1, n, M] int16 (trimmed
    to the class's largest outlier count M, which may be 0), adversarial_critical_num [1, n] int16, defended_pc_input,
    defended_pc_recon [1, n, N, 3], defense_metrics [1, n, 4] (defended-vs-source error and NRE, adversarial-vs-source error
    and NRE),
  <output_folder_name>_orig/<class>/: original_source_critical_points, original_critical_idx, original_critical_num,
    defended_source_input, defended_source_recon, defense_source_metrics [n, 4] (its last two columns: the source's own AE
    loss and 1),
  and defense_configuration.json in both folders.

Differences forced by the environment:
  - configurations are JSON: the attack's is read from attack_configuration.json (run_attack writes it), and the defense's is
    written as defense_configuration.json (the attack's settings plus num_knn_for_defense and knn_dist_thresh) in place of
    the pickled Configuration, which needs tflearn,
  - the victim's weights are read from <ae_folder>/models.ckpt-<restore_epoch> without TensorFlow (weights.npz is the fallback),
  - --num_knn_for_defense is at most 7: the kernel forms numpy's mean as a left-to-right float32 sum, which is numpy's own
    order only below 8 elements,
  - the distance weight of every attack comes from analysis_results/source_target_norm_min_idx.npy (evaluate_attack); without
    it, an attack run with a single distance weight uses weight 0, one with several is refused.
"""
import argparse


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--num_knn_for_defense', type=int, default=2)
    p.add_argument('--knn_dist_thresh', type=float, default=0.04)
    p.add_argument('--do_sanity_checks', type=int, default=0)
    p.add_argument('--output_folder_name', type=str, default='defense_surface_res')
    p.add_argument('--top_dir', type=str, default='.', help='root that the folder flags are relative to')
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Run defense surface flags:', flags)
    if not 1 <= flags.num_knn_for_defense <= 7:
        raise SystemExit('run_defense_surface: --num_knn_for_defense must be in [1, 7] (got %d)' % flags.num_knn_for_defense)
    from .defense_cli import run_defense
    run_defense(flags, 'surface')


if __name__ == '__main__':
    main()
