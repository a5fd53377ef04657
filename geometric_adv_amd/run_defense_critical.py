"""defender/run_defense_critical.py on MI355X: the critical-points defense.  For every attacked class, the points of each
adversarial cloud (at the selected distance weight) that own a channel of the encoder's max pooling are dropped, the victim AE
reconstructs what is left, and the reconstruction is scored against the clean source; the same runs on the clean sources
(the _orig half).

    python -m geometric_adv_amd.run_defense_critical --ae_folder log/autoencoder_victim --do_sanity_checks 1

Everything of a class runs on the GPU from load to download: the pre-pool max / argmax (PointNetAE.max_and_argmax, without
the (n, N, 128) pre-symmetry tensor), the critical-point split (ops.critical_split), the victim AE and Chamfer.

Writes, as the reference does:
  <output_folder_name>/<class>/: adversarial_critical_points [1, n, bneck, 3], adversarial_critical_idx [1, n, bneck] int16,
    adversarial_critical_num [1, n] int16 (not trimmed), defended_pc_input, defended_pc_recon [1, n, N, 3], defense_metrics
    [1, n, 4],
  <output_folder_name>_orig/<class>/: original_source_critical_points, original_critical_idx, original_critical_num,
    defended_source_input, defended_source_recon, defense_source_metrics [n, 4],
  and defense_configuration.json in both folders.
--do_sanity_checks 1 adds the reference's two checks of this defense: the reconstruction of an adversarial cloud's critical
points equals that of the whole cloud (np.array_equal), and the sources' within 1e-6 of reconstructions_test_set.  Both hold
because the encoder's per-point arithmetic does not depend on the other points of the cloud.

Differences forced by the environment:
  - configurations are JSON (attack_configuration.json in, defense_configuration.json out) in place of the pickled
    Configuration, which needs tflearn; the victim's weights are read without TensorFlow,
  - critical points owning equally many channels come in the kernel's stable order (descending point index).  The reference
    orders them with numpy's default argsort, which is not stable, so its order inside such a group depends on the numpy build;
    the set of critical points, their counts and everything reconstructed from them do not,
  - the distance weight of every attack comes from analysis_results/source_target_norm_min_idx.npy (evaluate_attack); without
    it, an attack run with a single distance weight uses weight 0, one with several is refused.
"""
import argparse


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--do_sanity_checks', type=int, default=0)
    p.add_argument('--output_folder_name', type=str, default='defense_critical_res')
    p.add_argument('--top_dir', type=str, default='.', help='root that the folder flags are relative to')
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Run defense critical flags:', flags)
    from .defense_cli import run_defense
    run_defense(flags, 'critical')


if __name__ == '__main__':
    main()
