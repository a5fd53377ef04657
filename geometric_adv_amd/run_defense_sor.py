"""Statistical outlier removal (SOR) as a defense, on MI355X: the baseline of DUP-Net and IF-Defense, which the reference does
not have.  For every attacked class, the points of each adversarial cloud (at the selected distance weight) whose mean distance
to its num_knn_for_defense nearest neighbours exceeds the CLOUD's own mean + sor_alpha * standard deviation of that score are
dropped, the victim AE reconstructs what is left, and the reconstruction is scored against the clean source; the same runs on
the clean sources (the _orig half).  It is the scale-free form of run_defense_surface, whose one absolute threshold (0.04) is
tuned to the reference's ShapeNet scale.

    python -m geometric_adv_amd.run_defense_sor --ae_folder log/autoencoder_victim --do_sanity_checks 1
    python -m geometric_adv_amd.evaluate_defense --output_folder_name defense_sor_res
    python -m geometric_adv_amd.run_classifier --data_type after_defense --defense_folder defense_sor_res

Reads no kNN files: the distances are computed on the device (ops.knn_dists) and go straight into the filter
(ops.sor_filter; the rule, float64 statistics in a fixed summation order and a threshold test without a square root, is
written out in include/geoadv.h).  Everything of a class runs on the GPU from load to download.

Writes exactly the files of run_defense_surface (adversarial_critical_* and original_*critical* hold the OUTLIERS, trimmed to
the class's largest count), in <output_folder_name>/<class>/ and <output_folder_name>_orig/<class>/, and
defense_configuration.json (the attack's settings plus num_knn_for_defense and sor_alpha) in both folders; evaluate_defense and
run_classifier read them unchanged.
"""
import argparse
import math


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--num_knn_for_defense', type=int, default=2)
    p.add_argument('--sor_alpha', type=float, default=1.1)
    p.add_argument('--do_sanity_checks', type=int, default=0)
    p.add_argument('--output_folder_name', type=str, default='defense_sor_res')
    p.add_argument('--top_dir', type=str, default='.', help='root that the folder flags are relative to')
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Run defense sor flags:', flags)
    if not 1 <= flags.num_knn_for_defense <= 64:
        raise SystemExit('run_defense_sor: --num_knn_for_defense must be in [1, 64] (got %d)' % flags.num_knn_for_defense)
    if not (flags.sor_alpha >= 0 and math.isfinite(flags.sor_alpha)):
        raise SystemExit('run_defense_sor: --sor_alpha must be finite and >= 0 (got %r)' % flags.sor_alpha)
    from .defense_cli import run_defense
    run_defense(flags, 'sor')


if __name__ == '__main__':
    main()
