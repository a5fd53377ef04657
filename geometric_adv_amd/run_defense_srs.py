"""Simple random sampling (SRS) as a defense, on MI355X: the other baseline of the point-cloud attack literature, which the
reference does not have.  For every attacked class, drop_num points of each adversarial cloud (at the selected distance weight)
are dropped at random, the victim AE reconstructs what is left, and the reconstruction is scored against the clean source; the
same runs on the clean sources (the _orig half).

    python -m geometric_adv_amd.run_defense_srs --ae_folder log/autoencoder_victim --drop_num 500 --seed 0
    python -m geometric_adv_amd.evaluate_defense --output_folder_name defense_srs_res
    python -m geometric_adv_amd.run_classifier --data_type after_defense --defense_folder defense_srs_res

The draw is counter-based (ops.random_drop; the rule is written out in include/geoadv.h) and does not touch torch's or numpy's
generators: a class passes its position in pc_classes as the counter, row r of the adversarial half is slot r and row r of the
_orig half slot (number of rows + r).  A rerun with the same --seed therefore writes the same bytes, whatever ran before it.

Writes exactly the files of run_defense_surface, in <output_folder_name>/<class>/ and <output_folder_name>_orig/<class>/:
adversarial_critical_points [1, n, drop_num, 3] / adversarial_critical_idx [1, n, drop_num] int16 hold the DROPPED points
(ascending indices), adversarial_critical_num [1, n] int16 is drop_num throughout (original_* likewise), and
defense_configuration.json (the attack's settings plus drop_num and seed) in both folders; evaluate_defense and run_classifier
read them unchanged.
"""
import argparse


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--drop_num', type=int, default=500)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--do_sanity_checks', type=int, default=0)
    p.add_argument('--output_folder_name', type=str, default='defense_srs_res')
    p.add_argument('--top_dir', type=str, default='.', help='root that the folder flags are relative to')
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Run defense srs flags:', flags)
    if flags.drop_num < 0:
        raise SystemExit('run_defense_srs: --drop_num must be >= 0 (got %d)' % flags.drop_num)
    if not 0 <= flags.seed < 1 << 64:
        raise SystemExit('run_defense_srs: --seed must be in [0, 2^64) (got %d)' % flags.seed)
    from .defense_cli import run_defense
    run_defense(flags, 'srs')


if __name__ == '__main__':
    main()
