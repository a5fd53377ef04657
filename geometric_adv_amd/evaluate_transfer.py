"""transfer/evaluate_transfer.py, without its plots: the transfer table.  For every attack, at the distance weight, target
instance and target class evaluate_attack selected on the victim, the target reconstruction error (T-RE) and its ratio to
the clean target's (T-NRE) on the other auto-encoder and on the victim, and the reference's text reports over all classes.
numpy only: no GPU.

    python -m geometric_adv_amd.evaluate_transfer --transfer_ae_folder log/atlasnet_ae --ae_folder log/autoencoder_victim

Reads, from the victim's eval folder, <attack_folder>/attack_configuration.json, pc_classes*, ae_loss_test_set* and per
attacked class dist_weight.npy and analysis_results/source_target_norm_min*_idx.npy (evaluate_attack); from
<transfer_ae_folder>/eval/<output_folder_name>/<class>/ (run_transfer) transfer_metrics.npy [1 or W, n_attacks, 4]:
transferred T-RE, transferred T-NRE, adversarial T-RE, adversarial T-NRE.  Writes targeted_attacks.txt,
untargeted_attacks.txt and eval_stats.txt under <transfer_ae_folder>/eval/<output_folder_name>/over_classes/; the statistics
follow src/adversary_utils.py:260-295.

Two quirks of the reference are kept, because the texts are pinned to its own byte for byte:
  - the targeted lines are named def_<class>_<j>_target_<class>_<t> and labelled "tra T-RE / def S-NRE / adv S-RE / adv S-NRE"
    (evaluate_transfer.py:232-235), though their columns are the four T- quantities above,
  - the untargeted lines are named tra_... and carry the "tra T-RE / tra T-NRE / adv T-RE / adv T-NRE" labels.

Differences forced by the environment, as in evaluate_attack:
  - the attack's settings are read from attack_configuration.json,
  - --save_graphs 1 and --save_pc_plots 1 are refused: they draw with matplotlib and seaborn, which this project does not use,
  - what the reference loads for its plots only is not read: the clouds, the neighbour indices, --attack_pc_idx, the
    prediction labels and transferred_pc_recon.npy.
"""
import argparse
import os.path as osp

import numpy as np

LINE_LABELS_TARGETED = ('tra T-RE', 'def S-NRE', 'adv S-RE', 'adv S-NRE')
LINE_LABELS_UNTARGETED = ('tra T-RE', 'tra T-NRE', 'adv T-RE', 'adv T-NRE')
HEADING = ('Shape\t\tTra\t\tTra\t\tAdv\t\tAdv\n', 'Class\t\tT-RE\t\tT-NRE\t\tT-RE\t\tT-NRE\n')
NAMES = ('targeted_attacks.txt', 'untargeted_attacks.txt', 'eval_stats.txt')


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--transfer_ae_folder', type=str, default='log/autoencoder_for_transfer')
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--output_folder_name', type=str, default='attack_res_transfer')
    p.add_argument('--save_graphs', type=int, default=0)
    p.add_argument('--save_pc_plots', type=int, default=0)
    p.add_argument('--top_dir', type=str, default='.', help='root that the folder flags are relative to')
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    from . import _report as R
    R.refuse_plots('evaluate_transfer', flags)
    print('Evaluate transfer flags:', flags)

    attack_path, conf, pc_classes = R.load_attack(flags.top_dir, flags.ae_folder, flags.attack_folder)
    output_path = osp.join(flags.top_dir, flags.transfer_ae_folder, 'eval', flags.output_folder_name)
    if not osp.isdir(output_path):
        raise SystemExit('evaluate_transfer: %s is missing: run geometric_adv_amd.run_transfer with --transfer_ae_folder %s '
                         '--output_folder_name %s first' % (output_path, flags.transfer_ae_folder, flags.output_folder_name))

    def metrics_of_class(name, num_dist_weight):
        return R.over_weights(np.load(osp.join(output_path, name, 'transfer_metrics.npy')), num_dist_weight)

    R.report(attack_path, conf, pc_classes, metrics_of_class, (0, 'def', LINE_LABELS_TARGETED),
             (1, 'tra', LINE_LABELS_UNTARGETED), HEADING, osp.join(output_path, 'over_classes'), NAMES)


if __name__ == '__main__':
    main()
