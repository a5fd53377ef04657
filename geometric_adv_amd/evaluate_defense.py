"""defender/evaluate_defense.py, without its plots: the defense table.  For every attack, at the distance weight, target
instance and target class evaluate_attack selected, the source reconstruction error (S-RE) and its ratio to the clean
source's (S-NRE) after the defense and before it, and the reference's text reports over all classes.  numpy only: no GPU.

    python -m geometric_adv_amd.evaluate_defense --ae_folder log/autoencoder_victim --output_folder_name defense_surface_res

Reads <eval>/<attack_folder>/attack_configuration.json, pc_classes* and ae_loss_test_set* of the eval folder, per attacked
class dist_weight.npy and analysis_results/source_target_norm_min*_idx.npy (evaluate_attack), and from
<attack_folder>/<output_folder_name>/ (run_defense_surface / run_defense_critical) defense_configuration.json and
<class>/defense_metrics.npy [1 or W, n_attacks, 4]: defended S-RE, defended S-NRE, adversarial S-RE, adversarial S-NRE.  With
--use_adversarial_data 0 the folder is <output_folder_name>_orig and the file defense_source_metrics.npy [n_attacks, 4] (the
defense applied to the clean source), repeated for every distance weight.

Writes, under <that folder>/over_classes/: targeted_attacks.txt, untargeted_attacks.txt and eval_stats.txt; with
--use_params_for_stat_file_name 1 and a defense configuration that holds num_knn_for_defense and knn_dist_thresh (the surface
defense), *_k_<num_knn_for_defense>_th_<knn_dist_thresh, two decimals>.txt.  The statistics follow
src/adversary_utils.py:222-257.

Two quirks of the reference are kept, because the texts are pinned to its own byte for byte:
  - the per-target-class lines of a shape class go into the UNTARGETED file, before that class's "Shape class" header, with
    the labels "tra T-RE / tra T-NRE / adv T-RE / adv T-NRE" (evaluate_defense.py:274),
  - so targeted_attacks.txt holds the class headers only.

Differences forced by the environment, as in evaluate_attack:
  - the configurations are read from attack_configuration.json and defense_configuration.json,
  - --save_graphs 1 and --save_pc_plots 1 are refused: they draw with matplotlib and seaborn, which this project does not use,
  - --do_sanity_checks is accepted and has no effect: in the reference it only acts inside the plot branch,
  - what the reference loads for its plots only is not read: the clouds, the neighbour indices, --attack_pc_idx, the critical
    points, the defended clouds and the prediction labels.
"""
import argparse
import json
import os.path as osp

import numpy as np

LINE_LABELS_TARGETED = ('tra T-RE', 'tra T-NRE', 'adv T-RE', 'adv T-NRE')
LINE_LABELS_UNTARGETED = ('def S-RE', 'def S-NRE', 'adv S-RE', 'adv S-NRE')
HEADING = ('Shape\t\tDef\t\tDef\t\tAdv\t\tAdv\n', 'Class\t\tS-RE\t\tS-NRE\t\tS-RE\t\tS-NRE\n')


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--do_sanity_checks', type=int, default=0, help='accepted; acts only on the plots, which are left out')
    p.add_argument('--output_folder_name', type=str, default='defense_critical_res')
    p.add_argument('--use_adversarial_data', type=int, default=1)
    p.add_argument('--use_params_for_stat_file_name', type=int, default=0)
    p.add_argument('--save_graphs', type=int, default=0)
    p.add_argument('--save_pc_plots', type=int, default=0)
    p.add_argument('--top_dir', type=str, default='.', help='root that --ae_folder is relative to')
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    from . import _report as R
    R.refuse_plots('evaluate_defense', flags)
    print('Evaluate defense flags:', flags)

    attack_path, conf, pc_classes = R.load_attack(flags.top_dir, flags.ae_folder, flags.attack_folder)
    output_path = osp.join(attack_path, flags.output_folder_name + ('' if flags.use_adversarial_data else '_orig'))
    conf_file = osp.join(output_path, 'defense_configuration.json')
    if not osp.exists(conf_file):
        raise SystemExit('evaluate_defense: %s is missing: run geometric_adv_amd.run_defense_surface or '
                         'geometric_adv_amd.run_defense_critical with --output_folder_name %s first'
                         % (conf_file, flags.output_folder_name))
    with open(conf_file) as f:
        def_conf = json.load(f)

    suffix = ''
    if flags.use_params_for_stat_file_name and def_conf.get('num_knn_for_defense') is not None \
            and def_conf.get('knn_dist_thresh') is not None:
        suffix = '_k_%d_th_%.2f' % (def_conf['num_knn_for_defense'], def_conf['knn_dist_thresh'])
    names = [base + suffix + '.txt' for base in ('targeted_attacks', 'untargeted_attacks', 'eval_stats')]

    def metrics_of_class(name, num_dist_weight):
        if flags.use_adversarial_data:
            return R.over_weights(np.load(osp.join(output_path, name, 'defense_metrics.npy')), num_dist_weight)
        source = np.load(osp.join(output_path, name, 'defense_source_metrics.npy'))
        return np.vstack([np.expand_dims(source, axis=0)] * num_dist_weight)

    R.report(attack_path, conf, pc_classes, metrics_of_class, (1, 'def', LINE_LABELS_TARGETED),
             (1, 'def', LINE_LABELS_UNTARGETED), HEADING, osp.join(output_path, 'over_classes'), names)


if __name__ == '__main__':
    main()
