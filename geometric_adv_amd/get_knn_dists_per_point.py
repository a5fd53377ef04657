"""defender/get_knn_dists_per_point.py on MI355X: for every attacked class, the distances from every point to its num_knn
nearest neighbours (self excluded) in the adversarial clouds at the selected distance weight and in their clean sources --
the input of run_defense_surface.

    python -m geometric_adv_amd.get_knn_dists_per_point --ae_folder log/autoencoder_victim --num_knn 8

Writes, per class:
  - <eval>/<attack_folder>/<output_folder_name>/<class>/knn_dists_adversarial_pc_input.npy   [1, num_pc, N, num_knn] float32,
  - <eval>/<attack_folder>/<output_folder_name>_orig/<class>/knn_dists_source_pc.npy         [num_pc, N, num_knn] float32.
One launch of the fused kNN kernel (ops.knn_dists, csrc/grouping.hip) serves a whole class's clouds, which go to the GPU once.

Differences forced by the environment:
  - the attack's settings come from <eval>/<attack_folder>/attack_configuration.json, written by run_attack (the reference
    unpickles a Configuration, which needs tflearn),
  - --use_tf_knn 1 (the reference's TF grouping graph) and --use_tf_knn 0 (its numpy sort of the distance matrix) both give
    the kernel's values: the kernel is pinned bit for bit to goldens made from the reference's TF grouping graph
    (tests/golden/grouping.npz), and its CPU restatement agrees with the numpy path to float rounding (the CPU golden
    tests of the grouping ops),
  - the distance weight of every attack comes from analysis_results/source_target_norm_min_idx.npy (evaluate_attack); without
    it, an attack run with a single distance weight uses weight 0 (what that file would hold), one with several is refused.
"""
import argparse
import os.path as osp
import time

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--attack_pc_idx', type=str, default='log/autoencoder_victim/eval/sel_idx_rand_100_test_set_13l.npy')
    p.add_argument('--attack_folder', type=str, default='attack_res')
    p.add_argument('--num_knn', type=int, default=8)
    p.add_argument('--use_tf_knn', type=int, default=1, help='accepted for the reference; both values run the same kernel')
    p.add_argument('--output_folder_name', type=str, default='defense_surface_res')
    p.add_argument('--top_dir', type=str, default='.', help='root that the folder flags are relative to')
    p.add_argument('--device', type=str, default='cuda:0')
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Get knn dists flags:', flags)
    import torch
    from . import ops
    from .attack_data import create_dir
    from .defense_cli import AttackFolder

    folder = AttackFolder(flags.top_dir, flags.ae_folder, flags.attack_folder, flags.attack_pc_idx, ['point_clouds_test_set'])
    output_path = create_dir(osp.join(folder.attack_dir, flags.output_folder_name))
    output_path_orig = create_dir(osp.join(folder.attack_dir, flags.output_folder_name + '_orig'))
    dev = torch.device(flags.device)
    for i, name in folder.attacked():
        print('compute knn dists for shape class %s (%d out of %d classes) ' % (name, i + 1, len(folder.pc_classes)))
        start = time.time()
        source_pc, _ = folder.prep(i, 'point_clouds_test_set')
        adversarial_pc_input, = folder.selected(name, ['adversarial_pc_input'])
        adv = torch.from_numpy(np.ascontiguousarray(adversarial_pc_input[0], dtype=np.float32)).to(dev)
        src = torch.from_numpy(np.ascontiguousarray(source_pc, dtype=np.float32)).to(dev)
        knn_adv = ops.knn_dists(adv, flags.num_knn)
        knn_src = ops.knn_dists(src, flags.num_knn)
        np.save(osp.join(create_dir(osp.join(output_path, name)), 'knn_dists_adversarial_pc_input'), knn_adv.cpu().numpy()[None])
        np.save(osp.join(create_dir(osp.join(output_path_orig, name)), 'knn_dists_source_pc'), knn_src.cpu().numpy())
        print('Duration (minutes): %.2f' % ((time.time() - start) / 60.0))


if __name__ == '__main__':
    main()
