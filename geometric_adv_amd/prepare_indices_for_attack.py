"""attacker/prepare_indices_for_attack.py on MI355X: the three index files the attack and everything after it
read from the victim's eval folder.  Same flags, files and stage order as the reference (:28-39,183-200):

  --get_rand_idx 1        sel_idx_rand_<num>_<set>.npy (:70-86), int16 [classes, --num_instance_per_class]: per class the first
                          entries of a seed-55 shuffle of its instances, -1 where the class is smaller.  The default
                          --attack_pc_idx of every later command.  Host only.
  --get_latent_nn_idx 1   latent_dist_mat_<set>.npy, the float32 Euclidean distances between the latent codes of the test set
                          (:89-101; ops.latent_dist_matrix, the reference's bits; --device cpu: scorer.latent_dist_mat_host), and
                          latent_nn_idx_<set>.npy = sort_dist_mat(...): target_pc_idx_type 'latent_nn'.
  --get_chamfer_nn_idx 1  the all-pairs Chamfer distance matrix of the test set and the per-class-pair neighbour order the
                          attack picks its targets from (target_pc_idx_type 'chamfer_nn_complete').

--get_chamfer_nn_idx (:32-36,104-164): every call fills columns [pc_start_idx, pc_start_idx +
pc_batch_size) of chamfer_dist_mat_complete_<set>.npy (created with -1 on the first call) and, once no -1 is left, writes
chamfer_nn_idx_complete_<set>.npy = sort_dist_mat(...).  The reference needs 44 processes of 100 columns each
(runner_indices_for_attack.sh:11-15); here --pc_batch_size may simply be the whole set, or the slices may be dealt over
ranks with scorer.get_chamfer_dist_mat_sharded.

    python -m geometric_adv_amd.prepare_indices_for_attack --ae_folder log/autoencoder_victim --get_rand_idx 1 \
        --get_latent_nn_idx 1 --get_chamfer_nn_idx 1 --pc_batch_size 100000
"""
import argparse
import os
import os.path as osp
import time

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--ae_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--get_rand_idx', type=int, default=0)
    p.add_argument('--get_latent_nn_idx', type=int, default=0)
    p.add_argument('--get_chamfer_nn_idx', type=int, default=0)
    p.add_argument('--num_instance_per_class', type=int, default=100)
    p.add_argument('--pc_start_idx', type=int, default=0)
    p.add_argument('--pc_batch_size', type=int, default=100)
    p.add_argument('--top_dir', type=str, default='.')
    p.add_argument('--device', type=str, default='cuda:0')
    return p


SEED = 55       # :67


def _eval_files(flags):
    """-> (eval folder, its files, the last three parts of the slice_idx file name, e.g. test_set_13l.npy (:58-59))."""
    data_path = osp.join(flags.top_dir, flags.ae_folder, 'eval')
    files = [f for f in os.listdir(data_path) if osp.isfile(osp.join(data_path, f))]
    return data_path, files, [f for f in files if 'slice_idx_test_set' in f][0].split('_')[-3:]


def get_rand_idx(flags):
    from .attack_data import load_data
    data_path, files, parts = _eval_files(flags)
    pc_classes, slice_idx = load_data(data_path, files, ['pc_classes', 'slice_idx_test_set'])
    num = flags.num_instance_per_class
    sel_idx = -1 * np.ones([len(pc_classes), num], dtype=np.int16)
    for i in range(len(pc_classes)):
        np.random.seed(SEED)                    # per class, as the reference: classes of one size get one permutation
        num_examples = slice_idx[i + 1] - slice_idx[i]
        perm = np.arange(num_examples)
        np.random.shuffle(perm)
        sel_idx[i, :min(num, num_examples)] = perm[:num]
    np.save(osp.join(data_path, '_'.join(['sel_idx', 'rand', '%d' % num] + parts)), sel_idx)


def get_latent_nn(flags):
    from .attack_data import load_data
    from .scorer import get_latent_dist_mat, latent_dist_mat_host, sort_dist_mat
    data_path, files, parts = _eval_files(flags)
    latent_vectors, slice_idx = load_data(data_path, files, ['latent_vectors_test_set', 'slice_idx_test_set'])
    if str(flags.device).startswith('cpu'):
        mat = latent_dist_mat_host(latent_vectors)
    else:
        mat = get_latent_dist_mat(latent_vectors, flags.device)
    assert np.array_equal(mat, mat.T), 'The distance matrix should be a symmetric matrix!'      # general_utils.py:104
    np.save(osp.join(data_path, '_'.join(['latent_dist_mat'] + parts)), mat)
    np.save(osp.join(data_path, '_'.join(['latent_nn_idx'] + parts)), sort_dist_mat(mat, slice_idx))


def get_chamfer_nn(flags):
    from .attack_data import load_data
    from .scorer import get_chamfer_dist_mat_slice, sort_dist_mat
    start_time = time.time()
    data_path = osp.join(flags.top_dir, flags.ae_folder, 'eval')
    files = [f for f in os.listdir(data_path) if osp.isfile(osp.join(data_path, f))]
    point_clouds, slice_idx = load_data(data_path, files, ['point_clouds_test_set', 'slice_idx_test_set'])
    parts = [f for f in files if 'slice_idx_test_set' in f][0].split('_')[-3:]              # e.g. test_set_13l.npy (:58-59)
    n_all = len(point_clouds)
    if flags.pc_start_idx == 0 and flags.pc_batch_size >= n_all:        # the whole matrix at once: half the work (symmetry)
        from .scorer import get_chamfer_dist_mat_full
        cur = get_chamfer_dist_mat_full(point_clouds, flags.device)
    else:
        cur = get_chamfer_dist_mat_slice(point_clouds, flags.pc_start_idx, flags.pc_batch_size, flags.device)
    assert cur.min() >= 0, 'the chamfer_dist_mat_curr matrix was not filled correctly'
    mat_path = osp.join(data_path, '_'.join(['chamfer_dist_mat_complete'] + parts))
    mat = np.load(mat_path) if osp.exists(mat_path) else -1 * np.ones([n_all, n_all], dtype=np.float32)
    mat[:, flags.pc_start_idx:flags.pc_start_idx + flags.pc_batch_size] = cur
    np.save(mat_path, mat)
    print('start index %d end index %d, out of size %d, duration (minutes): %.2f' %
          (flags.pc_start_idx, min(flags.pc_start_idx + flags.pc_batch_size, n_all), n_all, (time.time() - start_time) / 60.0))
    if mat.min() >= 0:
        np.save(osp.join(data_path, '_'.join(['chamfer_nn_idx_complete'] + parts)), sort_dist_mat(mat, slice_idx))


def main(argv=None):
    flags = build_parser().parse_args(argv)
    if flags.get_rand_idx:
        get_rand_idx(flags)
    if flags.get_latent_nn_idx:
        get_latent_nn(flags)
    if flags.get_chamfer_nn_idx:
        get_chamfer_nn(flags)


if __name__ == '__main__':
    main()
