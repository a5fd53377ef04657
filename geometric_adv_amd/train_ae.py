"""autoencoder/train_ae.py on MI355X: trains the victim auto-encoder and writes `models.ckpt-<epoch>`
(TF V2 checkpoint format, written without TensorFlow by tf_checkpoint.py; saver_step 50 plus the first and last epoch,
autoencoder.py:213-215), `train_stats.txt` (epoch, loss, minutes: autoencoder.py:206-209) and `configuration.json` (what
tst_ae reads back: JSON where the reference pickles its Configuration) into --train_folder.

Limitation of the checkpoint: the bundle holds the 36 `autoencoder/*` model variables (weights, biases, BN parameters and
moving averages) -- exactly what the attack path restores (restore_ae_model filters the var_list by the 'autoencoder' prefix,
adversary_autoencoder.py:42-51).  It does NOT hold `autoencoder/epoch`, the Adam slots or the beta powers, so the
reference's own AutoEncoder.restore_model (neural_net.py:33-36, a Saver over ALL globals) would fail with NotFound on it:
it is a victim for the attack, not a resumable training state.  The reader / writer pair is pinned to the published format
and to its own round trip only; no TF-written bundle exists in this environment to test against.

Two sources of training clouds:
  --data_dir   the ShapeNet PLY folder (<data_dir>/<synset id>/<model>.ply), as the reference: in_out.load_dataset of
               --class_names for the train and the validation set, axes sorted on the device (--sort_axes 1), both sets
               shuffled with seed 55 when there is more than one class, batches drawn through PointCloudDataSet.next_batch, and
               every --held_out_step epochs the validation loss (mean of get_loss_per_pc over the whole batches; a set smaller
               than one batch is taken whole) appended to train_stats.txt as `On Held_Out: <epoch>\t<loss>\t<minutes>`
               (autoencoder.py:222-226).
  --train_data one `.npy` of shape (n, n_points, 3) (axes already sorted if wanted), shuffled once per epoch with numpy.
Data side (all off by default; with the defaults every path, file and bit is what it was):
  --device_data 1          the training clouds are uploaded once (device_data.DevicePointCloudDataSet) and every batch is one
                           gather launch by index; shuffles reorder a host index array.  The --train_data path replaces
                           data[perm] by that index gather.
  --gauss_augment_sigma S [--gauss_augment_mu M], --z_rotate 1, --denoising 1
                           the reference's Configuration.gauss_augment / z_rotate / denoising (src/general_utils.py:124-144,
                           src/pointnet_ae.py:116-128), applied on the device in the batch's launch.  z_rotate draws its matrix
                           from numpy's global stream as the reference does; the Gaussian noise is the device generator's
                           (csrc/dataset.hip) keyed by --seed and the batch count, so a run with noise does not advance numpy's
                           stream by the reference's np.random.normal draws and its later shuffles differ from the reference's.
                           configuration.json gains `denoising`, `z_rotate` and `gauss_augment` only when one of them is set.
Multi-GPU: launch with torchrun; every rank takes its shard of each batch and the flat gradient buffer is all-reduced (RCCL).

    python -m geometric_adv_amd.train_ae --data_dir data/shape_net_core_uniform_samples_2048 --train_folder log/autoencoder_victim
    python -m geometric_adv_amd.train_ae --train_data clouds.npy --train_folder log/autoencoder_victim --training_epochs 500
"""
import argparse
import json
import os
import os.path as osp

import numpy as np


CLASS_NAMES_13 = ['table', 'car', 'chair', 'airplane', 'sofa', 'rifle', 'lamp', 'watercraft', 'bench', 'loudspeaker', 'cabinet',
                  'display', 'telephone']                          # autoencoder/train_ae.py:49
CONFIGURATION_KEYS = ('n_input', 'loss', 'batch_size', 'learning_rate', 'training_epochs', 'saver_step', 'bneck_size',
                      'object_class', 'class_names', 'sort_axes', 'experiment_name', 'held_out_step', 'data_source')


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--training_epochs', type=int, default=500, help='Number of training epochs [default: 500]')
    p.add_argument('--train_folder', type=str, default='log/autoencoder_victim')
    p.add_argument('--train_data', type=str, default=None, help='.npy of shape (n, n_points, 3)')
    p.add_argument('--data_dir', type=str, default=None, help='ShapeNet PLY folder (<synset id>/<model>.ply); not together with --train_data')
    p.add_argument('--class_names', nargs='+', default=list(CLASS_NAMES_13), help='shape classes read from --data_dir [default: the 13 of the reference]')
    p.add_argument('--sort_axes', type=int, default=1, help='1: Sort point cloud axes, 0: Do not sort axes [default: 1] (--data_dir input only)')
    p.add_argument('--save_config_and_exit', type=int, default=0, help='1: Save autoencoder configuration and exit, 0: Do not exit [default: 0]')
    p.add_argument('--held_out_step', type=int, default=5, help='epochs between two evaluations of the validation set (--data_dir only) [default: 5]')
    p.add_argument('--batch_size', type=int, default=50)            # default_train_params, ae_templates.py:43-51
    p.add_argument('--learning_rate', type=float, default=0.0005)
    p.add_argument('--saver_step', type=int, default=50)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--device_data', type=int, default=0, help='1: keep the training clouds on the GPU and gather every batch there, 0: host batches [default: 0]')
    p.add_argument('--denoising', type=int, default=0, help='1: feed the augmented batch and take the loss against the clean one [default: 0]')
    p.add_argument('--z_rotate', type=int, default=0, help='1: one random rotation about z per batch [default: 0]')
    p.add_argument('--gauss_augment_mu', type=float, default=0.0, help='mean of the Gaussian noise added to every coordinate [default: 0]')
    p.add_argument('--gauss_augment_sigma', type=float, default=0.0, help='its standard deviation; 0: no noise [default: 0]')
    return p


def parse_flags(argv=None):
    p = build_parser()
    flags = p.parse_args(argv)
    if flags.train_data is None and flags.data_dir is None:
        p.error('one of --data_dir (ShapeNet PLY folder) and --train_data (.npy of clouds) is required')
    if flags.train_data is not None and flags.data_dir is not None:
        p.error('--data_dir and --train_data are two sources of the training clouds: give one of them')
    if flags.gauss_augment_sigma < 0:
        p.error('--gauss_augment_sigma must be >= 0')
    return flags


def make_configuration(flags, n_points):
    """The fields of the reference's Configuration (autoencoder/train_ae.py:58-78) that tst_ae and the later stages read, and
    `data_source`: 'data_dir' or 'train_data'.  The classes, object_class and sort_axes describe a PLY folder; a run on a
    `.npy` of clouds says nothing about where those came from, so they are recorded as empty / 0 and tst_ae, which would
    have to read the classes' folders, refuses such a train folder."""
    from_ply = flags.data_dir is not None
    class_names = list(flags.class_names) if from_ply else []
    conf = {'n_input': [int(n_points), 3], 'loss': 'chamfer', 'batch_size': flags.batch_size, 'learning_rate': flags.learning_rate,
            'training_epochs': flags.training_epochs, 'saver_step': flags.saver_step, 'bneck_size': 128,
            'object_class': ['%dl' % len(class_names)] if from_ply else [], 'class_names': class_names,
            'sort_axes': int(flags.sort_axes) if from_ply else 0, 'experiment_name': 'autoencoder',
            'held_out_step': flags.held_out_step, 'data_source': 'data_dir' if from_ply else 'train_data'}
    gauss = flags.gauss_augment_sigma > 0
    if gauss or flags.z_rotate or flags.denoising:     # only then: the default dictionary stays as it was
        conf.update({'denoising': bool(flags.denoising), 'z_rotate': bool(flags.z_rotate),
                     'gauss_augment': {'mu': flags.gauss_augment_mu, 'sigma': flags.gauss_augment_sigma} if gauss else None})
    return conf


def save_configuration(train_dir, conf):
    os.makedirs(train_dir, exist_ok=True)
    with open(osp.join(train_dir, 'configuration.json'), 'w') as f:
        json.dump(conf, f, indent=1, sort_keys=True)
        f.write('\n')


def load_configuration(train_dir):
    with open(osp.join(train_dir, 'configuration.json')) as f:
        conf = json.load(f)
    missing = [k for k in CONFIGURATION_KEYS if k not in conf]
    if missing:
        raise ValueError('%s lacks %s' % (osp.join(train_dir, 'configuration.json'), missing))
    return conf


def _peek_n_points(flags):
    """Points per cloud of the training data without loading them all."""
    if flags.data_dir is not None:
        from . import in_out
        class_dir = osp.join(flags.data_dir, in_out.snc_category_to_synth_id()[flags.class_names[0]])
        first = next(in_out.files_in_subdirs(class_dir, '.ply'), None)
        if first is None:
            raise FileNotFoundError('no .ply file under %s' % class_dir)
        return in_out.load_ply(first).shape[0]
    return np.load(flags.train_data, mmap_mode='r').shape[1]


def sort_axes_on_device(point_clouds, device, chunk=8192):
    """ops.sort_axes of host clouds (N, n, 3), `chunk` clouds at a time -> float32 numpy."""
    import torch
    from . import ops
    out = np.empty(point_clouds.shape, np.float32)
    for s in range(0, len(point_clouds), chunk):
        x = torch.from_numpy(np.ascontiguousarray(point_clouds[s:s + chunk], dtype=np.float32)).to(device)
        out[s:s + chunk] = ops.sort_axes(x)[0].cpu().numpy()
    return out


class _RankShard(object):
    """next_batch of a PointCloudDataSet for one rank: every rank draws the same global batch and keeps its part.  The ranks'
    copies of the set reshuffle through numpy's global generator; main() reseeds it on every rank at the start of each epoch
    when there are several ranks, so a stray draw on one rank cannot leave them apart for longer than that epoch."""

    def __init__(self, data_set, rank, world):
        self.ds, self.rank, self.world = data_set, rank, world
        self.num_examples = data_set.num_examples // world

        self.device_resident = getattr(data_set, 'device_resident', False)

    def next_batch(self, local_bs, **device_kw):
        if self.device_resident:              # the global batch is drawn, this rank's slice of it gathered
            return self.ds.next_batch(local_bs * self.world, rank_slice=(self.rank, self.world), **device_kw)
        batch, labels, noisy = self.ds.next_batch(local_bs * self.world)
        window = slice(self.rank * local_bs, (self.rank + 1) * local_bs)
        return batch[window], labels, None if noisy is None else noisy[window]


def held_out_loss(weights, n_points, val_data, batch_size, device):
    """Mean of get_loss_per_pc over the whole batches of the validation set (taken whole if it is smaller than one batch)."""
    from .autoencoder import PointNetAE
    ae = PointNetAE(weights, n_points, device=device)
    pcs = val_data.point_clouds
    n_whole = (len(pcs) // batch_size) * batch_size or len(pcs)
    per_pc = np.concatenate([ae.get_loss_per_pc(pcs[s:s + batch_size]) for s in range(0, n_whole, batch_size)])
    return float(per_pc.mean())


def main(argv=None):
    flags = parse_flags(argv)
    from . import dist as gdist
    rank = gdist.env_rank()[0]
    if rank == 0:
        save_configuration(flags.train_folder, make_configuration(flags, _peek_n_points(flags)))
    if flags.save_config_and_exit:
        return []
    import time
    import torch
    from . import tf_checkpoint
    from .trainer import PointNetAETrainer, initial_weights
    rank, world, local = gdist.init()
    device = torch.device('cuda', local)
    assert flags.batch_size % world == 0, 'batch_size must divide over the ranks'
    local_bs = flags.batch_size // world
    pc_data_train = pc_data_val = None
    if flags.data_dir is not None:
        from . import in_out
        pc_data_train, _, _ = in_out.load_dataset(flags.class_names, 'train_set', flags.data_dir)
        pc_data_val, _, _ = in_out.load_dataset(flags.class_names, 'val_set', flags.data_dir)
        if flags.sort_axes:
            pc_data_train.point_clouds = sort_axes_on_device(pc_data_train.point_clouds, device)
            if pc_data_val.num_examples:
                pc_data_val.point_clouds = sort_axes_on_device(pc_data_val.point_clouds, device)
        if len(flags.class_names) > 1:                                         # autoencoder/train_ae.py:103-105
            pc_data_train.shuffle_data(seed=55)
            pc_data_val.shuffle_data(seed=55)
        n_points = pc_data_train.n_points
        if flags.device_data:                                                  # same order, same draws from here on
            from .device_data import DevicePointCloudDataSet
            pc_data_train = DevicePointCloudDataSet(pc_data_train.point_clouds, labels=pc_data_train.labels, device=device,
                                                    init_shuffle=False)
    else:
        data = np.load(flags.train_data).astype(np.float32)
        assert data.ndim == 3 and data.shape[2] == 3, 'train_data must be (n, n_points, 3)'
        n_points = data.shape[1]
        n_batches = len(data) // flags.batch_size
        if flags.device_data:
            from .device_data import DevicePointCloudDataSet
            resident = DevicePointCloudDataSet(data, device=device, init_shuffle=False)
    tr = PointNetAETrainer(initial_weights(n_points, seed=flags.seed), n_points, batch_size=local_bs,
                           learning_rate=flags.learning_rate, device=device)
    os.makedirs(flags.train_folder, exist_ok=True)
    fout = open(osp.join(flags.train_folder, 'train_stats.txt'), 'a', 1) if rank == 0 else None
    rng = np.random.default_rng(flags.seed)
    augment = None
    if flags.gauss_augment_sigma > 0 or flags.z_rotate:
        from .device_data import Augmentation
        augment = Augmentation(flags.gauss_augment_mu, flags.gauss_augment_sigma, z_rotate=bool(flags.z_rotate), seed=flags.seed)
        if flags.z_rotate and pc_data_train is None:
            np.random.seed(flags.seed)                                             # the rotations' stream (the ranks draw alike)
    how = dict(augment=augment, denoising=bool(flags.denoising))
    stats = []
    for epoch in range(1, flags.training_epochs + 1):
        if pc_data_train is not None:
            if world > 1:
                np.random.seed(flags.seed + epoch)                                 # the ranks must reshuffle alike
            loss, duration = tr._single_epoch_train(_RankShard(pc_data_train, rank, world), **how)
        else:
            perm = rng.permutation(len(data))[:n_batches * flags.batch_size]       # same permutation on every rank
            if flags.device_data:
                shard = resident.set_order(perm.reshape(n_batches, world, local_bs)[:, rank].reshape(-1))
            else:
                shard = data[perm].reshape(n_batches, world, local_bs, n_points, 3)[:, rank].reshape(-1, n_points, 3)
            loss, duration = tr._single_epoch_train(shard, **how)
        stats.append((epoch, loss, duration))
        if rank == 0:
            print("Epoch:", '%04d' % epoch, 'training time (minutes)=', "{:.4f}".format(duration / 60.0), "loss=", "{:.9f}".format(loss))
            fout.write('%04d\t%.9f\t%.4f\n' % (epoch, loss, duration / 60.0))
            if epoch % flags.saver_step == 0 or epoch == 1 or epoch == flags.training_epochs:
                tf_checkpoint.write_checkpoint(osp.join(flags.train_folder, 'models.ckpt-%d' % epoch), tr.export_weights())
            if pc_data_val is not None and pc_data_val.num_examples and flags.held_out_step > 0 and epoch % flags.held_out_step == 0:
                start = time.time()
                val_loss = held_out_loss(tr.export_weights(), n_points, pc_data_val, flags.batch_size, device)
                duration = time.time() - start
                print('validation set after epoch %04d: loss %.9f (%.4f minutes)' % (epoch, val_loss, duration / 60.0))
                fout.write('On Held_Out: %04d\t%.9f\t%.4f\n' % (epoch, val_loss, duration / 60.0))
    if fout:
        fout.close()
    return stats


if __name__ == '__main__':
    main()
