"""transfer/atlasnet/train.py for the point-cloud auto-encoder on the MI355X: the reference's flags as far as they apply, the
same per-epoch loop (training, then test_epoch in eval mode) and the same files in --dir_name after every epoch: a
`json_stats:` line appended to log.txt, options.json (with start_epoch = epochs finished), network.pth and optimizer.pth,
which AtlasNetAE and run_transfer --transfer_ae_type AtlasNet read back.  Paths are relative to --top_dir.

    python -m geometric_adv_amd.train_atlasnet --dir_name log/atlasnet_ae --nb_primitives 25 --template_type SQUARE \\
        --custom_data --no_metro --train_pc_path data/train.npy --eval_pc_path data/val.npy

A rerun in a folder that holds network.pth resumes from it (weights, running statistics, Adam's state, learning rate, epoch).
At epochs --lr_decay_1/2/3 the learning rate is divided by 10 and a NEW Adam starts, as the reference does.  Left out:
SPHERE, SVR, metro, visdom and the HTML report.  The epoch's shuffle is numpy's, seeded by --seed; the
last, partial batch of an epoch is trained at its own size if it holds at least 2 clouds, else dropped.

The data side (dataset/pointcloud_processor.py, dataset/augmenter.py, dataset_shapenet.py:213-215) runs on the GPU.  With
--normalization UnitBall / BoundingBox, --sample_points K or any of the reference's augmentation flags (--random_rotation,
--data_augmentation_axis_rotation, --data_augmentation_random_flips, --random_translation, --anisotropic_scaling) both sets are
uploaded once and normalised once (ops.normalize_clouds), and every training batch is ONE ops.augment_batch launch: gather,
K points drawn with replacement, the Augmenter's operators in its order.  The draws are keyed by (--seed, the number of
training steps taken in all, the cloud's slot in the batch), so a resumed run continues the stream; they are the device
generator's, with the reference's distributions and not torch's numbers.  The evaluation set is normalised and, with
--sample_points, sampled once under a fixed key, and never augmented: loss_val is comparable across epochs.  The shuffle
stream is the same with or without these flags, and with none of them the run is the host path, unchanged.
--normalization defaults to Identity, not to the reference's UnitBall: the reference normalises only its ShapeNet cache,
never the clouds of --custom_data (dataset_shapenet.py), and this command is always custom data.
"""
import argparse
import json
import os
import os.path as osp

import numpy as np

FSCORE_THRESHOLD = 0.001


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--dir_name', type=str, default='log/atlasnet_ae')
    p.add_argument('--nb_primitives', type=int, default=1)
    p.add_argument('--template_type', type=str, default='SQUARE', choices=['SQUARE', 'SPHERE'])
    p.add_argument('--num_layers', type=int, default=2)
    p.add_argument('--number_points', type=int, default=2500, help='template points per reconstruction in training')
    p.add_argument('--number_points_eval', type=int, default=2500)
    p.add_argument('--batch_size', type=int, default=32,
                   help='batch size (>= 2: bn4 and bn5 take their statistics over the batch).  The last, partial batch of an '
                        'epoch is trained at its own size if it holds at least 2 clouds, else dropped')
    p.add_argument('--batch_size_test', type=int, default=32)
    p.add_argument('--nepoch', type=int, default=150)
    p.add_argument('--lrate', type=float, default=0.001)
    p.add_argument('--lr_decay_1', type=int, default=120)
    p.add_argument('--lr_decay_2', type=int, default=140)
    p.add_argument('--lr_decay_3', type=int, default=145)
    p.add_argument('--loop_per_epoch', type=int, default=1, help='passes over the training set per epoch')
    p.add_argument('--remove_all_batchNorms', action='store_true', help='no batch norm in the decoder')
    p.add_argument('--custom_data', action='store_true', help='accepted; always on: the clouds come from the two .npy files')
    p.add_argument('--no_metro', action='store_true', help='accepted; always on')
    p.add_argument('--train_pc_path', type=str, required=True, help='.npy (clouds, points, 3)')
    p.add_argument('--eval_pc_path', type=str, required=True, help='.npy (clouds, points, 3)')
    p.add_argument('--top_dir', type=str, default='.', help='root that the path flags are relative to')
    p.add_argument('--seed', type=int, default=0, help='initial weights, the shuffles, the template generator and the augmentation draws')
    p.add_argument('--normalization', type=str, default='Identity', choices=['Identity', 'UnitBall', 'BoundingBox'],
                   help='both sets are normalised once on the GPU.  [default: Identity -- the reference\'s UnitBall default only '
                        'ever touches its ShapeNet cache, never --custom_data clouds, and this command is always custom data]')
    p.add_argument('--sample_points', type=int, default=0,
                   help='K > 0: every training cloud of a batch is K points drawn with replacement from the file\'s cloud (which may '
                        'hold more, e.g. 30000), and the evaluation clouds are K points drawn once.  [default: 0 = off]')
    p.add_argument('--random_rotation', action='store_true', help='apply data augmentation : random rotation')
    p.add_argument('--data_augmentation_axis_rotation', action='store_true', help='apply data augmentation : random rotation about axis 1')
    p.add_argument('--data_augmentation_random_flips', action='store_true', help='apply data augmentation : random flips of the axes 0 and 2')
    p.add_argument('--random_translation', action='store_true', help='apply data augmentation : random translation')
    p.add_argument('--anisotropic_scaling', action='store_true', help='apply data augmentation : anisotropic scaling')
    return p


EVAL_SAMPLE_COUNTER = (1 << 64) - 1     # the fixed key of the evaluation set's sampling: no step counter reaches it


def augmenter_of(flags):
    """The device_data.CloudAugmenter of the reference's augmentation flags (training/trainer.py:60-62)."""
    from .device_data import CloudAugmenter
    return CloudAugmenter(translation=flags.random_translation, rotation_axis=(1,) if flags.data_augmentation_axis_rotation else (),
                          rotation_3D=flags.random_rotation, anisotropic_scaling=flags.anisotropic_scaling,
                          flips=(0, 2) if flags.data_augmentation_random_flips else (), seed=flags.seed)


def fscore(dist1, dist2, threshold=FSCORE_THRESHOLD):
    """auxiliary/ChamferDistancePytorch/fscore.py: per cloud, from the squared nearest-neighbour distances of both directions."""
    p1 = (dist1 < threshold).float().mean(dim=1)
    p2 = (dist2 < threshold).float().mean(dim=1)
    f = 2 * p1 * p2 / (p1 + p2)
    f[f != f] = 0
    return f


def test_epoch(trainer, clouds, batch_size):
    """The reference's test_epoch: eval mode on every cloud; (loss_val, fscore), each the mean over the batches."""
    import torch
    from . import ops
    ae = trainer.eval_model()
    losses, scores = [], []
    for s in range(0, len(clouds), batch_size):
        x = torch.as_tensor(clouds[s:s + batch_size]).to(ae.device)
        _, recon = ae.forward(x)
        d1, _, d2, _ = ops.nn_distance(x, recon)
        losses.append(float(d1.mean() + d2.mean()))
        scores.append(float(fscore(d1, d2).mean()))
    return float(np.mean(losses)), float(np.mean(scores))


def main(argv=None):
    flags = build_parser().parse_args(argv)
    from . import atlas_weights as AW
    from .atlas_trainer import AtlasNetTrainer, check_batch
    check_batch(flags.batch_size)
    print('Train AtlasNet flags:', flags)
    top = flags.top_dir
    train = np.load(osp.join(top, flags.train_pc_path)).astype(np.float32)
    val = np.load(osp.join(top, flags.eval_pc_path)).astype(np.float32)
    folder = osp.join(top, flags.dir_name)
    options = dict(nb_primitives=flags.nb_primitives, template_type=flags.template_type, num_layers=flags.num_layers,
                   number_points=flags.number_points, number_points_eval=flags.number_points_eval,
                   remove_all_batchNorms=bool(flags.remove_all_batchNorms))
    AW.check_options(AW.options(None, options))
    lrate, start_epoch = flags.lrate, 0
    resume = osp.exists(osp.join(folder, 'network.pth'))
    if resume:
        saved = AW.options(folder)
        lrate, start_epoch = float(saved.get('lrate', lrate)), int(saved.get('start_epoch', 0))
        print('resuming from %s at epoch %d, learning rate %g' % (folder, start_epoch, lrate))
    B, n = flags.batch_size, train.shape[1]
    if flags.sample_points < 0:
        raise ValueError("--sample_points must be >= 0, got %d" % flags.sample_points)
    augmenter, K = augmenter_of(flags), flags.sample_points
    on_device = augmenter.active or K > 0 or flags.normalization != 'Identity'
    if on_device:
        import torch
        from . import ops
        device = torch.device("cuda:0")
        train_dev = ops.normalize_clouds(torch.from_numpy(train).to(device), flags.normalization)
        val = ops.normalize_clouds(torch.from_numpy(val).to(device), flags.normalization)
        if K > 0:
            val = ops.augment_batch(val, None, dict(seed=flags.seed % (1 << 64), counter=EVAL_SAMPLE_COUNTER, sample=1), n_out=K)
            n = K
    trainers, current = {}, None     # one handle per batch size (the full one and the epoch's last, partial one)

    def trainer(size):
        """The handle of this batch size, brought to the state of the one that stepped last."""
        nonlocal current
        if size not in trainers or (current is not None and current is not trainers[size]):
            kw = dict(num_points=n, batch_size=size, seed=flags.seed)
            if current is not None:
                step, tracked = current.counters()
                trainers[size] = AtlasNetTrainer(weights=current.export_state_dict(), options=options, learning_rate=current.learning_rate,
                                                 step=step, slots=current.slots(), tracked=tracked, **kw)
            elif resume:
                trainers[size] = AtlasNetTrainer.restore(folder, options=options, learning_rate=lrate, **kw)
            else:
                trainers[size] = AtlasNetTrainer(options=options, learning_rate=lrate, **kw)
        current = trainers[size]
        return current

    rng = np.random.RandomState(flags.seed)
    for _ in range(start_epoch * flags.loop_per_epoch):       # a resumed run continues the interrupted run's sequence of shuffles
        rng.permutation(len(train))
    for epoch in range(start_epoch, flags.nepoch):
        if epoch in (flags.lr_decay_1, flags.lr_decay_2, flags.lr_decay_3):
            lrate = lrate / 10.0
            print('learning rate decay %g: a new Adam' % lrate)
            trainer(min(B, len(train))).set_learning_rate(lrate, reset_optimizer=True)
        losses = []
        for _ in range(flags.loop_per_epoch):
            order = rng.permutation(len(train))
            for i, s in enumerate(range(0, len(order), B)):
                idx = order[s:s + B]
                if len(idx) < 2:
                    break
                if on_device:
                    handle = trainer(len(idx))
                    batch = augmenter(train_dev, idx, counter=handle.counters()[1], sample_points=K)
                    loss = handle.train_step(batch)
                else:
                    loss = trainer(len(idx)).train_step(train[idx])
                losses.append(loss)
                print('[%d: %d/%d] chamfer train loss: %f' % (epoch, i, len(order) // B, loss))
        loss_val, fs = test_epoch(current, val, flags.batch_size_test)
        stats = {'epoch': epoch + 1, 'lr': lrate, 'loss_train_total': float(np.mean(losses)), 'loss_val': loss_val, 'fscore': fs}
        print(stats)
        os.makedirs(folder, exist_ok=True)
        with open(osp.join(folder, 'log.txt'), 'a') as f:
            f.write('json_stats: ' + json.dumps(stats) + '\n')
        extra = dict(vars(flags), lrate=lrate, start_epoch=epoch + 1)
        current.save(folder, extra_options=extra)
        print('saved', folder)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
