"""transfer/foldingnet/train_foldingnet.py on the MI355X: the reference's flags and defaults, the same per-epoch loop and
the same files in --outf: checkpoint_<epoch>.pth after every epoch ({'epoch', 'model', 'optimizer'}), which FoldingNetAE and
run_transfer --transfer_ae_type FoldingNet read back.  Paths are relative to --top_dir.

    python -m geometric_adv_amd.train_foldingnet --outf log/foldingnet --nepoch 25 --graph_seed 7

Left out: the plots and --workers (the data is one array in memory).  The epoch's shuffle is numpy's, seeded by --seed.
"""
import argparse
import os.path as osp

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--training_set', type=str, default='log/autoencoder_victim/eval_train/point_clouds_train_set_13l.npy')
    p.add_argument('--validation_set', type=str, default='log/autoencoder_victim/eval_val/point_clouds_val_set_13l.npy')
    p.add_argument('--batchSize', type=int, default=8,
                   help='batch size (>= 2: bn6 takes its statistics over the batch).  The last, partial batch of an epoch is '
                        'trained at its own size if it holds at least 2 clouds, else dropped')
    p.add_argument('--num_points', type=int, default=2048)
    p.add_argument('--nepoch', type=int, default=25)
    p.add_argument('--outf', type=str, default='log/foldingnet')
    p.add_argument('--checkpoint_num', type=int, default=0, help='epoch of the checkpoint in --outf to continue from (0: none); the shuffles continue where that run stopped')
    p.add_argument('--top_dir', type=str, default='.', help='root that the path flags are relative to')
    p.add_argument('--seed', type=int, default=0, help='initial weights and the shuffle of every epoch')
    p.add_argument('--graph_seed', type=int, default=0, help='key of the neighbour sampling of both graph pools')
    p.add_argument('--sampling', type=str, default='device', choices=['device', 'reference'])
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    from .fold_trainer import FoldingNetTrainer, check_batch
    check_batch(flags.batchSize)
    print('Train FoldingNet flags:', flags)
    top = flags.top_dir
    train = np.load(osp.join(top, flags.training_set)).astype(np.float32)
    val = np.load(osp.join(top, flags.validation_set)).astype(np.float32)
    assert train.shape[1] == flags.num_points and val.shape[1] == flags.num_points, 'the clouds must have --num_points points'
    outf = osp.join(top, flags.outf)
    B = flags.batchSize
    trainers, current = {}, None      # one handle per batch size (the full one and the epoch's last, partial one)

    def trainer(size):
        """The handle of this batch size, brought to the state of the one that stepped last."""
        nonlocal current
        if size not in trainers or (current is not None and current is not trainers[size]):
            kw = dict(num_points=flags.num_points, batch_size=size, seed=flags.graph_seed, sampling=flags.sampling)
            if current is not None:
                step, ordinal = current.counters()
                trainers[size] = FoldingNetTrainer(weights=current.export_state_dict(), step=step, slots=current.slots(),
                                                   ordinal=ordinal, **kw)
            elif flags.checkpoint_num:
                trainers[size] = FoldingNetTrainer.restore(outf, flags.checkpoint_num, **kw)
            else:
                from . import fold_weights
                trainers[size] = FoldingNetTrainer(weights=fold_weights.initial_weights(flags.seed), **kw)
        current = trainers[size]
        return current

    rng = np.random.RandomState(flags.seed)
    for _ in range(flags.checkpoint_num):       # a resumed run continues the interrupted run's sequence of shuffles
        rng.permutation(len(train))
    val_at = 0
    for epoch in range(flags.checkpoint_num + 1, flags.nepoch + 1):
        order = rng.permutation(len(train))
        for i, s in enumerate(range(0, len(order), B)):
            idx = order[s:s + B]
            if len(idx) < 2:
                break
            tr = trainer(len(idx))
            loss, mid = tr.train_step(train[idx])
            print('[%d: %d/%d] train loss: %f middle loss: %f' % (epoch, i, len(order) // B, loss, mid))
            if i % 100 == 0 and len(val) >= 2:
                size = min(B, len(val))
                if val_at + size > len(val):
                    val_at = 0
                ae = tr.eval_model()
                recon = ae.get_reconstructions(val[val_at:val_at + size])
                print('[%d: %d/%d] val loss: %f' % (epoch, i, len(order) // B,
                                                     float(np.mean(ae.get_loss_per_pc(recon, val[val_at:val_at + size])))))
                val_at += size
        print('saved', current.save(outf, epoch))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
