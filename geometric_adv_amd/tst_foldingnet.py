"""transfer/foldingnet/tst_foldingnet.py on the MI355X: scores a checkpoint that train_foldingnet wrote on a set of clouds --
the mean Chamfer distance between every cloud and its reconstruction (test loss), and between it and fold1's output (middle
test loss).  The flags are the ones train_foldingnet keeps; paths are relative to --top_dir.

    python -m geometric_adv_amd.tst_foldingnet --outf log/foldingnet --checkpoint_num 24 --graph_seed 7

Prints the reference's line per batch and its closing line (without colour codes), writes nothing, and returns
(test loss, middle test loss).

Left out: --workers (the data is one array in memory), --mode and --metric (the graph is the reference's default one), as in
train_foldingnet.  --graph_seed is required: the reference's Graph_Pooling draws neighbours with an unseeded
np.random.choice, so its own score moves from run to run (see foldingnet.py for --sampling).

One difference in the arithmetic: the reference forms a float32 mean over each batch and weights it by the batch size; here
the two numbers are float64 means of the per-cloud float32 losses (FoldingNetAE.evaluate), in cloud order.  The two agree to
float32 rounding, and this one does not move with --batchSize.
"""
import argparse
import os.path as osp

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--test_set', type=str, default='log/autoencoder_victim/eval/point_clouds_test_set_13l.npy')
    p.add_argument('--batchSize', type=int, default=16)
    p.add_argument('--num_points', type=int, default=2048)
    p.add_argument('--outf', type=str, default='log/foldingnet')
    p.add_argument('--checkpoint_num', type=int, default=24, help='epoch of the checkpoint in --outf to score')
    p.add_argument('--top_dir', type=str, default='.', help='root that the path flags are relative to')
    p.add_argument('--graph_seed', type=int, default=None, help='key of the neighbour sampling of both graph pools (required)')
    p.add_argument('--sampling', type=str, default='device', choices=['device', 'reference'])
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    if flags.graph_seed is None:
        raise SystemExit('tst_foldingnet: --graph_seed is needed: FoldingNet\'s Graph_Pooling draws neighbours with an unseeded '
                         'np.random.choice (foldingnet.py:36-39), so without a seed its score is not reproducible, not even '
                         'by the reference')
    print('Test FoldingNet flags:', flags)
    top = flags.top_dir
    point_clouds = np.load(osp.join(top, flags.test_set)).astype(np.float32)
    assert point_clouds.ndim == 3 and point_clouds.shape[1] == flags.num_points, \
        'the clouds must have --num_points points (%d); got %s' % (flags.num_points, point_clouds.shape)
    print('Test set: %d examples' % len(point_clouds))

    from .foldingnet import FoldingNetAE
    ae = FoldingNetAE(osp.join(top, flags.outf), epoch=flags.checkpoint_num, seed=flags.graph_seed, sampling=flags.sampling,
                      batch_size=flags.batchSize)
    print('Checkpoint successfully loaded')
    num_batch = len(point_clouds) / flags.batchSize
    res = ae.evaluate(point_clouds, progress=lambda j, seconds: print(
        'Batch %d/%d\t Duration (minutes): %.3f ' % (j, num_batch, seconds / 60.0)))
    loss = float(np.mean(res['loss_per_pc'], dtype=np.float64))
    mid_loss = float(np.mean(res['mid_loss_per_pc'], dtype=np.float64))
    print('%s test loss: %f middle test loss: %f' % ('Testing', loss, mid_loss))
    return loss, mid_loss


if __name__ == '__main__':
    main()
