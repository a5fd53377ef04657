"""classifier/train_classifier.py on the MI355X: the reference's flags and defaults, the same per-epoch loop (shuffle, jitter,
train on file_size // B full batches, evaluate) and the same files in --log_dir: model-%03d.ckpt every save_model_interval
epochs, the five statistics .npy files and log_train.txt.  Paths are relative to --top_dir.

    python -m geometric_adv_amd.train_classifier --log_dir log/pointnet --num_classes 13 \
        --train_data <...>/point_clouds_train_set_13l.npy --train_labels <...>/pc_label_train_set_13l.npy \
        --val_data <...>/point_clouds_val_set_13l.npy --val_labels <...>/pc_label_val_set_13l.npy

Host randomness (shuffle, jitter) is numpy's global generator seeded by --seed; dropout uses the device generator of
csrc/cls_train.hip keyed by --seed and the step counter.  Rotation augmentation stays off, as in the reference.

--jitter_on_device 1 keeps the training clouds on the GPU: the epoch order is the same np.random.shuffle(idx) draw, and every
batch is one ops.batch_gather launch (gather by index, jitter sigma 0.01 clipped at 0.05) with the device generator of
csrc/dataset.hip keyed by --seed and the global step (epoch * batches per epoch + batch).  The host's np.random.randn draws are
then not made, so numpy's stream -- and the shuffle order of every epoch after the first -- differs from the default mode's.
"""
import argparse
import os
import os.path as osp
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--model', default='pointnet_cls', help='pointnet_cls (pointnet_cls_basic is not provided)')
    p.add_argument('--log_dir', default='log/pointnet')
    p.add_argument('--num_point', type=int, default=2048)
    p.add_argument('--max_epoch', type=int, default=150)
    p.add_argument('--batch_size', type=int, default=32)
    p.add_argument('--learning_rate', type=float, default=0.001)
    p.add_argument('--momentum', type=float, default=0.9)
    p.add_argument('--optimizer', default='adam', help='adam or momentum')
    p.add_argument('--decay_step', type=int, default=200000)
    p.add_argument('--decay_rate', type=float, default=0.7)
    p.add_argument('--save_model_interval', type=int, default=10)
    p.add_argument('--num_classes', type=int, default=13)
    p.add_argument('--train_data', type=str, default='log/autoencoder_victim/eval_train/point_clouds_train_set_13l.npy')
    p.add_argument('--train_labels', type=str, default='log/autoencoder_victim/eval_train/pc_label_train_set_13l.npy')
    p.add_argument('--val_data', type=str, default='log/autoencoder_victim/eval_val/point_clouds_val_set_13l.npy')
    p.add_argument('--val_labels', type=str, default='log/autoencoder_victim/eval_val/pc_label_val_set_13l.npy')
    p.add_argument('--model_path', default=None, help='checkpoint prefix to continue training from')
    p.add_argument('--restore_epoch', type=int, default=0)
    p.add_argument('--seed', type=int, default=0, help='numpy seed (shuffle, jitter, initial weights) and dropout key')
    p.add_argument('--jitter_on_device', type=int, default=0, help='1: resident training clouds, batches gathered and jittered on the GPU [default: 0]')
    p.add_argument('--top_dir', type=str, default='.', help='root that the path flags are relative to')
    return p


def shuffle_data(data, labels):
    """provider.shuffle_data."""
    idx = np.arange(len(labels))
    np.random.shuffle(idx)
    return data[idx, ...], labels[idx], idx


def jitter_point_cloud(batch_data, sigma=0.01, clip=0.05):
    """provider.jitter_point_cloud."""
    B, N, C = batch_data.shape
    return np.clip(sigma * np.random.randn(B, N, C), -1 * clip, clip) + batch_data


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Train classifier flags:', flags)
    if flags.model != 'pointnet_cls':
        raise SystemExit("train_classifier: --model %s is not provided here; only pointnet_cls (the model run_classifier "
                         "reads) is" % flags.model)
    if flags.optimizer not in ('adam', 'momentum'):
        raise SystemExit("train_classifier: --optimizer must be adam or momentum, got %s" % flags.optimizer)
    from .cls_trainer import PointNetClassifierTrainer

    top = flags.top_dir
    log_dir = osp.join(top, flags.log_dir)
    os.makedirs(log_dir, exist_ok=True)
    log_fout = open(osp.join(log_dir, 'log_train.txt'), 'a')
    log_fout.write(str(flags) + '\n')

    def log_string(s):
        log_fout.write(s + '\n')
        log_fout.flush()
        print(s)

    np.random.seed(flags.seed)
    B, N, NC = flags.batch_size, flags.num_point, flags.num_classes
    kw = dict(num_points=N, batch_size=B, num_classes=NC, learning_rate=flags.learning_rate, optimizer=flags.optimizer,
              momentum=flags.momentum, decay_step=flags.decay_step, decay_rate=flags.decay_rate, seed=flags.seed)
    if flags.model_path is not None:
        tr = PointNetClassifierTrainer.restore(osp.join(top, flags.model_path), **kw)
        log_string('Model restored.')
    else:
        tr = PointNetClassifierTrainer(**kw)

    train_data = np.load(osp.join(top, flags.train_data))[:, 0:N, :]
    train_label = np.squeeze(np.load(osp.join(top, flags.train_labels))).astype(np.int64)
    val_data = np.load(osp.join(top, flags.val_data))[:, 0:N, :]
    val_label = np.squeeze(np.load(osp.join(top, flags.val_labels))).astype(np.int64)

    slots = int(flags.max_epoch / flags.save_model_interval)
    stats = {k: np.zeros(slots) for k in ('mean_loss', 'accuracy', 'eval_mean_loss', 'eval_accuracy', 'eval_avg_class_acc')}
    if flags.jitter_on_device:
        import torch
        from . import ops
        train_dev = torch.from_numpy(np.ascontiguousarray(train_data, dtype=np.float32)).to(tr.device)
    for epoch in range(flags.restore_epoch, flags.max_epoch):
        log_string('**** EPOCH %03d ****' % epoch)
        sys.stdout.flush()
        # train_one_epoch
        if flags.jitter_on_device:
            idx = np.arange(len(train_label))
            np.random.shuffle(idx)                                     # shuffle_data's draw; the clouds stay where they are
            label = train_label[idx]
        else:
            data, label, _ = shuffle_data(train_data, train_label)
        num_batches = len(label) // B
        total_correct = total_seen = 0
        loss_sum = 0.0
        for bi in range(num_batches):
            s, e = bi * B, (bi + 1) * B
            if flags.jitter_on_device:
                jittered = ops.batch_gather(train_dev, idx[s:e], dict(seed=flags.seed % (1 << 64), counter=epoch * num_batches + bi,
                                                                      noise_sigma=0.01, noise_clip=0.05))
            else:
                jittered = jitter_point_cloud(data[s:e]).astype(np.float32)
            loss_val, pred = tr.train_step(jittered, label[s:e])
            total_correct += int(np.sum(pred == label[s:e]))
            total_seen += B
            loss_sum += loss_val
        mean_loss = loss_sum / float(max(num_batches, 1))
        accuracy = total_correct / float(max(total_seen, 1))
        log_string('mean loss: %f' % mean_loss)
        log_string('accuracy: %f' % accuracy)
        # eval_one_epoch
        num_batches = val_data.shape[0] // B
        total_correct = total_seen = 0
        loss_sum = 0.0
        seen_c, correct_c = np.zeros(NC), np.zeros(NC)
        for bi in range(num_batches):
            s, e = bi * B, (bi + 1) * B
            loss_val, pred = tr.eval_step(val_data[s:e].astype(np.float32), val_label[s:e])
            total_correct += int(np.sum(pred == val_label[s:e]))
            total_seen += B
            loss_sum += loss_val * B
            for i in range(s, e):
                seen_c[val_label[i]] += 1
                correct_c[val_label[i]] += pred[i - s] == val_label[i]
        eval_mean_loss = loss_sum / float(max(total_seen, 1))
        eval_accuracy = total_correct / float(max(total_seen, 1))
        with np.errstate(invalid='ignore', divide='ignore'):
            eval_avg_class_acc = float(np.mean(correct_c / seen_c))     # the reference's np.mean (nan for an unseen class)
        log_string('eval mean loss: %f' % eval_mean_loss)
        log_string('eval accuracy: %f' % eval_accuracy)
        log_string('eval avg class acc: %f' % eval_avg_class_acc)
        if (epoch + 1) % flags.save_model_interval == 0:
            save_path = tr.save(osp.join(log_dir, 'model-%03d.ckpt' % (epoch + 1)))
            log_string('Model saved in file: %s' % save_path)
            k = int(epoch / flags.save_model_interval)
            if k < slots:
                for name, v in (('mean_loss', mean_loss), ('accuracy', accuracy), ('eval_mean_loss', eval_mean_loss),
                                ('eval_accuracy', eval_accuracy), ('eval_avg_class_acc', eval_avg_class_acc)):
                    stats[name][k] = v
            for name, arr in stats.items():
                np.save(osp.join(log_dir, name), arr)
    log_fout.close()
    return tr


if __name__ == '__main__':
    main()
