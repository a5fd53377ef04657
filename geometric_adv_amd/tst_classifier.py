"""classifier/tst_classifier.py on the MI355X: the trained PointNet classifier on the test set, with rotation votes, through
PointNetClassifier.evaluate (one geoadv_cls_evaluate per batch; csrc/cls_eval.hip).

    python -m geometric_adv_amd.tst_classifier --model_path log/pointnet/model-150.ckpt --dump_dir log/pointnet/log_test \
        --test_data <eval>/point_clouds_test_set_13l.npy --test_labels <eval>/pc_label_test_set_13l.npy \
        --pc_classes <eval>/pc_classes_13l.npy --save_pred_labels 1

The reference's flags and defaults; paths are relative to --top_dir.  Writes under --dump_dir, in the reference's formats:
log_test.txt (the flags, 'Model restored.', the three 'test ...' lines and one '%10s:\t%0.3f' line per class), pred_label.txt
('%d, %d' = predicted, true label per cloud) and test_accuracy.npy.

Differences from the reference:
  - --num_votes (default 1, the value the reference's __main__ hard-codes) sets the number of rotation votes,
  - --save_pred_labels 1 also writes the predicted labels next to --test_labels, under that file's name with 'pc_label_'
    replaced by 'pc_pred_labels_' and with its dtype and shape: the pc_pred_labels_test_set*.npy that --correct_pred_only 1
    reads everywhere (run_attack, get_dists_per_point, the defenses, run_classifier, run_transfer), which the reference
    downloads instead,
  - the number of clouds need not be a multiple of --batch_size,
  - --model_path is read by the TF-free checkpoint reader (an .npz of the same variable names is accepted too).
"""
import argparse
import os
import os.path as osp

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--gpu', type=int, default=0, help='GPU to use [default: GPU 0]')
    p.add_argument('--model', default='pointnet_cls', help='pointnet_cls (pointnet_cls_basic is not provided)')
    p.add_argument('--batch_size', type=int, default=2)
    p.add_argument('--num_point', type=int, default=2048)
    p.add_argument('--num_classes', type=int, default=13)
    p.add_argument('--model_path', default='log/pointnet/model-150.ckpt')
    p.add_argument('--dump_dir', default='log/pointnet/log_test')
    p.add_argument('--test_data', type=str, default='log/autoencoder_victim/eval/point_clouds_test_set_13l.npy')
    p.add_argument('--test_labels', type=str, default='log/autoencoder_victim/eval/pc_label_test_set_13l.npy')
    p.add_argument('--pc_classes', type=str, default='log/autoencoder_victim/eval/pc_classes_13l.npy')
    p.add_argument('--num_votes', type=int, default=1, help='rotation votes per cloud [default: 1]')
    p.add_argument('--save_pred_labels', type=int, default=0,
                   help="1: write the predicted labels next to --test_labels as pc_pred_labels_* [default: 0]")
    p.add_argument('--top_dir', type=str, default='.', help='root that the path flags are relative to')
    return p


def pred_labels_path(test_labels):
    """<dir>/pc_label_test_set_13l.npy -> <dir>/pc_pred_labels_test_set_13l.npy (the name attack_data.load_data finds by
    'pc_pred_labels_test_set'); a file name without 'pc_label_' is refused."""
    folder, name = osp.split(test_labels)
    if 'pc_label_' not in name:
        raise SystemExit("tst_classifier: --save_pred_labels 1 names its output after --test_labels by replacing 'pc_label_' "
                         "with 'pc_pred_labels_', and %r does not contain 'pc_label_'" % name)
    return osp.join(folder, name.replace('pc_label_', 'pc_pred_labels_'))


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Test classifier flags:', flags)
    if flags.model != 'pointnet_cls':
        raise SystemExit("tst_classifier: --model %s is not provided here; only pointnet_cls (the model run_classifier "
                         "reads) is" % flags.model)
    top = flags.top_dir
    labels_file = osp.join(top, flags.test_labels)
    pred_file = pred_labels_path(labels_file) if flags.save_pred_labels else None      # refused before anything is written

    from .classifier import PointNetClassifier

    dump_dir = osp.join(top, flags.dump_dir)
    os.makedirs(dump_dir, exist_ok=True)
    log_fout = open(osp.join(dump_dir, 'log_test.txt'), 'w')
    log_fout.write(str(flags) + '\n')

    def log_string(s):
        log_fout.write(s + '\n')
        log_fout.flush()
        print(s)

    pc_classes = np.load(osp.join(top, flags.pc_classes))
    data = np.load(osp.join(top, flags.test_data))[:, 0:flags.num_point, :]
    stored_label = np.load(labels_file)
    label = np.squeeze(stored_label).reshape(-1)

    clf = PointNetClassifier(None, num_points=flags.num_point, batch_size=flags.batch_size, num_classes=flags.num_classes,
                             weights=osp.join(top, flags.model_path), device='cuda:%d' % flags.gpu)
    log_string('Model restored.')
    res = clf.evaluate(data, label, num_votes=flags.num_votes)

    with open(osp.join(dump_dir, 'pred_label.txt'), 'w') as fout:
        for p, l in zip(res['pred'], label):
            fout.write('%d, %d\n' % (p, l))
    log_string('test mean loss: %f' % res['mean_loss'])
    log_string('test accuracy: %f' % res['accuracy'])
    log_string('test avg class acc: %f' % res['avg_class_acc'])
    np.save(osp.join(dump_dir, 'test_accuracy'), res['accuracy'])
    for i, name in enumerate(pc_classes):
        log_string('%10s:\t%0.3f' % (name, res['class_accuracies'][i]))
    if pred_file is not None:
        np.save(pred_file, res['pred'].astype(stored_label.dtype).reshape(stored_label.shape))
        log_string('Predicted labels saved in file: %s' % pred_file)
    log_fout.close()
    return res


if __name__ == '__main__':
    main()
