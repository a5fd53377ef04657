"""White-box attack on the PointNet classifier (not in the reference; cls_attack.py):

    python -m geometric_adv_amd.run_cls_attack --classifier_folder log/pointnet --input clouds.npy --labels labels.npy \\
        [--target_labels targets.npy] --method cw [--knn_weight 5 --knn_k 5 --knn_alpha 1.05 --clip_linf 0.1] --output_dir cls_attack_res

--input: (num, n, 3) float clouds; --labels: (num,) their true classes.  With --target_labels the attack is targeted at
them; without, it is untargeted (away from --labels).  Paths are relative to --top_dir.  Writes into --output_dir:
  adversarial_pc_input.npy      (num, n, 3) float32: the best adversarial cloud of every source (its last iterate without success),
  adversarial_metrics.npy       (num, 4) float32: success flag, best distance, best iteration (-1: none), last loss,
  adversarial_pred_labels.npy   (num,) int8: PointNetClassifier.classify of the written clouds,
  cls_attack_configuration.json the flags.
--knn_weight adds the kNN attack's outlier term (ops.knn_outlier_loss) to the cw loss, the term aimed at run_defense_sor.
The clouds are what run_defense_sor / run_defense_srs (ops.sor_filter, ops.random_drop) take.  A rerun writes the same bytes.
"""
import argparse
import json
import os.path as osp

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--classifier_folder', type=str, default='log/pointnet')
    p.add_argument('--classifier_restore_epoch', type=int, default=150)
    p.add_argument('--num_classes', type=int, default=13)
    p.add_argument('--input', type=str, required=True, help='clouds (num, n, 3) .npy')
    p.add_argument('--labels', type=str, required=True, help='true classes (num,) .npy')
    p.add_argument('--target_labels', type=str, default=None, help='targets (num,) .npy: given = targeted, absent = untargeted')
    p.add_argument('--method', type=str, default='cw', choices=('cw', 'ifgsm'))
    p.add_argument('--dist_type', type=str, default='l2', choices=('l2', 'chamfer'), help='cw: the distance term')
    p.add_argument('--dist_weight', type=float, default=1.0, help='cw: weight of the distance term')
    p.add_argument('--kappa', type=float, default=0.0, help='cw: confidence')
    p.add_argument('--learning_rate', type=float, default=0.01, help='cw: Adam step')
    p.add_argument('--eps', type=float, default=0.05, help='ifgsm: the box |adv - x| <= eps')
    p.add_argument('--alpha', type=float, default=None, help='ifgsm: step (default eps / num_iterations)')
    p.add_argument('--knn_weight', type=float, default=0.0, help='cw: weight of the kNN outlier term inside the distance term (0 = off)')
    p.add_argument('--knn_k', type=int, default=5, help='cw: neighbours of the kNN term')
    p.add_argument('--knn_alpha', type=float, default=1.05, help='cw: the kNN term penalises scores above mean + knn_alpha * std')
    p.add_argument('--clip_linf', type=float, default=None, help='cw: clamp the perturbation to [-c, c] after every step (default: none)')
    p.add_argument('--num_iterations', type=int, default=200)
    p.add_argument('--batch_size', type=int, default=10)
    p.add_argument('--output_dir', type=str, default='cls_attack_res')
    p.add_argument('--top_dir', type=str, default='.', help='root that the path flags are relative to')
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    print('Run classifier attack flags:', flags)
    from .attack_data import create_dir
    from .classifier import PointNetClassifier
    from .cls_attack import ClassifierAttack
    from .run_classifier import classifier_weights_path

    clouds = np.load(osp.join(flags.top_dir, flags.input))
    labels = np.load(osp.join(flags.top_dir, flags.labels)).reshape(-1)
    if clouds.ndim != 3 or clouds.shape[2] != 3:
        raise SystemExit('run_cls_attack: --input must hold clouds of shape (num, n, 3), got %s' % (clouds.shape,))
    if len(labels) != len(clouds):
        raise SystemExit('run_cls_attack: %d labels for %d clouds' % (len(labels), len(clouds)))
    targeted = flags.target_labels is not None
    goal = np.load(osp.join(flags.top_dir, flags.target_labels)).reshape(-1) if targeted else labels
    if len(goal) != len(clouds):
        raise SystemExit('run_cls_attack: %d target labels for %d clouds' % (len(goal), len(clouds)))

    classifier_path = osp.join(flags.top_dir, flags.classifier_folder)
    clf = PointNetClassifier(classifier_path, flags.classifier_restore_epoch, num_points=clouds.shape[1],
                             batch_size=flags.batch_size, num_classes=flags.num_classes,
                             weights=classifier_weights_path(classifier_path, flags.classifier_restore_epoch))
    attack = ClassifierAttack(clf, method=flags.method, targeted=targeted, dist_type=flags.dist_type, dist_weight=flags.dist_weight,
                              kappa=flags.kappa, learning_rate=flags.learning_rate, num_iterations=flags.num_iterations,
                              eps=flags.eps, alpha=flags.alpha, knn_weight=flags.knn_weight, knn_k=flags.knn_k,
                              knn_alpha=flags.knn_alpha, clip_linf=flags.clip_linf)
    metrics, adversarial = attack.attack(clouds, goal)
    pred = clf.classify(adversarial)

    out = create_dir(osp.join(flags.top_dir, flags.output_dir))
    np.save(osp.join(out, 'adversarial_pc_input.npy'), adversarial)
    np.save(osp.join(out, 'adversarial_metrics.npy'), metrics)
    np.save(osp.join(out, 'adversarial_pred_labels.npy'), pred)
    conf = dict(vars(flags), targeted=targeted, alpha=attack.alpha, num_clouds=int(len(clouds)), num_points=int(clouds.shape[1]))
    with open(osp.join(out, 'cls_attack_configuration.json'), 'w') as f:
        json.dump(conf, f, sort_keys=True)
    print('Successful attacks: %d of %d' % (int(metrics[:, 0].sum()), len(clouds)))


if __name__ == '__main__':
    main()
