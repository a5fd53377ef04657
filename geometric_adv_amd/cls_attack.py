"""White-box attacks on the PointNet classifier (not in the reference, which attacks the auto-encoder): the two standard
semantic attacks the SOR / SRS defenses were designed against, as plain torch tensor operations around
PointNetClassifier.input_gradient (csrc/cls_grad.hip).  The loop has no host synchronisation.

    atk = ClassifierAttack(clf, method='cw', targeted=True, dist_type='l2', dist_weight=1.0, num_iterations=200)
    metrics, adversarial_pc = atk.attack(clouds, target_labels)

method='cw': Xiang et al.'s point perturbation (Generating 3D Adversarial Point Clouds, CVPR 2019) without the binary search
over the weight: a per-cloud perturbation from zero, loss f(x + pert) + dist_weight * D with f the Carlini-Wagner logit loss
(GEOADV_CLS_LOSS_CW_*, confidence kappa) and D = sum ||pert||^2 ('l2') or the Chamfer distance of x + pert to x
(ops.nn_distance_autograd: mean of both directions), minimised by Adam in TF's form (beta1 .9, beta2 .999, eps 1e-8:
alpha_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); m += (g - m)(1 - beta1); v += (g g - v)(1 - beta2);
pert -= alpha_t m / (sqrt(v) + eps) -- the update AdvAE documents).

method='ifgsm': Liu et al.'s iterative gradient sign (Extending Adversarial Attacks and Defenses to Deep 3D Point Cloud
Classifiers, ICIP 2019): x_{k+1} = clip(x_k -/+ alpha sign(g), x - eps, x + eps) with g the cross-entropy gradient --
descending on the target label, or ascending on the true label; alpha defaults to eps / num_iterations; D = max |pert|.

knn_weight != 0 (method='cw', either dist_type) adds the kNN term of Tsai, Yang and Chen's kNN attack (Robust Adversarial Objects
against Deep Learning Models, AAAI 2020), the literature's answer to SOR: K = ops.knn_outlier_loss(x + pert, knn_k, knn_alpha),
the mean squared kNN distance of exactly the points a statistical outlier filter would remove (csrc/knn_loss.hip).  The loss is
f + dist_weight * (D + knn_weight * K), its gradient g + dist_weight * (dD + knn_weight * dK); keep-best still ranks by D.
clip_linf=c clamps pert to [-c, c] after each Adam step and forms the iterate with box(), so |adv - x| <= c holds exactly.

Keep-best, per cloud: among the iterates that the SAME call's logits classify adversarially (the first arg-max equals the
target, or differs from the true label) the one of smallest D.  A cloud that never succeeds is returned as its last iterate.
"""
import numpy as np
import torch

METHODS = ("cw", "ifgsm")
DIST_TYPES = ("l2", "chamfer")
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def first_argmax(logits):
    """np.argmax's rule on a (b, C) tensor: the lowest index among equal maxima."""
    C = logits.shape[1]
    idx = torch.arange(C, device=logits.device).expand_as(logits)
    return torch.where(logits == logits.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, C)).min(dim=1).values


def box(x, pert, eps):
    """x + pert for |pert| <= eps, such that |result - x| <= eps holds in the tensors' own arithmetic: the sum's rounding can
    carry a coordinate past the box by half an ulp, which one step back towards x undoes."""
    adv = x + pert
    out = (adv - x).abs() > eps
    return torch.where(out, torch.nextafter(adv, x), adv)


class ClassifierAttack:
    def __init__(self, clf, method="cw", targeted=True, dist_type="l2", dist_weight=1.0, kappa=0.0, learning_rate=0.01,
                 num_iterations=200, eps=0.05, alpha=None, history=None, knn_weight=0.0, knn_k=5, knn_alpha=1.05, clip_linf=None):
        """clf: a PointNetClassifier (anything with input_gradient, device and batch_size).  history: None or a callable
        (iteration, adv, success, D, loss) that sees every iterate's device tensors as the keep-best rule judged them."""
        if method not in METHODS:
            raise ValueError("method must be one of %s" % (METHODS,))
        if dist_type not in DIST_TYPES:
            raise ValueError("dist_type must be one of %s" % (DIST_TYPES,))
        self.clf = clf
        self.method = method
        self.targeted = bool(targeted)
        self.dist_type = dist_type
        self.dist_weight = float(dist_weight)
        self.kappa = float(kappa)
        self.learning_rate = float(learning_rate)
        self.num_iterations = int(num_iterations)
        self.eps = float(eps)
        self.alpha = float(alpha) if alpha is not None else self.eps / max(self.num_iterations, 1)
        self.history = history
        self.knn_weight = float(knn_weight)
        self.knn_k = int(knn_k)
        self.knn_alpha = float(knn_alpha)
        self.clip_linf = float(clip_linf) if clip_linf is not None else None
        if self.num_iterations < 1:
            raise ValueError("num_iterations must be >= 1")
        if self.kappa < 0 or not np.isfinite(self.kappa):
            raise ValueError("kappa must be finite and >= 0")
        if method == "ifgsm" and not (self.eps > 0 and self.alpha > 0):
            raise ValueError("ifgsm needs eps > 0 and alpha > 0")
        if not np.isfinite(self.knn_weight):
            raise ValueError("knn_weight must be finite")
        if method == "ifgsm" and self.knn_weight != 0.0:
            raise ValueError("the kNN term belongs to method='cw' (ifgsm follows the sign of the cross-entropy gradient alone)")
        if self.knn_weight != 0.0 and not (self.knn_k >= 1 and self.knn_alpha >= 0 and np.isfinite(self.knn_alpha)):
            raise ValueError("the kNN term needs knn_k >= 1 and a finite knn_alpha >= 0")
        if self.clip_linf is not None and not (self.clip_linf > 0 and np.isfinite(self.clip_linf)):
            raise ValueError("clip_linf must be None or finite and > 0")

    # ------------------------------------------------------------------------------------------ distances
    def _distance(self, x, pert):
        """(D (b,), dD / dpert (b, n, 3)) of the CW loss's distance term."""
        if self.dist_type == "l2":
            return (pert * pert).sum(dim=(1, 2)), 2.0 * pert
        from . import ops
        p = pert.detach().clone().requires_grad_(True)
        d1, _, d2, _ = ops.nn_distance_autograd(x + p, x)
        D = d1.mean(dim=1) + d2.mean(dim=1)
        D.sum().backward()
        return D.detach(), p.grad

    def _iterate(self, x, pert):
        """The cloud the classifier sees for a perturbation."""
        if self.method == "cw" and self.clip_linf is None:
            return x + pert
        return box(x, pert, self.eps if self.method == "ifgsm" else self.clip_linf)

    def _judge(self, logits, labels):
        pred = first_argmax(logits)
        return pred == labels if self.targeted else pred != labels

    # ------------------------------------------------------------------------------------------ one chunk
    def _run(self, x, labels):
        clf, T = self.clf, self.num_iterations
        b = x.shape[0]
        labels64 = labels.to(torch.int64)
        pert = torch.zeros_like(x)
        m, v = torch.zeros_like(x), torch.zeros_like(x)
        best_d = torch.full((b,), float("inf"), dtype=x.dtype, device=x.device)
        best_it = torch.full((b,), -1, dtype=torch.int64, device=x.device)
        best_adv = x.clone()
        last_loss = None
        loss_kind = ("cw_targeted" if self.targeted else "cw_untargeted") if self.method == "cw" else "xent"
        for it in range(T):
            adv = self._iterate(x, pert)
            f, g, logits = clf.input_gradient(adv, labels, loss=loss_kind, kappa=self.kappa, return_logits=True)[:3]
            if self.method == "cw":
                D, dD = self._distance(x, pert)
                if self.knn_weight != 0.0:
                    from . import ops
                    K, dK = ops.knn_outlier_loss(adv, self.knn_k, self.knn_alpha)
                    last_loss = f + self.dist_weight * (D + self.knn_weight * K.to(D.dtype))
                    dD = dD + self.knn_weight * dK
                else:
                    last_loss = f + self.dist_weight * D
            else:
                D = (adv - x).abs().amax(dim=(1, 2))
                last_loss = f
            ok = self._judge(logits, labels64)
            better = ok & (D < best_d)
            best_d = torch.where(better, D, best_d)
            best_it = torch.where(better, torch.full_like(best_it, it), best_it)
            best_adv = torch.where(better[:, None, None], adv, best_adv)
            if self.history is not None:
                self.history(it, adv, ok, D, last_loss)
            if self.method == "cw":
                total = g + self.dist_weight * dD
                t = it + 1
                alpha_t = self.learning_rate * np.sqrt(1.0 - ADAM_BETA2 ** t) / (1.0 - ADAM_BETA1 ** t)
                m = m + (total - m) * (1.0 - ADAM_BETA1)
                v = v + (total * total - v) * (1.0 - ADAM_BETA2)
                pert = pert - alpha_t * m / (torch.sqrt(v) + ADAM_EPS)
                if self.clip_linf is not None:
                    pert = torch.clamp(pert, -self.clip_linf, self.clip_linf)
            else:
                step = self.alpha * torch.sign(g)
                pert = torch.clamp(pert - step if self.targeted else pert + step, -self.eps, self.eps)
        last = self._iterate(x, pert)
        found = best_it >= 0
        out = torch.where(found[:, None, None], best_adv, last)
        metrics = torch.stack([found.to(x.dtype), best_d, best_it.to(x.dtype), last_loss.to(x.dtype)], dim=1)
        return metrics, out

    def attack(self, source_pc, labels):
        """source_pc (num, n, 3); labels (num,) integers: the targets (targeted) or the true classes.  Returns
        (metrics (num, 4) float32: success flag, best D (inf without success), best iteration (-1 without), the loss at
        the last iteration; adversarial_pc (num, n, 3) float32) as numpy arrays.  Any number of clouds, in chunks of
        clf.batch_size."""
        clf = self.clf
        dtype = getattr(clf, "dtype", torch.float32)
        x = source_pc if isinstance(source_pc, torch.Tensor) else torch.as_tensor(np.asarray(source_pc))
        x = x.to(clf.device, dtype=dtype).contiguous()
        if x.dim() != 3 or x.shape[2] != 3:
            raise ValueError("point clouds must be of shape (num, points, 3); got %s" % (tuple(x.shape),))
        lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
        if lab.dtype.kind not in "iu":
            raise ValueError("labels must be integers, got %s" % lab.dtype)
        lab = lab.reshape(-1)
        if len(lab) != x.shape[0]:
            raise ValueError("%d labels for %d clouds" % (len(lab), x.shape[0]))
        C = getattr(clf, "num_classes", None)
        if len(lab) and C is not None and (lab.min() < 0 or lab.max() >= C):
            raise ValueError("labels must lie in [0, %d)" % C)
        lab = torch.from_numpy(lab.astype(np.int32)).to(clf.device)
        metrics, advs = [], []
        for s in range(0, x.shape[0], clf.batch_size):
            mt, adv = self._run(x[s:s + clf.batch_size], lab[s:s + clf.batch_size])
            metrics.append(mt)
            advs.append(adv)
        if not advs:
            return np.zeros((0, 4), np.float32), np.zeros(tuple(x.shape), np.float32)
        return (torch.cat(metrics).cpu().numpy().astype(np.float32), torch.cat(advs).cpu().numpy().astype(np.float32))
