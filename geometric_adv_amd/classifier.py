"""PointNetClassifier (classifier/pointnet_classifier.py) on the MI355X: the pretrained PointNet classifier the reference's
semantic evaluation feeds reconstructions to, as one geoadv_cls handle (include/geoadv.h; csrc/classifier.hip).

    clf = PointNetClassifier('log/pointnet', 150, num_points=2048, batch_size=10, num_classes=13)
    labels = clf.classify(clouds)            # int8, np.argmax of the logits (first maximum)
    logits = clf.logits(device_tensor)       # float32 (b, num_classes) on the GPU
    stats = clf.evaluate(clouds, labels, num_votes=12)   # tst_classifier.py's eval_one_epoch: loss, accuracies, voted labels

Unlike the reference, classify accepts any number of clouds (batch_size only sets the chunk), and any point count
1 ... 16384 (num_points is the default the reference's placeholder fixes).
"""
import ctypes as C

import numpy as np
import torch

from . import _abi, _lib, cls_weights as CW
from ._abi import ClsWeights as _ClsWeights
from ._model import DeviceModel

N_LAYERS = _abi.GEOADV_CLS_LAYERS
LOSS_KINDS = {"xent": _abi.GEOADV_CLS_LOSS_XENT, "cw_targeted": _abi.GEOADV_CLS_LOSS_CW_TARGETED,
              "cw_untargeted": _abi.GEOADV_CLS_LOSS_CW_UNTARGETED}


class PointNetClassifier(DeviceModel):
    _destroy = "geoadv_cls_destroy"

    def __init__(self, classifier_path, restore_epoch=CW.DEFAULT_EPOCH, num_points=2048, batch_size=10, num_classes=13,
                 weights=None, device=None):
        """Weights from <classifier_path>/model-%03d.ckpt (restore_epoch), unless `weights` is given: a {name: array} dict
        (cls_weights.variable_names), an .npz with those names, or a checkpoint prefix."""
        if weights is None:
            weights = CW.load(classifier_path, restore_epoch)
        elif isinstance(weights, str):
            weights = CW.load(weights)
        self.num_points = int(num_points)
        self.batch_size = int(batch_size)
        self.num_classes = int(num_classes)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        have = CW.num_classes_of(weights)
        if have != self.num_classes:
            raise ValueError("num_classes %d does not match the weights' fc3 (%d classes)" % (self.num_classes, have))
        self.device = torch.device(device if device is not None else "cuda:0")
        self._canon = CW.canonical(weights, self.num_classes)          # host arrays stay alive until create returns
        hw = _ClsWeights()
        hw.num_classes = self.num_classes
        for f in ("w", "b", "gamma", "beta", "mean", "var"):
            arr = getattr(hw, f)
            for i, a in enumerate(self._canon[f]):
                arr[i] = a.ctypes.data if a is not None else None
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().geoadv_cls_create(C.byref(self._h), C.byref(hw)), "cls_create")

    def forward(self, x, transforms=False):
        """(logits (b, C) float32, labels (b,) int32[, T1 (b, 3, 3), T2 (b, 64, 64)]) as device tensors, one call."""
        x = self._as_dev(x)
        b, n = int(x.shape[0]), int(x.shape[1])
        dev = self.device
        logits = torch.empty((b, self.num_classes), dtype=torch.float32, device=dev)
        labels = torch.empty((b,), dtype=torch.int32, device=dev)
        t1 = torch.empty((b, 3, 3), dtype=torch.float32, device=dev) if transforms else None
        t2 = torch.empty((b, 64, 64), dtype=torch.float32, device=dev) if transforms else None
        if b == 0:
            return (logits, labels, t1, t2) if transforms else (logits, labels)
        L = _lib.lib()
        with torch.cuda.device(dev):
            ws = self._workspace(L.geoadv_cls_workspace_bytes(self._h, b, n))
            st = L.geoadv_cls_forward(self._h, b, n, _lib.ptr(x), _lib.ptr(logits), _lib.ptr(labels), _lib.ptr(t1),
                                      _lib.ptr(t2), _lib.ptr(ws), _lib.stream_handle())
        _lib.check(st, "cls_forward")
        return (logits, labels, t1, t2) if transforms else (logits, labels)

    def input_gradient(self, x, labels, loss="xent", kappa=0.0, return_logits=False, return_winners=False):
        """One geoadv_cls_input_grad call (csrc/cls_grad.hip) on the current stream, no host synchronisation: the gradient of
        a logit loss with respect to the points, through the graph of forward() with both T-Nets differentiated.  labels: an
        int32 device tensor (b,) -- the class of the cross entropy ('xent') and of 'cw_untargeted', the target of
        'cw_targeted'.  Returns device tensors (loss (b,) float32 per cloud, grad (b, n, 3)[, logits (b, C) -- forward()'s
        bits][, winners (b, 3, 1024) int32: the row each of the three max pools chose per column])."""
        if loss not in LOSS_KINDS:
            raise ValueError("loss must be one of %s" % sorted(LOSS_KINDS))
        x = self._as_dev(x)
        b, n = int(x.shape[0]), int(x.shape[1])
        dev = self.device
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.device != x.device \
                or tuple(labels.shape) != (b,):
            raise ValueError("labels must be an int32 tensor of shape (%d,) on %s" % (b, x.device))
        labels = labels.contiguous()
        out_loss = torch.empty((b,), dtype=torch.float32, device=dev)
        grad = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
        logits = torch.empty((b, self.num_classes), dtype=torch.float32, device=dev) if return_logits else None
        winners = torch.empty((b, 3, 1024), dtype=torch.int32, device=dev) if return_winners else None
        if b:
            L = _lib.lib()
            with torch.cuda.device(dev):
                ws = self._workspace(L.geoadv_cls_input_grad_workspace_bytes(self._h, b, n))
                st = L.geoadv_cls_input_grad(self._h, b, n, _lib.ptr(x), _lib.ptr(labels), LOSS_KINDS[loss], float(kappa),
                                             _lib.ptr(out_loss), _lib.ptr(logits), _lib.ptr(winners), _lib.ptr(grad),
                                             _lib.ptr(ws), _lib.stream_handle())
            _lib.check(st, "cls_input_grad")
        out = (out_loss, grad)
        if return_logits:
            out += (logits,)
        if return_winners:
            out += (winners,)
        return out

    def logits(self, x):
        """float32 device tensor (b, num_classes) of the classifier's logits (pointnet_cls.py: fc3's output)."""
        return self.forward(x)[0]

    def classify(self, current_data):
        """pointnet_classifier.py:62-82: int8 labels (np.argmax of the logits, first maximum) of every cloud, in chunks of
        batch_size; any number of clouds."""
        x = self._as_dev(current_data)
        out = np.zeros(int(x.shape[0]), dtype=np.int8)
        for s in range(0, int(x.shape[0]), self.batch_size):
            out[s:s + self.batch_size] = self.forward(x[s:s + self.batch_size])[1].cpu().numpy().astype(np.int8)
        return out

    @staticmethod
    def vote_angles(num_votes):
        """tst_classifier.py:134: the rotation angle of every vote."""
        return [v / float(num_votes) * np.pi * 2 for v in range(int(num_votes))]

    def evaluate_batch(self, x, labels=None, num_votes=1):
        """One geoadv_cls_evaluate call (csrc/cls_eval.hip) on the current stream, no host synchronisation: x (b, n, 3) is
        classified num_votes times, rotated by vote_angles(num_votes).  labels: an int32 device tensor (b,) or None.  Returns
        device tensors (loss (V,) float32 or None without labels, pred (b,) int32 -- the first maximum of pred_sum,
        pred_sum (b, C) float64 -- the logits summed in vote order, vote_counts (b, C) int32)."""
        x = self._as_dev(x)
        b, n, V = int(x.shape[0]), int(x.shape[1]), int(num_votes)
        dev = self.device
        if labels is not None:
            if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.device != x.device \
                    or tuple(labels.shape) != (b,):
                raise ValueError("labels must be an int32 tensor of shape (%d,) on %s" % (b, x.device))
            labels = labels.contiguous()
        loss = torch.empty((max(V, 0),), dtype=torch.float32, device=dev) if labels is not None else None
        pred = torch.empty((b,), dtype=torch.int32, device=dev)
        pred_sum = torch.empty((b, self.num_classes), dtype=torch.float64, device=dev)
        counts = torch.empty((b, self.num_classes), dtype=torch.int32, device=dev)
        # the angles' cos / sin from numpy, as provider.rotate_point_cloud_by_angle (and ops.rotate_point_cloud_by_angle) takes them
        cs = (C.c_double * (2 * max(V, 1)))()
        for v, a in enumerate(self.vote_angles(V)):
            cs[2 * v], cs[2 * v + 1] = float(np.cos(a)), float(np.sin(a))
        L = _lib.lib()
        with torch.cuda.device(dev):
            ws = self._workspace(L.geoadv_cls_evaluate_workspace_bytes(self._h, b, n))
            st = L.geoadv_cls_evaluate(self._h, b, n, _lib.ptr(x), _lib.ptr(labels), V, cs, _lib.ptr(loss), _lib.ptr(pred),
                                       _lib.ptr(pred_sum), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_handle())
        _lib.check(st, "cls_evaluate")
        return loss, pred, pred_sum, counts

    def evaluate(self, data, labels=None, num_votes=1):
        """tst_classifier.py's eval_one_epoch over any number of clouds, in chunks of batch_size (the reference asserts that
        batch_size divides the set; a ragged last chunk is weighted by its size, as the reference's bookkeeping would).  One
        evaluate_batch per chunk and one copy to the host at the end.  Returns a dict:
          pred (int64, the voted labels), vote_loss ((chunks, V) float32: every chunk's loss per vote),
          mean_loss (sum over chunks and votes of loss * chunk size / num_votes, in float64, over the number of clouds),
          accuracy, class_accuracies (correct / seen per class: NaN for a class without clouds) and avg_class_acc.
        Without labels only pred is set; the other entries are None."""
        x = self._as_dev(data)
        total, V = int(x.shape[0]), int(num_votes)
        if labels is not None:
            labels = np.asarray(labels)
            if labels.dtype.kind not in "iu":
                raise ValueError("labels must be integers, got %s" % labels.dtype)
            labels = labels.reshape(-1).astype(np.int64)
            if len(labels) != total:
                raise ValueError("%d labels for %d clouds" % (len(labels), total))
            if total and (labels.min() < 0 or labels.max() >= self.num_classes):
                raise ValueError("labels must lie in [0, %d)" % self.num_classes)
            dev_labels = torch.from_numpy(labels.astype(np.int32)).to(self.device)
        starts = list(range(0, total, self.batch_size))
        losses, preds = [], []
        for s in starts:
            e = min(s + self.batch_size, total)
            loss, pred, _, _ = self.evaluate_batch(x[s:e], dev_labels[s:e] if labels is not None else None, V)
            losses.append(loss)
            preds.append(pred)
        pred = torch.cat(preds).cpu().numpy().astype(np.int64) if preds else np.zeros(0, np.int64)
        out = dict(pred=pred, vote_loss=None, mean_loss=None, accuracy=None, class_accuracies=None, avg_class_acc=None)
        if labels is None:
            return out
        vote_loss = torch.stack(losses).cpu().numpy() if losses else np.zeros((0, V), np.float32)
        loss_sum = 0.0
        for k, s in enumerate(starts):
            cur = min(s + self.batch_size, total) - s
            batch_loss_sum = 0.0
            for v in range(V):
                batch_loss_sum += float(vote_loss[k, v]) * cur / float(V)
            loss_sum += batch_loss_sum
        seen = np.bincount(labels, minlength=self.num_classes).astype(np.float64)
        correct = np.bincount(labels[pred == labels], minlength=self.num_classes).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            class_acc = correct / seen
            out.update(vote_loss=vote_loss, mean_loss=loss_sum / float(total) if total else float("nan"),
                       accuracy=float(np.sum(pred == labels)) / float(total) if total else float("nan"),
                       class_accuracies=class_acc, avg_class_acc=float(np.mean(class_acc)))
        return out
