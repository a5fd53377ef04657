"""PointNetClassifierTrainer (classifier/train_classifier.py's graph and train_op) on the MI355X: one geoadv_cls_trainer handle
(include/geoadv.h; csrc/cls_train.hip) per model.

    tr = PointNetClassifierTrainer(num_points=2048, batch_size=32, num_classes=13)
    loss, pred = tr.train_step(x, labels)        # is_training = True: batch statistics, dropout, one optimizer step
    loss, pred = tr.eval_step(x, labels)         # is_training = False: moving statistics, no dropout
    tr.save('log/pointnet/model-010.ckpt')       # TF V2 checkpoint: variables, moving averages, optimizer slots, step

eval_step runs the inference handle (PointNetClassifier) on the exported variables; its loss includes the feature-transform
regulariser, as eval_one_epoch's does.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi, _lib, cls_weights as CW
from ._abi import ClsTrainConfig as _ClsTrainConfig, ClsWeights as _ClsWeights
from ._layer_trainer import LayerTrainer
from .classifier import PointNetClassifier

OPTIMIZERS = {"adam": _abi.GEOADV_CLS_OPT_ADAM, "momentum": _abi.GEOADV_CLS_OPT_MOMENTUM}
_STATE = {k: getattr(_abi, "GEOADV_CLS_STATE_" + k.upper()) for k in (
    "bn_mean", "bn_var", "moving_mean", "moving_var", "dropout_mask", "pool_argmax", "t1", "t2", "logits", "slot1", "slot2", "pre_bn",
    "bn_inv", "bn_shift")}


def _loss64(logits, labels, t2):
    """mean softmax cross entropy + 0.001 * 0.5 * sum (T2 T2^T - I)^2, in float64."""
    z = np.asarray(logits, np.float64)
    m = z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z - m).sum(axis=1)) + m[:, 0]
    ce = lse - z[np.arange(len(z)), np.asarray(labels)]
    t = np.asarray(t2, np.float64).reshape(-1, 64, 64)
    e = t @ t.transpose(0, 2, 1) - np.eye(64)
    return float(ce.mean() + 0.001 * 0.5 * (e ** 2).sum())


class PointNetClassifierTrainer(LayerTrainer):
    _PREFIX, _STATE, _INT_STATES = "cls", _STATE, ("pool_argmax",)
    _COUNTERS = (C.c_longlong, C.c_float, C.c_float)          # counters(): (step, beta1_power, beta2_power) as they stand

    def __init__(self, weights=None, num_points=2048, batch_size=32, num_classes=13, learning_rate=0.001, optimizer="adam",
                 momentum=0.9, decay_step=200000, decay_rate=0.7, seed=0, step=0, slots=None, device=None):
        """weights: {name: array} with every name of cls_weights.variable_names() (None = cls_weights.initial_weights(
        num_classes, seed)).  step / slots: the step counter and the optimizer's variables ({name: array} with the names of
        cls_weights.slot_names(optimizer)) to continue from; None = a fresh optimizer."""
        if optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be 'adam' or 'momentum', got %r" % (optimizer,))
        if weights is None:
            weights = CW.initial_weights(num_classes, seed)
        have = CW.num_classes_of(weights)
        if have != int(num_classes):
            raise ValueError("num_classes %d does not match the weights' fc3 (%d classes)" % (num_classes, have))
        self.num_points, self.batch_size, self.num_classes = int(num_points), int(batch_size), int(num_classes)
        self.optimizer = optimizer
        self.device = torch.device(device if device is not None else "cuda:0")
        hw = _ClsWeights()
        hw.num_classes = self.num_classes
        cfg = _ClsTrainConfig(self.batch_size, self.num_points, OPTIMIZERS[optimizer], float(learning_rate), float(momentum),
                              int(decay_step), float(decay_rate), int(step), int(seed))
        self._open(CW.canonical(weights, self.num_classes), hw, (hw, cfg), _abi.GEOADV_CLS_LAYERS)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._pred = torch.zeros(self.batch_size, dtype=torch.int32, device=self.device)
        if slots is not None:
            self._set_slots(slots)

    @classmethod
    def restore(cls, prefix, weights_only=False, **kwargs):
        """A trainer from a checkpoint `save` (or train_classifier) wrote: the variables and moving averages, and unless
        weights_only the step counter and the optimizer's slots as well (saver.restore)."""
        from . import tf_checkpoint
        weights = CW.load(prefix)
        if weights_only:
            return cls(weights=weights, **kwargs)
        opt = kwargs.get("optimizer", "adam")
        wanted = set(CW.slot_names(opt)) | {CW.STEP_NAME}
        got = tf_checkpoint.load_checkpoint(prefix, lambda n: n in wanted)
        missing = sorted(wanted - set(got))
        if missing:
            raise KeyError("checkpoint %s lacks %d optimizer variable(s): %s" % (prefix, len(missing), ", ".join(missing[:8])))
        kwargs.setdefault("num_classes", CW.num_classes_of(weights))
        return cls(weights=weights, step=int(got.pop(CW.STEP_NAME)), slots=got, **kwargs)

    # ---- device views --------------------------------------------------------------------------------------
    def _state_shapes(self, layer):
        """state(what, layer): 'bn_mean' / 'bn_var' / 'moving_mean' / 'moving_var' / 'bn_inv' / 'bn_shift' of a BN layer
        (GEOADV_CLS_* index), 'pre_bn' of a BN layer ([rows][C]: B * N rows for a per-point layer, B for an fc layer),
        'dropout_mask' 0 / 1, 'pool_argmax' 0 / 1 / 2, 't1', 't2', 'logits', 'slot1', 'slot2'."""
        B = self.batch_size
        return {"dropout_mask": (B, -1), "pool_argmax": (B, 1024), "t1": (B, 3, 3), "t2": (B, 64, 64), "logits": (B, -1),
                "pre_bn": (-1, self._shapes()[layer][2])}

    def _shapes(self):
        nc = self.num_classes
        out = []
        for scope, fi, fo, bn, shape in CW.LAYERS:
            fo = nc if fo is None else fo
            shape = tuple(nc if d is None else d for d in shape)
            out.append((scope, fi, fo, bn, shape))
        return out

    def _tensors(self):
        for l, (scope, fi, fo, bn, shape) in enumerate(self._shapes()):
            o = self._offsets[4 * l: 4 * l + 4]
            yield scope + "/weights", o[0], fi * fo, shape, False
            yield scope + "/biases", o[1], fo, (fo,), False
            if bn:
                yield scope + "/bn/gamma", o[2], fo, (fo,), False
                yield scope + "/bn/beta", o[3], fo, (fo,), False

    def _set_slots(self, slots):
        if self.optimizer == "adam":
            self._upload_slots(self._flatten(slots, "/Adam"), self._flatten(slots, "/Adam_1"), float(slots["beta1_power"]),
                               float(slots["beta2_power"]))
        else:
            self._upload_slots(self._flatten(slots, "/Momentum"), None, 0.9, 0.999)

    def parameters(self):
        """Host copy of the flat parameter buffer."""
        return self._host(self._params_ptr)

    # ---- the steps -----------------------------------------------------------------------------------------
    def train_step(self, x, labels):
        """One sess.run([train_op, loss, pred]) at is_training = True: returns (loss of the pre-update variables, predicted
        labels (np.argmax of the logits))."""
        x = self._dev(x)
        y = self._dev(labels, torch.int32).reshape(-1)
        if tuple(x.shape) != (self.batch_size, self.num_points, 3) or y.numel() != self.batch_size:
            raise ValueError("train_step takes x (%d, %d, 3) and %d labels; got %s and %d"
                             % (self.batch_size, self.num_points, self.batch_size, tuple(x.shape), y.numel()))
        if int(y.min()) < 0 or int(y.max()) >= self.num_classes:
            raise ValueError("labels must lie in [0, %d)" % self.num_classes)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().geoadv_cls_trainer_step(self._h, _lib.ptr(x), _lib.ptr(y), _lib.ptr(self._loss),
                                                          _lib.ptr(self._pred), _lib.stream_handle()), "cls_trainer_step")
        self._eval = None
        return float(self._loss.item()), self._pred.cpu().numpy().copy()

    def eval_step(self, x, labels):
        """is_training = False (moving statistics, no dropout): (loss incl. the regulariser, predicted labels)."""
        if self._eval is None:
            self._eval = PointNetClassifier(None, weights=self.export_weights(slots=False), num_points=self.num_points,
                                            batch_size=self.batch_size, num_classes=self.num_classes, device=self.device)
        logits, pred, _, t2 = self._eval.forward(x, transforms=True)
        return _loss64(logits.cpu().numpy(), np.asarray(labels).reshape(-1), t2.cpu().numpy()), pred.cpu().numpy().astype(np.int64)

    # ---- what saver.save writes ----------------------------------------------------------------------------
    def export_weights(self, slots=True):
        """{name: array} of every variable: cls_weights.variable_names() and, with slots, the optimizer's variables
        (cls_weights.slot_names) and the step counter `Variable` (int32)."""
        out = self._unflatten(self.parameters())
        for l, (scope, fi, fo, bn, shape) in enumerate(self._shapes()):
            if not bn:
                continue
            names = CW.bn_names(scope)
            out[names["mean"]] = self.state("moving_mean", l)
            out[names["var"]] = self.state("moving_var", l)
        if slots:
            step, b1, b2 = self.counters()
            if self.optimizer == "adam":
                out.update(self._unflatten(self.state("slot1"), "/Adam"))
                out.update(self._unflatten(self.state("slot2"), "/Adam_1"))
                out["beta1_power"] = np.array(b1, np.float32)
                out["beta2_power"] = np.array(b2, np.float32)
            else:
                out.update(self._unflatten(self.state("slot1"), "/Momentum"))
            out[CW.STEP_NAME] = np.array(step, np.int32)
        return out

    def save(self, prefix):
        """saver.save: a TF V2 checkpoint `<prefix>.index` + `<prefix>.data-00000-of-00001` of every variable."""
        from . import tf_checkpoint
        tf_checkpoint.write_checkpoint(prefix, self.export_weights(slots=True))
        return prefix
