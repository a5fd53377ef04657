"""PointNetClassifier (classifier/pointnet_classifier.py) on the MI355X: the pretrained PointNet classifier the reference's
semantic evaluation feeds reconstructions to, as one geoadv_cls handle (include/geoadv.h; csrc/classifier.hip).

    clf = PointNetClassifier('log/pointnet', 150, num_points=2048, batch_size=10, num_classes=13)
    labels = clf.classify(clouds)            # int8, np.argmax of the logits (first maximum)
    logits = clf.logits(device_tensor)       # float32 (b, num_classes) on the GPU

Unlike the reference, classify accepts any number of clouds (batch_size only sets the chunk), and any point count
1 ... 16384 (num_points is the default the reference's placeholder fixes).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, cls_weights as CW
from ._model import DeviceModel

N_LAYERS = len(CW.LAYERS)


class _ClsWeights(C.Structure):
    """ctypes mirror of geoadv_cls_weights."""
    _fields_ = [("num_classes", C.c_int),
                ("w", C.c_void_p * N_LAYERS), ("b", C.c_void_p * N_LAYERS),
                ("gamma", C.c_void_p * N_LAYERS), ("beta", C.c_void_p * N_LAYERS),
                ("mean", C.c_void_p * N_LAYERS), ("var", C.c_void_p * N_LAYERS)]


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
