"""What the wrappers of a libgeoadv.so model handle share (PointNetClassifier, AtlasNetAE, FoldingNetAE, PointNetAE): the
handle and its release, the input conversion and the grow-only workspace."""
import ctypes as C

import numpy as np
import torch

from . import _lib


class DeviceModel:
    """A subclass names its geoadv_*_destroy in `_destroy`, sets `device` and creates `_h` (a c_void_p) in its constructor."""
    _destroy = None
    _h = None
    _ws = None

    def __del__(self):
        try:
            if self._h is not None and self._h.value:
                getattr(_lib.lib(), self._destroy)(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _as_dev(self, x):
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
        t = t.to(self.device, dtype=torch.float32).contiguous()
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("point clouds must be of shape (batch, points, 3); got %s" % (tuple(t.shape),))
        return t

    def _workspace(self, need):
        """A uint8 device tensor of at least `need` bytes, kept and only ever grown."""
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        return self._ws
