"""LayerTrainer: what the Python handles of the three layer-by-layer trainers share (cls_trainer.py, fold_trainer.py,
atlas_trainer.py over csrc/train_bn.h's TrainArena): the handle's lifetime, the flat buffers and their layout, state views,
counters, and the walk between a flat parameter-layout buffer and named tensors.

A subclass sets _PREFIX (its geoadv_<prefix>_trainer_* functions), _STATE ({name: GEOADV_*_STATE_* constant}), _INT_STATES
(the int32 ones) and _COUNTERS (the ctypes of what its counters function returns), and defines _state_shapes(layer) and
_tensors().
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def seed64(seed):
    """seed mod 2^64 as the int64 a config struct carries."""
    s = int(seed) & ((1 << 64) - 1)
    return s - (1 << 64) if s >= (1 << 63) else s


def torch_layer_tensors(name, bn_name, o, fi, fo, conv, q=0):
    """_tensors() entries of group q of a layer stored torch's way: .weight (fo, fi[, 1]) kept transposed, .bias, and the
    batch norm's .weight / .bias under bn_name (None = no norm); o = the layer's four offsets."""
    yield name + ".weight", o[0] + q * fi * fo, fi * fo, (fo, fi, 1) if conv else (fo, fi), True
    yield name + ".bias", o[1] + q * fo, fo, (fo,), False
    if bn_name:
        yield bn_name + ".weight", o[2] + q * fo, fo, (fo,), False
        yield bn_name + ".bias", o[3] + q * fo, fo, (fo,), False


class LayerTrainer:
    _PREFIX = None
    _STATE = {}
    _INT_STATES = ()
    _COUNTERS = (C.c_longlong, C.c_longlong)

    def _call(self, name, *args):
        who = "%s_trainer_%s" % (self._PREFIX, name)
        _lib.check(getattr(_lib.lib(), "geoadv_" + who)(*args), who)

    def _open(self, canon, hw, create_args, max_layers):
        """Points the weights struct hw at canon's arrays ({field: [array or None per layer]}), creates the handle from
        create_args (the structs of geoadv_*_trainer_create after the handle, hw among them) and fetches its buffers and
        layout (max_layers = what geoadv_*_trainer_layout writes)."""
        for key, arrays in canon.items():
            field = getattr(hw, key)
            for i, a in enumerate(arrays):
                field[i] = a.ctypes.data if a is not None else None
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            self._call("create", C.byref(self._h), *[C.byref(a) for a in create_args])
        pp, gp, cnt = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._call("buffers", self._h, C.byref(pp), C.byref(gp), C.byref(cnt))
        self._count, self._params_ptr, self._grads_ptr = int(cnt.value), pp.value, gp.value
        offs, moffs = (C.c_size_t * (4 * max_layers))(), (C.c_size_t * max_layers)()
        self._call("layout", self._h, offs, moffs)
        self._offsets, self._moving_offsets = list(offs), list(moffs)
        self._eval = None

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                getattr(_lib.lib(), "geoadv_%s_trainer_destroy" % self._PREFIX)(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # ---- device views --------------------------------------------------------------------------------------
    def state(self, what, layer=0, device=False):
        """Host copy of what the last step kept (geoadv_*_trainer_state), in the shape _state_shapes gives it.  device=True
        returns a view of the device buffer instead: it aliases the handle's memory, so it changes with the next step and
        dangles once this trainer is destroyed -- drop the view before the trainer."""
        p, cnt = C.c_void_p(), C.c_size_t()
        self._call("state", self._h, self._STATE[what], int(layer), C.byref(p), C.byref(cnt))
        torch.cuda.synchronize(self.device)
        if not cnt.value:
            raise ValueError("state(%r) is empty before the first step" % what)
        a = _lib.device_view(p.value, cnt.value, "<i4" if what in self._INT_STATES else "<f4", self.device)
        if not device:
            a = a.cpu().numpy().copy()
        shapes = self._state_shapes(int(layer))
        return a.reshape(shapes[what]) if what in shapes else a

    def counters(self):
        vals = [t() for t in self._COUNTERS]
        self._call("counters", self._h, *[C.byref(v) for v in vals])
        return tuple(v.value for v in vals)

    @property
    def step(self):
        return self.counters()[0]

    def _dev(self, x, dtype=torch.float32):
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        return t.to(self.device, dtype=dtype).contiguous()

    # ---- flat buffers <-> named tensors ----------------------------------------------------------------------
    # _tensors() yields (key, offset, count, shape, transposed) of every parameter tensor: `count` floats at `offset` of a
    # parameter-layout buffer are the tensor of that shape, or, transposed, the [fan_in][fan_out] transpose of a
    # (fan_out, fan_in[, 1]) one.
    def _unflatten(self, flat, suffix=""):
        """{key + suffix: array in its own shape} from a flat parameter-layout buffer."""
        out = {}
        for key, o, cnt, shape, tr in self._tensors():
            a = flat[o:o + cnt]
            out[key + suffix] = np.ascontiguousarray(a.reshape(-1, shape[0]).T).reshape(shape) if tr else a.reshape(shape).copy()
        return out

    def _flatten(self, named, suffix=""):
        flat = np.zeros(self._count, np.float32)
        for key, o, cnt, shape, tr in self._tensors():
            a = np.asarray(named[key + suffix], np.float32)
            flat[o:o + cnt] = a.reshape(shape[0], -1).T.reshape(-1) if tr else a.reshape(-1)
        return flat

    def _host(self, ptr):
        torch.cuda.synchronize(self.device)
        return _lib.device_view(ptr, self._count, "<f4", self.device).cpu().numpy().copy()

    def parameters(self):
        """{parameter key: array} of the trainable tensors (host copies, in their own shapes)."""
        return self._unflatten(self._host(self._params_ptr))

    def gradients(self):
        """{parameter key: d loss / d parameter} of the last step (host copies; without any weight-decay term)."""
        return self._unflatten(self._host(self._grads_ptr))

    def slots(self):
        """Adam's {'exp_avg': {key: array}, 'exp_avg_sq': {key: array}} (the two optimizer slots)."""
        return {"exp_avg": self._unflatten(self.state("slot1")), "exp_avg_sq": self._unflatten(self.state("slot2"))}

    def _upload_slots(self, slot1, slot2, *extra):
        """Flat parameter-layout buffers (None = leave as it is) into the optimizer's slots."""
        self._call("set_slots", self._h, *[s.ctypes.data if s is not None else None for s in (slot1, slot2)], *extra)
