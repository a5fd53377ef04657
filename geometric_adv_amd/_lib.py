"""ctypes binding of libgeoadv.so (include/geoadv.h).  There is NO fallback: if the HIP library
is missing or a call fails, this raises -- the product never routes through a CPU path."""
import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgeoadv.so")

_lib = None


class GeoAdvError(RuntimeError):
    pass


def lib():
    """The loaded library (loads on first use)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GeoAdvError(
                "libgeoadv.so not built: %s is missing. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C geometric_adv_amd/csrc` (needs hipcc, --offload-arch=gfx950)." % LIB_PATH)
        import torch  # noqa: F401  -- first: libgeoadv.so must bind to the HIP runtime torch ships, not to a second copy
        _lib = C.CDLL(LIB_PATH)
        for name in _abi.SIGNATURES:         # every call converts its arguments by the header's types, or raises TypeError
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = _abi.ctypes_signature(name)
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().geoadv_last_error().decode("utf-8", "replace")
        if status == _abi.GEOADV_EINVAL:
            raise ValueError("%s: %s" % (what, msg))
        raise GeoAdvError("%s failed (status %d): %s" % (what, status, msg))


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def device_view(ptr, count, typestr, device):
    """1-D torch tensor over `count` elements of device memory at `ptr` (typestr '<f4', '<i4', '<f8'): a view, not a copy --
    it aliases the owner's memory and dangles once the owner frees it."""
    import torch

    class _Arr:
        pass
    a = _Arr()
    a.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    with torch.cuda.device(device):
        return torch.as_tensor(a, device=device)


def stream_handle():
    """hipStream_t of torch's current stream, as void*."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
