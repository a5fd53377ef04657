"""Guarded device buffers of the GPU tests that call the C interface directly: an overrun shows as a changed byte, never as a
fault."""
import ctypes as C

import numpy as np

DEV = "cuda:0"
PAD = 256                  # guard bytes before and after every buffer
FILL = 0xA5                # guards and unwritten outputs


class Buf:
    """A device allocation of pad + nbytes + pad bytes (at least) filled with FILL; the payload optionally holds `host`.  With
    `skew` the payload starts that many bytes past a 256-byte boundary."""

    def __init__(self, shape, dtype, host=None, pad=PAD, skew=None):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.t = torch.full((self.nbytes + 2 * pad + (0 if skew is None else 256),), FILL, dtype=torch.uint8, device=DEV)
        self.at = pad if skew is None else pad + (skew - self.t.data_ptr() - pad) % 256
        if host is not None:
            host = np.array(host, dtype=self.dtype, order="C")       # (a copy: the shared clouds are read-only)
            assert host.shape == self.shape
            self.t[self.at:self.at + self.nbytes] = torch.from_numpy(host.reshape(-1).view(np.uint8)).to(DEV)
        self.ptr = C.c_void_p(self.t.data_ptr() + self.at)

    def get(self):
        """-> the payload; asserts both guards first."""
        raw = self.t.cpu().numpy()
        assert (raw[:self.at] == FILL).all() and (raw[self.at + self.nbytes:] == FILL).all(), "a guard changed"
        return raw[self.at:self.at + self.nbytes].view(self.dtype).reshape(self.shape)
