"""What the GPU tests of the entry-point families share (imported by test modules; not a conftest): the sentinel-filled output buffer
between guard bands, the bit-for-bit comparison of a dict of outputs, and the kernels the library launched while a callable ran."""
import numpy as np
import torch

from musediffusion_amd import _lib

SENTINEL, GUARD = -77, 64


class Guarded:
    """a buffer of `shape` between two guard bands, all of it filled with `sentinel`; `ptr` is the buffer's first element"""

    def __init__(self, *shape, dtype=torch.int32, sentinel=SENTINEL):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.sentinel = sentinel
        self.buf = torch.full((self.n + 2 * GUARD,), sentinel, device="cuda", dtype=dtype)
        self.ptr = self.buf.data_ptr() + self.buf.element_size() * GUARD

    def get(self):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.sentinel).all() and (host[GUARD + self.n:] == self.sentinel).all(), "guard band written"
        return host[GUARD:GUARD + self.n].reshape(self.shape)


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(got, want, what=""):
    for name in got:
        assert np.array_equal(bits(got[name]), bits(want[name])), (what, name, np.argwhere(bits(got[name]) != bits(want[name]))[:5].tolist())


def library_launches(fn, strip=""):
    """the kernel texts of the launches the library made while fn ran, from its launch recorder.  A template instantiation is launched
    in parentheses: strip="()" takes them off"""
    return [r.kernel.strip(strip) for r in _lib.record_launches(fn)]
