"""Guarded buffers and status-returning calls for tests that drive a kernel through the raw C ABI.

A ``Guarded`` array is a slice of a larger byte buffer filled with one sentinel byte: 256 bytes (64 float32) in front of it, ``off``
elements of misalignment, the array, and at least 256 bytes behind it.  The buffer starts 16-byte aligned, so the array starts
``off`` elements past a 16-byte boundary.  ``guards_ok()`` is true while nothing but the array itself was written;
``untouched()`` while not even the array was."""
import ctypes as C

import torch

GUARD_BYTES = 256
FILL = 0xA5


class Guarded:
    def __init__(self, numel, dtype, dev, off=0, init=None):
        item = torch.empty(0, dtype=dtype).element_size()
        self.nbytes = int(numel) * item
        self.start = GUARD_BYTES + int(off) * item
        total = (self.start + self.nbytes + GUARD_BYTES + 15) // 16 * 16
        self.raw = torch.full((total,), FILL, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.t = self.raw[self.start:self.start + self.nbytes].view(dtype)
        self.ptr = self.raw.data_ptr() + self.start
        if init is not None:
            self.t.copy_(init.reshape(-1))

    def guards_ok(self) -> bool:
        a, b = self.raw[:self.start], self.raw[self.start + self.nbytes:]
        return bool((a == FILL).all()) and bool((b == FILL).all())

    def untouched(self) -> bool:
        return bool((self.raw == FILL).all())

    def cpu(self):
        return self.t.cpu()


def raw_call(backend, fn, args) -> int:
    """``gf_<fn>`` (HIP library, torch's current stream) or ``gfo_<fn>`` (CPU oracle): the status code, not an exception."""
    if backend.name == "hip":
        f = getattr(backend.lib, "gf_" + fn)
        f.restype = C.c_int
        return f(C.byref(args), C.c_void_p(backend._stream()))
    f = getattr(backend.lib, "gfo_" + fn)
    f.restype = C.c_int
    return f(C.byref(args))


def sync(dev) -> None:
    if dev != "cpu":
        torch.cuda.synchronize()
