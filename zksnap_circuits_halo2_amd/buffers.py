"""`DeviceBuffer`: the one owner of `zkhip_alloc` memory in the package (no torch here: these buffers come from the C ABI)."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib


def _release(lib, ptr) -> None:
    if ptr:
        lib.zkhip_free(ptr)
        ptr.value = None


class DeviceBuffer:
    """`nbytes` of device memory: `ptr` is the c_void_p the library's calls take, `address` the same as an integer (None once freed).
    Freed by `free()`, by leaving the `with` block, or when the object is collected without either.  `zkhip_free` waits for the device."""

    def __init__(self, nbytes: int):
        self.lib = _lib.load()
        self.ptr = C.c_void_p()
        self.nbytes = nbytes
        _lib.check(self.lib.zkhip_alloc(nbytes, C.byref(self.ptr)))
        self._finalizer = weakref.finalize(self, _release, self.lib, self.ptr)
        self._finalizer.atexit = False          # at interpreter exit the process's memory goes with it; the library may be shut down by then

    @property
    def address(self):
        return self.ptr.value

    def upload(self, a: np.ndarray, offset: int = 0) -> None:
        a = np.ascontiguousarray(a)
        _lib.check(self.lib.zkhip_upload(C.c_void_p(self.ptr.value + offset), a.ctypes.data, a.nbytes))

    def download(self, shape, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype=np.uint64)
        _lib.check(self.lib.zkhip_download(out.ctypes.data, C.c_void_p(self.ptr.value + offset), out.nbytes))
        return out

    def free(self) -> None:
        self._finalizer()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
