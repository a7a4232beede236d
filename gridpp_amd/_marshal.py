"""Argument marshalling of the Python wrappers (the SWIG typemaps of swig/vector.i, plus the device path).

A field argument is anything numpy can convert (host path: staged through HBM by the library) or a torch CUDA tensor (device
path: the kernels read and write the tensor's HBM).  Every wrapper of gridpp_amd converts its fields with `field`, works out
the `mem` argument of its entry point with `flags` and, where the entry point ends in (..., out, mem), calls it with `run`.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _capi
from ._capi import check, lib


def _is_dev(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _wants_f64(*fields):
    """The large field arrays of a call are float64 numpy arrays: hand every input over as float64 (GPP_HOST_F64, cast on the
    device) instead of paying numpy's astype on them."""
    big = [a for a in fields if isinstance(a, np.ndarray) and a.size >= (1 << 20)]
    return bool(big) and all(a.dtype == np.float64 for a in big)


def _vec(a, ndim, name="array", dtype=np.float32):
    """Any dtype -> C-contiguous float32 (float64 in a GPP_HOST_F64 call); wrong ndim raises like the typemap (swig/vector.i:39-41)."""
    if _is_dev(a):
        import torch
        if a.dim() != ndim:
            raise RuntimeError("%s must have %d dimensions" % (name, ndim))
        return a.contiguous().to(torch.float32)
    arr = np.ascontiguousarray(np.asarray(a), dtype=dtype)
    if arr.ndim != ndim:
        if arr.size == 0 and arr.ndim <= ndim:   # e.g. [] or [[]]
            return arr.reshape((0,) * ndim)
        raise RuntimeError("%s must have %d dimensions, got %d" % (name, ndim, arr.ndim))
    return arr


def field(a, ndim=None, name="array", f64=False, dtype=None, dev_message=None):
    """The one conversion of a field argument.  None stays None; a torch CUDA tensor becomes contiguous float32 (int32 where
    `dtype` says so); anything else a C-contiguous numpy array of `dtype`, else float64 in an `f64` call, else float32 -- the
    same buffer where it already is one.  ndim: the rank to insist on, with _vec's rule and messages (dev_message: the text a
    device tensor of the wrong rank raises instead); None converts only, for a caller that accepts several ranks."""
    if a is None:
        return None
    if _is_dev(a):
        import torch
        if ndim is not None and a.dim() != ndim:
            raise RuntimeError(dev_message or "%s must have %d dimensions" % (name, ndim))
        return a.contiguous().to(torch.int32 if dtype == np.int32 else torch.float32)
    dtype = dtype or (np.float64 if f64 else np.float32)
    if ndim is None:
        return np.ascontiguousarray(np.asarray(a), dtype=dtype)
    return _vec(a, ndim, name, dtype)


def _ptr(a):
    if a is None:
        return None
    if _is_dev(a):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _shape(a):
    return tuple(a.shape)


def _ndim(a):
    return a.dim() if _is_dev(a) else np.ndim(a)


class _PinnedPool:
    """Result arrays of 1 MiB and more live in page-locked host memory (gpp_host_alloc): the device-to-host copy is then one
    DMA transfer.  Buffers return to a free list when their numpy array dies (up to 2 GiB are kept for reuse)."""
    MIN_BYTES, KEEP_BYTES = 1 << 20, 2 << 30

    def __init__(self):
        self.free, self.kept = {}, 0

    def take(self, nbytes):
        lst = self.free.get(nbytes)
        if lst:
            self.kept -= nbytes
            return lst.pop()
        ptr = C.c_void_p()
        if lib().gpp_host_alloc(nbytes, C.byref(ptr)) != _capi.GPP_OK or not ptr.value:
            return None
        return ptr.value

    def give(self, ptr, nbytes):
        if self.kept + nbytes <= self.KEEP_BYTES:
            self.free.setdefault(nbytes, []).append(ptr)
            self.kept += nbytes
        else:
            lib().gpp_host_free(C.c_void_p(ptr))


_pinned = _PinnedPool()


def _host_empty(shape):
    n = int(np.prod(shape))
    if 4 * n < _PinnedPool.MIN_BYTES or os.environ.get("GPP_PAGEABLE_RESULTS"):
        return np.empty(shape, dtype=np.float32)
    ptr = _pinned.take(4 * n)
    if ptr is None:
        return np.empty(shape, dtype=np.float32)
    buf = (C.c_float * n).from_address(ptr)
    weakref.finalize(buf, _pinned.give, ptr, 4 * n)
    return np.frombuffer(buf, dtype=np.float32).reshape(shape)     # the array keeps `buf` alive


def _empty_like_field(shape, like, dtype=np.float32):
    if _is_dev(like):
        import torch
        return torch.empty(shape, dtype=torch.int32 if dtype == np.int32 else torch.float32, device=like.device)
    if dtype == np.int32:
        return np.empty(shape, dtype=np.int32)
    return _host_empty(shape)


def _mem(*arrays):
    dev = [_is_dev(a) for a in arrays if a is not None]
    if any(dev) and not all(dev):
        raise ValueError("either all field arguments are torch CUDA tensors or none is")
    return _capi.MEM_DEVICE if dev and all(dev) else _capi.MEM_HOST


def _sync_if_dev(mem):
    if mem == _capi.MEM_DEVICE:
        import torch
        torch.cuda.current_stream().synchronize()   # producers of the inputs ran on torch's stream


def flags(f64, *fields):
    """The `mem` argument of a call on these fields (_mem's mixed-memory ValueError included).  Device fields: torch's current
    stream is synchronised first.  Host fields of an `f64` call (they were converted with field(..., f64=True)): GPP_HOST_F64."""
    mem = _mem(*fields)
    _sync_if_dev(mem)
    if f64 and mem == _capi.MEM_HOST:
        mem |= _capi.HOST_F64
    return mem


def run(entry, *args, out_shape, like, mem, dtype=np.float32):
    """Calls an entry point that ends in (..., out, mem) and returns its result, allocated where `like` lives (dtype: np.int32 for an
    entry point that writes int32)."""
    out = _empty_like_field(out_shape, like, dtype)
    check(entry(*args, _ptr(out), mem))
    return out


def _out_shape(o):
    """the shape of a field on a Grid, whose size() is [Y, X], or on a Points, whose size() is N"""
    size = o.size()
    return tuple(size) if isinstance(size, list) else (size,)
