"""The ctypes glue under every module of the package: pointers, the three-int and column-major forms of the C ABI
(include/warpsense_hip.h), the packed TSDF entry, and library-owned device buffers as torch tensors."""
from __future__ import annotations

import ctypes as C

import numpy as np

MATRIX_RESOLUTION = 32768  # include/warpsense/consts.h:12-13
WEIGHT_RESOLUTION = 64     # include/warpsense/consts.h:9-10


def _ptr(a):
    """void* of a numpy array, a ctypes array or a torch tensor (host or device)."""
    if a is None:
        return None
    if isinstance(a, C.Array):
        return a
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _is_device(a) -> bool:
    return hasattr(a, "is_cuda") and bool(a.is_cuda)


_I3 = C.c_int32 * 3


def _i3(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(3))


def _i3c(v):
    """three int32 for the C ABI only; tuples and lists skip numpy (this sits between two scans of a stream)"""
    if isinstance(v, (tuple, list)) and len(v) == 3:
        return _I3(int(v[0]), int(v[1]), int(v[2]))
    return _i3(v)


def _colmajor(T) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(4, 4).T).reshape(16)


def pack_entry(value, weight):
    """TSDFEntry raw word: low 16 bits value, high 16 bits weight (include/map/tsdf.h:16-23)."""
    v = np.asarray(value).astype(np.int16).astype(np.uint16).astype(np.uint32)
    w = np.asarray(weight).astype(np.int16).astype(np.uint16).astype(np.uint32)
    return v | (w << np.uint32(16))


def unpack_entry(raw):
    raw = np.asarray(raw, dtype=np.uint32)
    return (raw & 0xFFFF).astype(np.uint16).astype(np.int16), (raw >> 16).astype(np.uint16).astype(np.int16)


class _DeviceArray:
    """a library-owned device buffer as torch sees it (__cuda_array_interface__); `owner` keeps the handle alive"""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        self._owner = owner


def _device_tensor(ptr, shape, typestr: str, owner):
    import torch
    if not ptr or shape[0] == 0:
        return torch.empty(shape, dtype=torch.int32 if typestr == "<i4" else torch.float32, device="cuda")
    return torch.as_tensor(_DeviceArray(ptr, shape, typestr, owner), device="cuda")
