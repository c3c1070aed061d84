"""What the tests of all five map queries (surface, mesh, ray cast, sample, distance) share: byte equality, the window of a map
and a box of its ring, the download of a device map, the digest the C++ drop-ins print, the unpacking of raw entries, and the
parser of include/warpsense_hip.h with the base table from C types to ctypes.  No GPU and no built library at import."""
import ctypes as C
import os
import re

import numpy as np


def ring_box(data, size, pos, offset, lo, hi):
    """values.value(x, y, z) for the inclusive box: HDF5LocalMap::get_index, z fastest"""
    size, pos, offset = (np.asarray(v, dtype=np.int64) for v in (size, pos, offset))
    ax = [(np.arange(lo[k], hi[k] + 1, dtype=np.int64) - pos[k] + offset[k] + size[k]) % size[k] for k in range(3)]
    return data.reshape(tuple(int(s) for s in size))[np.ix_(ax[0], ax[1], ax[2])]


def window(size, pos):
    """map.h:19-26: left = pos - size / 2, right = pos + size / 2 (odd sizes); for an even size each ring cell once"""
    size, pos = np.asarray(size, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    lo = pos - size // 2
    return lo, lo + size - 1


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def download(W, tm, lm, which=0):
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    (tm.tsdf().avg_map() if which == 0 else tm.tsdf().new_map()).to_host(host)
    return host


def wrapper(t, which):
    return t.avg_map() if which == 0 else t.new_map()


def fnv1a(b: bytes) -> int:
    h = 1469598103934665603
    for chunk in np.frombuffer(b, dtype=np.uint8).tolist():
        h = ((h ^ chunk) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def unpack(box):
    value = (box & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32)
    weight = (box >> 16).astype(np.uint16).view(np.int16).astype(np.int32)
    return value, weight


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "warpsense_hip.h")).read()


CTYPE = {"ws_map *": C.c_void_p, "const ws_map *": C.c_void_p, "int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "size_t": C.c_size_t,
         "const int32_t [3]": C.c_void_p, "float [3]": C.c_void_p, "void *": C.c_void_p, "uint32_t *": C.c_void_p, "size_t *": C.POINTER(C.c_size_t)}


def _declared(name):
    """(return type, [parameter types]) of `name` as the header declares it, parameter names stripped"""
    m = re.search(r"\n([A-Za-z_0-9 ]+?[ \*])" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    params = []
    for p in m.group(2).split(","):
        p = re.sub(r"/\*.*?\*/", "", p).strip()
        arr = re.search(r"\[(\d+)\]$", p)
        p = re.sub(r"\[\d+\]$", "", p).strip()
        t = re.sub(r"\b[a-z_0-9]+$", "", p).strip()  # drop the parameter's name
        params.append(t + (f" [{arr.group(1)}]" if arr else ""))
    return m.group(1).strip(), params
