"""CPU tests of the device global map's host side (ws_store_*, include/warpsense_hip.h): the chunk keys of a box against
np.floor_divide, and that every new symbol is declared, bound and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from window_host_routes import expected_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ws_store_create", "ws_store_destroy", "ws_store_reserve", "ws_store_count", "ws_store_keys", "ws_store_has", "ws_store_get_chunk",
       "ws_store_put_chunk", "ws_store_drop_chunk", "ws_store_chunk_dev", "ws_store_save_box", "ws_store_load_box", "ws_shift_device",
       "ws_store_chunks_of_box", "ws_debug_store_timing", "ws_shift_plan"]
WS_ERR_INVALID = -1


def _i3(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


BOXES = [((-100, -1, 0), (70, 64, 63)),          # negative coordinates, and chunk borders inside
         ((-64, -128, -65), (-1, -65, -64)),     # exactly one chunk in x, one in y, two in z: all negative
         ((0, 64, 128), (63, 127, 191)),         # exactly on chunk borders: one chunk
         ((63, 63, 63), (64, 64, 64)),           # two voxels across a border in every axis: eight chunks
         ((-1, -1, -1), (0, 0, 0)),              # the same around the origin
         ((5, -7, 200), (5, -7, 200)),           # one voxel
         ((-64, 0, 0), (-64, 0, 0)),             # one voxel, the first of a negative chunk
         ((-65, 0, 0), (-65, 0, 0)),             # ... and the last of the one before
         ((-513, -512, -40), (511, 512, -1))]    # a z slab of a 1025^3 window


@pytest.mark.parametrize("lo,hi", BOXES)
def test_chunks_of_box_equals_floor_divide(lo, hi):
    from warpsense_amd import _lib
    import warpsense_amd as W
    L = _lib.load()
    want = expected_keys(lo, hi)
    n = C.c_size_t(0)
    assert L.ws_store_chunks_of_box(_p(_i3(lo)), _p(_i3(hi)), None, 0, C.byref(n)) == 0 and n.value == len(want)
    got = np.full((len(want) + 1, 3), 12345, dtype=np.int32)
    assert L.ws_store_chunks_of_box(_p(_i3(lo)), _p(_i3(hi)), _p(got), len(want) + 1, C.byref(n)) == 0 and n.value == len(want)
    assert np.array_equal(got[:-1], want) and np.all(got[-1] == 12345)
    assert [tuple(k) for k in got[:-1]] == sorted(tuple(k) for k in want)  # ascending (cx, cy, cz)
    # a capacity that is too small: a prefix, and still the whole count
    if len(want) > 1:
        part = np.full((len(want), 3), 12345, dtype=np.int32)
        n.value = 0
        assert L.ws_store_chunks_of_box(_p(_i3(lo)), _p(_i3(hi)), _p(part), len(want) - 1, C.byref(n)) == 0 and n.value == len(want)
        assert np.array_equal(part[:-1], want[:-1]) and np.all(part[-1] == 12345)
    assert np.array_equal(W.chunks_of_box(lo, hi), want)


def test_chunks_of_box_refuses_an_empty_box():
    from warpsense_amd import _lib
    L = _lib.load()
    n = C.c_size_t(77)
    assert L.ws_store_chunks_of_box(_p(_i3((0, 0, 1))), _p(_i3((0, 0, 0))), None, 0, C.byref(n)) == WS_ERR_INVALID and n.value == 77
    assert L.ws_store_chunks_of_box(None, _p(_i3((0, 0, 0))), None, 0, C.byref(n)) == WS_ERR_INVALID


def test_store_symbols_are_declared_bound_and_exported():
    from warpsense_amd import _lib
    import warpsense_amd as W
    header = open(os.path.join(ROOT, "include", "warpsense_hip.h")).read()
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", header))
    L = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name  # in the ctypes table
    assert "typedef struct ws_store ws_store;" in header
    assert W.DeviceGlobalMap is not None and "DeviceGlobalMap" in W.__all__
    for method in ("keys", "has_chunk", "chunk", "put_chunk", "drop_chunk", "count", "reserve", "flush_to", "load_from", "close"):
        assert callable(getattr(W.DeviceGlobalMap, method)), method
    assert callable(W.TSDFMapping.shift_map_device)
