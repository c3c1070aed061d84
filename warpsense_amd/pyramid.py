"""Coarser levels of the global map in device memory (ws_store_coarsen, include/warpsense_hip.h): the statistics of a call and the
call itself behind DeviceGlobalMap.coarsen, parents_of, MapPyramid, and global_pyramid of TSDFMapping."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._abi import _i3, _ptr, unpack_entry
from ._lib import check


@dataclass(frozen=True)
class CoarsenStats:
    """stats[4] of ws_store_coarsen"""
    chunks: int    # chunks of DST written
    created: int   # ... of which the call created
    valued: int    # coarse voxels that received a value
    short: int     # coarse voxels with 1 <= n < min_observed observed children

    def as_tuple(self):
        return (self.chunks, self.created, self.valued, self.short)


def _keys_array(keys):
    return np.ascontiguousarray(np.asarray(keys, dtype=np.int32).reshape(-1, 3))


def _coarsen_call(L, src, dst, keys, min_observed, stats):
    out = np.zeros(4, dtype=np.uint64) if stats else None
    k = None if keys is None else _keys_array(keys)
    check(L.ws_store_coarsen(dst.handle, src.handle, _ptr(k), 0 if k is None else len(k), int(min_observed), _lib.WS_COARSEN_DEFAULT, _ptr(out)),
          "ws_store_coarsen")
    return CoarsenStats(*(int(v) for v in out)) if stats else None


def parents_of(keys) -> np.ndarray:
    """host only: the (m, 3) parents k >> 1 of the (n, 3) chunk keys, unique and ascending (ws_store_parents_of)"""
    L = _lib.load()
    k = _keys_array(keys)
    n = C.c_size_t(0)
    check(L.ws_store_parents_of(_ptr(k), len(k), None, 0, C.byref(n)), "ws_store_parents_of")
    out = np.zeros((n.value, 3), dtype=np.int32)
    check(L.ws_store_parents_of(_ptr(k), len(k), _ptr(out), n.value, C.byref(n)), "ws_store_parents_of")
    return out


class MapPyramid:
    """`levels` coarser copies of a DeviceGlobalMap, each with twice the voxel edge of the one below (DeviceGlobalMap.coarsen).
    store(0) is `base`, which the pyramid does not own; store(l) is queried like any DeviceGlobalMap with resolution(l) =
    resolution << l: no query is duplicated.  The levels follow the base only when rebuild() or refresh() is called."""

    def __init__(self, base, levels: int, resolution: int, min_observed: int = 8, segment_chunks: int = 0):
        if int(levels) < 1:
            raise ValueError("MapPyramid: levels must be at least 1")
        self.base, self.levels, self.min_observed = base, int(levels), int(min_observed)
        self._resolution = int(resolution)
        value, weight = unpack_entry(base.default_raw)
        self._stores = [base] + [type(base)(int(value), int(weight), segment_chunks=segment_chunks, ctx=base.ctx) for _ in range(self.levels)]

    def store(self, level: int):
        return self._stores[level]

    def resolution(self, level: int) -> int:
        return self._resolution << level

    def rebuild(self, stats=True):
        """every level from the one below, over the parents of all its chunks; returns the CoarsenStats per level (None each
        with stats=False, which waits for nothing).  A chunk dropped from the base leaves its ancestors as they were: that wants
        refresh() of the dropped chunk's box."""
        return [self._stores[l - 1].coarsen(self._stores[l], None, self.min_observed, stats) for l in range(1, self.levels + 1)]

    def refresh(self, lo, hi, stats=True):
        """after a change of the base inside the inclusive box [lo, hi] of base voxels: level 1 recomputes the parents of the chunks
        the box overlaps, every level above the parents of those; nothing else is touched"""
        L, lo, hi, n = _lib.load(), _i3(lo), _i3(hi), C.c_size_t(0)
        check(L.ws_store_chunks_of_box(_ptr(lo), _ptr(hi), None, 0, C.byref(n)), "ws_store_chunks_of_box")
        keys = np.zeros((n.value, 3), dtype=np.int32)
        check(L.ws_store_chunks_of_box(_ptr(lo), _ptr(hi), _ptr(keys), n.value, C.byref(n)), "ws_store_chunks_of_box")
        out = []
        for l in range(1, self.levels + 1):
            keys = parents_of(keys)
            out.append(self._stores[l - 1].coarsen(self._stores[l], keys, self.min_observed, stats))
        return out

    def close(self):
        for s in self._stores[1:]:
            s.close()
        self._stores = self._stores[:1]


class PyramidQueries:
    """global_pyramid of TSDFMapping (mapping.py): the levels of detail of everything the run has seen"""

    def _pyramid_touch(self, lo=None, hi=None):
        """the base changed inside [lo, hi] (None: anywhere) since global_pyramid last ran"""
        if getattr(self, "_pyramid", None) is None:
            return
        if lo is None:
            self._pyramid_all = True
            return
        lo, hi, d = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64), self._pyramid_dirty
        self._pyramid_dirty = (lo, hi) if d is None else (np.minimum(d[0], lo), np.maximum(d[1], hi))

    def _level_mesh(self, level, **kw):
        """global_mesh(level=...): the mesh of store(level) of global_pyramid at resolution(level); the pyramid the mapping keeps is
        used if it has that many levels, else one of `level` levels is built.  lo and hi are voxels of that level."""
        p = getattr(self, "_pyramid", None)
        p = self.global_pyramid(max(level, p.levels if p is not None else 0), p.min_observed if p is not None else 8)
        with self.mutex_:
            return p.store(level).mesh(p.resolution(level), **kw)

    def global_pyramid(self, levels, min_observed=8, segment_chunks=0):
        """Coarser levels of everything the run has seen: the window goes into the chunks of device_global_map exactly as in
        global_mesh, then a MapPyramid over it is rebuilt (the first call, other levels or min_observed, or after merge_map) or
        refreshed over the windows the mapping has held since the last call.  Returns the pyramid, which the mapping keeps; chunks
        written into the store behind the mapping's back want MapPyramid.rebuild(); a chunk dropped from the store wants
        MapPyramid.refresh() of its box, which a rebuild does not cover."""
        with self._window_in_store("global_pyramid") as store:
            lo, hi = self.local_map_.window()
            p = getattr(self, "_pyramid", None)
            if p is None or p.base is not store or p.levels != int(levels) or p.min_observed != int(min_observed):
                if p is not None:
                    p.close()
                self._pyramid = p = MapPyramid(store, levels, int(self.params_.map.resolution), min_observed, segment_chunks)
                self._pyramid_all, self._pyramid_dirty = True, None
            self._pyramid_touch(lo, hi)
            if self._pyramid_all:
                p.rebuild(stats=False)
            else:
                p.refresh(*self._pyramid_dirty, stats=False)
            self._pyramid_all, self._pyramid_dirty = False, None
            return p
