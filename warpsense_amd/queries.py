"""What the window map (ws_map_*) and the chunk store (ws_store_*) share on the host side of their queries: the box, the call,
the download or the device tensors of surface, mesh, ray cast, point sample, distance field, frontier, reach and view gain, and the
timing read-out."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import _device_tensor, _i3, _is_device, _ptr
from ._lib import WsError, check
from .records import VIEW_GAIN_RAY, VIEW_GAIN_RECORD, FRONTIER_CLUSTER, FRONTIER_RECORD, REACH_PATH_HEADER, REACH_PATH_RECORD, RAY, SAMPLE, SAMPLE_CLASSES, SURFACE_RECORD, VERT
from .scan import DevicePoints


def _box_ptrs(what, lo, hi):
    """The two box arguments of a query of `what` ("surface", "mesh", ...): pointers to three int32 each, or None, None for the
    query's default box."""
    if (lo is None) != (hi is None):
        raise WsError(f"{what}: give both lo and hi, or neither")
    return _ptr(_i3(lo)) if lo is not None else None, _ptr(_i3(hi)) if hi is not None else None


def _timing(L, name, handle, n, enable):
    """The n device milliseconds that the debug entry `name` (ws_debug_*_timing) keeps for the last call on `handle`."""
    ms = (C.c_float * n)()
    check(getattr(L, name)(handle, int(enable), ms), name)
    return tuple(float(v) for v in ms)


def _surface_call(L, name, owner, lead, lo, hi, band, tail, marker, device):
    """The surface call `name` (ws_map_surface, ws_store_surface) on owner.handle and its result: `lead` are the arguments of the entry
    point before the box, `tail` those between the band and the flags.  owner keeps the device tensors' memory alive."""
    box = _box_ptrs("surface", lo, hi)
    n = C.c_size_t(0)
    flags = _lib.WS_SURFACE_MARKER if marker else _lib.WS_SURFACE_RECORDS
    check(getattr(L, name)(owner.handle, *lead, *box, int(band) if band is not None else 0, *tail, flags, C.byref(n)), name)
    n = int(n.value)
    if device:
        cnt = C.c_size_t(0)
        rec = _device_tensor(getattr(L, name + "_records_dev")(owner.handle, C.byref(cnt)), (n, 4), "<i4", owner)
        if not marker:
            return rec
        return rec, _device_tensor(getattr(L, name + "_marker_dev")(owner.handle, C.byref(cnt)), (n, 7), "<f4", owner)
    rec = np.empty(n, dtype=SURFACE_RECORD)
    mk = np.empty((n, 7), dtype=np.float32) if marker else None
    got = C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), _ptr(mk), n, C.byref(got)), name + "_download")
    if int(got.value) != n:
        raise WsError("surface: another call replaced the result before it was downloaded")
    return (rec, mk) if marker else rec


def _mesh_call(L, name, owner, lead, lo, hi, tail, any_weight, device):
    """The mesh call `name` (ws_map_mesh, ws_store_mesh) on owner.handle and its result: `lead` and `tail` are the arguments of the
    entry point before and behind the box.  owner keeps the device tensors' memory alive."""
    box = _box_ptrs("mesh", lo, hi)
    nv, nf = C.c_size_t(0), C.c_size_t(0)
    flags = _lib.WS_MESH_ANY_WEIGHT if any_weight else _lib.WS_MESH_DEFAULT
    check(getattr(L, name)(owner.handle, *lead, *box, *tail, flags, C.byref(nv), C.byref(nf)), name)
    nv, nf = int(nv.value), int(nf.value)
    if device:
        cnt = C.c_size_t(0)
        return (_device_tensor(getattr(L, name + "_vertices_dev")(owner.handle, C.byref(cnt)), (nv, 4), "<i4", owner),
                _device_tensor(getattr(L, name + "_faces_dev")(owner.handle, C.byref(cnt)), (nf, 3), "<i4", owner))
    vert, face = np.empty(nv, dtype=VERT), np.empty((nf, 3), dtype=np.uint32)
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(vert), _ptr(face), nv, nf, C.byref(gv), C.byref(gf)), name + "_download")
    if (int(gv.value), int(gf.value)) != (nv, nf):
        raise WsError("mesh: another call replaced the result before it was downloaded")
    return vert, face


def _raycast_call(L, name, handle, lead, origin_mm, dirs, max_range_mm, tail, any_weight, gradient, targets):
    """The ray cast `name` (ws_map_raycast, ws_store_raycast; name + "_dev" for directions on the device) and its download: `lead` are
    the arguments of the entry point before the origin, `tail` those between the range and the flags.  Returns (records, gradient |
    None, hits)."""
    n = int(dirs.shape[0])
    flags = ((_lib.WS_RAYCAST_ANY_WEIGHT if any_weight else 0) | (_lib.WS_RAYCAST_GRADIENT if gradient else 0)
             | (_lib.WS_RAYCAST_TARGETS if targets else 0))
    hits = C.c_size_t(0)
    if _is_device(dirs):
        name_call, d = name + "_dev", dirs
    else:
        name_call, d = name, np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 3)
    check(getattr(L, name_call)(handle, *lead, _ptr(_i3(origin_mm)), _ptr(d), n, int(max_range_mm), *tail, flags, C.byref(hits)), name_call)
    rec = np.empty(n, dtype=RAY)
    grad = np.empty((n, 3), dtype=np.int32) if gradient else None
    got = C.c_size_t(0)
    check(getattr(L, name + "_download")(handle, _ptr(rec), _ptr(grad), n, C.byref(got)), name + "_download")
    if int(got.value) != n:
        raise WsError("raycast: another call replaced the result before it was downloaded")
    return rec, grad, int(hits.value)


class _SampleSelection:
    """what keeps the selection of a sample call reachable as DevicePoints: the owner of the buffers, and the way back to the host"""

    def __init__(self, L, name, owner, n_sel):
        self._L, self._name, self._owner, self._n = L, name, owner, int(n_sel)

    def download(self) -> np.ndarray:
        out = np.empty((self._n, 3), dtype=np.int32)
        n, ns = C.c_size_t(0), C.c_size_t(0)
        check(getattr(self._L, self._name + "_download")(self._owner.handle, None, None, _ptr(out), 0, self._n, C.byref(n), C.byref(ns)), self._name + "_download")
        if int(ns.value) != self._n:
            raise WsError("sample: another call replaced the selection before it was downloaded")
        return out


def _sample_flags(any_weight, gradient, select):
    flags = (_lib.WS_SAMPLE_ANY_WEIGHT if any_weight else 0) | (_lib.WS_SAMPLE_GRADIENT if gradient else 0)
    for name in ([select] if isinstance(select, str) else (select or ())):
        if name not in SAMPLE_CLASSES:
            raise WsError(f"sample: select names classes out of {SAMPLE_CLASSES}, not {name!r}")
        flags |= _lib.WS_SAMPLE_SELECT_UNKNOWN << SAMPLE_CLASSES.index(name)
    return flags


def _sample_call(L, name, owner, lead, points, band_mm, tail, any_weight, gradient, select, device):
    """The point sample `name` (ws_map_sample, ws_store_sample; name + "_dev" for points on the device) on owner.handle and its
    result: `lead` are the arguments of the entry point before the points, `tail` those between the band and the flags.  Returns
    (records, counts, gradient | None, selection | None); owner keeps device results' memory alive."""
    n = int(points.shape[0])
    flags = _sample_flags(any_weight, gradient, select)
    selecting = (flags >> 2) != 0
    counts = np.zeros(4, dtype=np.uint64)
    if _is_device(points):
        name_call, pts = name + "_dev", points
    else:
        name_call, pts = name, np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 3)
    check(getattr(L, name_call)(owner.handle, *lead, _ptr(pts), n, int(band_mm), *tail, flags, _ptr(counts)), name_call)
    n_sel = int(sum(int(counts[c]) for c in range(4) if (flags >> (2 + c)) & 1))
    cnt = C.c_size_t(0)
    if device:
        rec = _device_tensor(getattr(L, name + "_records_dev")(owner.handle, C.byref(cnt)), (n, 4), "<i4", owner)
        if int(cnt.value) != n:
            raise WsError("sample: another call replaced the result")
        grad = _device_tensor(getattr(L, name + "_gradient_dev")(owner.handle, C.byref(cnt)), (n, 3), "<i4", owner) if gradient else None
        sel = DevicePoints(getattr(L, name + "_selected_dev")(owner.handle, C.byref(cnt)) or 0, n_sel, _SampleSelection(L, name, owner, n_sel)) if selecting else None
        return rec, counts, grad, sel
    rec = np.empty(n, dtype=SAMPLE)
    grad = np.empty((n, 3), dtype=np.int32) if gradient else None
    sel = np.empty((n_sel, 3), dtype=np.int32) if selecting else None
    got, got_sel = C.c_size_t(0), C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), _ptr(grad), _ptr(sel), n, n_sel, C.byref(got), C.byref(got_sel)), name + "_download")
    if int(got.value) != n or (selecting and int(got_sel.value) != n_sel):
        raise WsError("sample: another call replaced the result before it was downloaded")
    return rec, counts, grad, sel


def _distance_call(L, name, owner, lead, lo, hi, max_dist_vox, unknown_occupied, columns, any_weight, device, default_shape):
    """The distance call `name` (ws_map_distance, ws_store_distance) on owner.handle and its result: `lead` are the arguments of the
    entry point before the box, default_shape() the extent of the box that lo = hi = None stands for.  owner keeps a device tensor's
    memory alive.  Returns (records, sites)."""
    box = _box_ptrs("distance", lo, hi)
    flags = ((_lib.WS_DISTANCE_ANY_WEIGHT if any_weight else 0) | (_lib.WS_DISTANCE_UNKNOWN_OCCUPIED if unknown_occupied else 0)
             | (_lib.WS_DISTANCE_COLUMNS if columns else 0))
    if lo is not None:
        shape = tuple(int(v) for v in (_i3(hi).astype(np.int64) - _i3(lo).astype(np.int64) + 1))
    else:
        shape = default_shape()
    sites = C.c_size_t(0)
    check(getattr(L, name)(owner.handle, *lead, *box, int(max_dist_vox), flags, C.byref(sites)), name)
    if columns:
        shape = shape[:2]
    n = int(np.prod(shape, dtype=np.int64))
    cnt = C.c_size_t(0)
    if device:
        ptr = getattr(L, name + "_dev")(owner.handle, C.byref(cnt))
        if int(cnt.value) != n:
            raise WsError("distance: another call replaced the result")
        return _device_tensor(ptr, shape, "<i4", owner), int(sites.value)
    rec = np.empty(n, dtype=np.uint32)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), n, C.byref(cnt)), name + "_download")
    if int(cnt.value) != n:
        raise WsError("distance: another call replaced the result before it was downloaded")
    return rec.reshape(shape), int(sites.value)


def _frontier_call(L, name, owner, lead, lo, hi, min_value, any_weight, clusters, device):
    """The frontier call `name` (ws_map_frontier, ws_store_frontier) on owner.handle and its result: `lead` are the arguments of the
    entry point before the box.  Returns the records, or with `clusters` (records, labels, table); owner keeps the device tensors'
    memory alive."""
    box = _box_ptrs("frontier", lo, hi)
    n, k = C.c_size_t(0), C.c_size_t(0)
    flags = (_lib.WS_FRONTIER_ANY_WEIGHT if any_weight else 0) | (_lib.WS_FRONTIER_CLUSTERS if clusters else 0)
    check(getattr(L, name)(owner.handle, *lead, *box, int(min_value), flags, C.byref(n), C.byref(k)), name)
    n, k = int(n.value), int(k.value)
    if device:
        cnt = C.c_size_t(0)
        rec = _device_tensor(getattr(L, name + "_records_dev")(owner.handle, C.byref(cnt)), (n, 4), "<i4", owner)
        if int(cnt.value) != n:
            raise WsError("frontier: another call replaced the result")
        if not clusters:
            return rec
        return (rec, _device_tensor(getattr(L, name + "_labels_dev")(owner.handle, C.byref(cnt)), (n,), "<i4", owner),
                _device_tensor(getattr(L, name + "_clusters_dev")(owner.handle, C.byref(cnt)), (k, 16), "<i4", owner))
    rec = np.empty(n, dtype=FRONTIER_RECORD)
    labels = np.empty(n, dtype=np.uint32) if clusters else None
    table = np.empty(k, dtype=FRONTIER_CLUSTER) if clusters else None
    got, got_k = C.c_size_t(0), C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), _ptr(labels), _ptr(table), n, k, C.byref(got), C.byref(got_k)), name + "_download")
    if int(got.value) != n or (clusters and int(got_k.value) != k):
        raise WsError("frontier: another call replaced the result before it was downloaded")
    return (rec, labels, table) if clusters else rec


def _reach_call(L, name, owner, seeds, clear_d2, unknown_free, max_rounds, device):
    """The reach call `name` (ws_map_reach, ws_store_reach) on owner.handle, over the owner's last distance result.  Returns (costs,
    info): one uint32 cost per record of that result, shaped like it ((nx, ny, nz), or (nx, ny) for a column map: the box the
    reach result carries, name + "_box"), and info = dict(seeded, reached, rounds).  owner keeps a device tensor's memory alive."""
    seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
    kept, reached, rounds = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0)
    flags = _lib.WS_REACH_UNKNOWN_FREE if unknown_free else 0
    check(getattr(L, name)(owner.handle, _ptr(seeds), len(seeds), int(clear_d2), flags, int(max_rounds), C.byref(kept), C.byref(reached), C.byref(rounds)), name)
    info = dict(seeded=int(kept.value), reached=int(reached.value), rounds=int(rounds.value))
    cnt = C.c_size_t(0)
    ptr = getattr(L, name + "_dev")(owner.handle, C.byref(cnt))
    n = int(cnt.value)
    ext, columns = np.zeros(3, dtype=np.uint32), C.c_int32(0)
    check(getattr(L, name + "_box")(owner.handle, None, _ptr(ext), C.byref(columns)), name + "_box")
    shape = tuple(int(v) for v in (ext[:2] if columns.value else ext))
    if int(np.prod(shape, dtype=np.int64)) != n:
        raise WsError("reach: another call replaced the result")
    if device:
        return _device_tensor(ptr, shape, "<i4", owner), info
    cost = np.empty(n, dtype=np.uint32)
    check(getattr(L, name + "_download")(owner.handle, _ptr(cost), n, C.byref(cnt)), name + "_download")
    if int(cnt.value) != n:
        raise WsError("reach: another call replaced the result before it was downloaded")
    return cost.reshape(shape), info


def _reach_lookup_call(L, name, owner, points):
    """The costs of the owner's reach result at `points` (name: ws_map_reach_lookup, ws_store_reach_lookup): an (n, 3) or (n, 4) int32
    numpy array -> uint32 numpy array; a CUDA tensor of such rows (the records of a frontier call with device=True) -> an int32 CUDA
    tensor of the same bits, through the _dev form."""
    if _is_device(points):
        import torch
        n, stride = int(points.shape[0]), int(points.shape[1])
        out = torch.empty(n, dtype=torch.int32, device=points.device)
        check(getattr(L, name + "_dev")(owner.handle, _ptr(points), n, stride, _ptr(out)), name + "_dev")
        return out
    points = np.ascontiguousarray(points, dtype=np.int32)
    points = points.reshape(-1, points.shape[-1] if points.ndim == 2 else 3)
    out = np.empty(len(points), dtype=np.uint32)
    check(getattr(L, name)(owner.handle, _ptr(points), len(points), int(points.shape[1]), _ptr(out)), name)
    return out


def _reach_paths_call(L, name, owner, goals, cap_steps):
    """The paths of the owner's reach result from `goals` ((g, 3) int32 world voxels) back to a seed.  Returns (headers, records): dtype
    REACH_PATH_HEADER [g] and REACH_PATH_RECORD [g, cap_steps] (the first headers["written"][i] of row i are the path, goal first)."""
    goals = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 3)
    hdr = np.zeros(len(goals), dtype=REACH_PATH_HEADER)
    rec = np.zeros((len(goals), int(cap_steps)), dtype=REACH_PATH_RECORD)
    if len(goals):
        check(getattr(L, name)(owner.handle, _ptr(goals), len(goals), int(cap_steps), _ptr(hdr), _ptr(rec) if cap_steps else None), name)
    return hdr, rec


def _view_gain_call(L, name, owner, lead, lo, hi, origins_mm, dirs, max_range_mm, tail, min_value, any_weight, rays, device):
    """The view-gain call `name` (ws_map_view_gain, ws_store_view_gain) on owner.handle and its result: `lead` are the arguments of the
    entry point before the box, `tail` those between the range and min_value.  Returns (records, rays | None, best): one
    VIEW_GAIN_RECORD per origin, with `rays` a (views, rays) array of VIEW_GAIN_RAY, and the largest unknown_k2; device=True: torch
    int32 tensors on the GPU instead -- (views, 8) and (views, rays, 2) -- that alias the library's buffers.  No origin or no
    direction: empty arrays, nothing is called."""
    box = _box_ptrs("view_gain", lo, hi)
    org = np.ascontiguousarray(origins_mm, dtype=np.int32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 3)
    m, n = len(org), len(d)
    if m == 0 or n == 0:
        return np.zeros(m if n else 0, dtype=VIEW_GAIN_RECORD), (np.zeros((m, n), dtype=VIEW_GAIN_RAY) if rays else None), 0
    flags = (_lib.WS_GAIN_ANY_WEIGHT if any_weight else 0) | (_lib.WS_GAIN_RAYS if rays else 0)
    best = C.c_uint64(0)
    check(getattr(L, name)(owner.handle, *lead, *box, _ptr(org), m, _ptr(d), n, int(max_range_mm), *tail, int(min_value), flags, C.byref(best)), name)
    cnt = C.c_size_t(0)
    if device:
        rec = _device_tensor(getattr(L, name + "_records_dev")(owner.handle, C.byref(cnt)), (m, 8), "<i4", owner)
        if int(cnt.value) != m:
            raise WsError("view_gain: another call replaced the result")
        ray = _device_tensor(getattr(L, name + "_rays_dev")(owner.handle, C.byref(cnt)), (m, n, 2), "<i4", owner) if rays else None
        return rec, ray, int(best.value)
    rec = np.empty(m, dtype=VIEW_GAIN_RECORD)
    ray = np.empty((m, n), dtype=VIEW_GAIN_RAY) if rays else None
    got, got_r = C.c_size_t(0), C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), _ptr(ray), m, m * n if rays else 0, C.byref(got), C.byref(got_r)), name + "_download")
    if int(got.value) != m or (rays and int(got_r.value) != m * n):
        raise WsError("view_gain: another call replaced the result before it was downloaded")
    return rec, ray, int(best.value)
