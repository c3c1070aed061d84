"""The sliding window: DeviceMap (the host view), LocalMap (the host ring buffer), and the device copies a TSDFCuda owns
(DeviceMapMemWrapper) with the TSDF update (ws_map_*, ws_tsdf_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import _i3, _i3c, _is_device, _ptr, pack_entry, unpack_entry
from ._lib import WS_MAP_AVG, WS_MAP_NEW, check
from .clearance import _clearance_call
from .context import Context
from .global_map import GlobalMap
from .ground import _ground_call, _ground_distance_call
from .queries import _distance_call, _frontier_call, _reach_call, _reach_lookup_call, _reach_paths_call, _mesh_call, _raycast_call, _sample_call, _surface_call, _timing, _view_gain_call


class DeviceMap:
    """Non-owning view of a ring-buffer local map in HOST memory: size, offset, data, pos
    (include/warpsense/cuda/device_map.h:32-48).  The arrays are shared with whoever owns the map."""

    def __init__(self, size, offset, data, pos):
        self.size_ = np.asarray(size, dtype=np.int32).reshape(3)
        self.offset_ = np.asarray(offset, dtype=np.int32).reshape(3)
        self.pos_ = np.asarray(pos, dtype=np.int32).reshape(3)
        self.data_ = data
        if data is not None:
            assert data.dtype == np.uint32 and data.flags["C_CONTIGUOUS"]
            assert data.size == int(np.prod(self.size_.astype(np.int64)))

    def n_voxels(self) -> int:
        return int(np.prod(self.size_.astype(np.int64)))


class LocalMap:
    """HDF5LocalMap without the file (src/map/hdf5_local_map.cpp): a 3-D ring buffer of TSDF entries around `pos`.
    Sizes are forced odd, offset = size/2, every voxel starts as the global map's default entry (:5-20);
    shift() moves the window, saving the slabs that leave to the global map and loading the ones that enter
    (:53-118).  Owns the host arrays a DeviceMap views."""

    def __init__(self, sx, sy, sz, default_value, default_weight=0, global_map: GlobalMap | None = None, host_voxels: bool = True):
        self.size = np.array([s if s % 2 == 1 else s + 1 for s in (int(sx), int(sy), int(sz))], dtype=np.int32)
        self.pos = np.zeros(3, dtype=np.int32)
        self.offset = (self.size // 2).astype(np.int32)
        self.map_ = global_map or GlobalMap(default_value, default_weight)
        # host_voxels=False: the window lives on the device only (a 2049^3 window is 34 GB; the device-side shift and
        # export never need the host copy)
        self.data = np.full(int(np.prod(self.size.astype(np.int64))), self.map_.default_raw, dtype=np.uint32) if host_voxels else None

    def device_map(self) -> DeviceMap:
        return DeviceMap(self.size, self.offset, self.data, self.pos)

    def get_index(self, x, y, z) -> int:
        s, p, o = self.size.astype(np.int64), self.pos.astype(np.int64), self.offset.astype(np.int64)
        xi = (x - p[0] + o[0] + s[0]) % s[0]
        yi = (y - p[1] + o[1] + s[1]) % s[1]
        zi = (z - p[2] + o[2] + s[2]) % s[2]
        return int((xi * s[1] + yi) * s[2] + zi)

    def in_bounds(self, x, y, z) -> bool:
        d = np.abs(np.array([x, y, z], dtype=np.int64) - self.pos)
        return bool(np.all(d <= self.size // 2))

    def value(self, x, y, z):
        if not self.in_bounds(x, y, z):
            raise IndexError(f"Index out of bounds: {x}; {y}; {z}")  # std::out_of_range, hdf5_local_map.h:172-181
        v, w = unpack_entry(self.data[self.get_index(x, y, z)])
        return int(v), int(w)

    def set_value(self, x, y, z, value, weight):
        if not self.in_bounds(x, y, z):
            raise IndexError(f"Index out of bounds: {x}; {y}; {z}")
        self.data[self.get_index(x, y, z)] = pack_entry(value, weight)

    # -- save_load_area<save> (hdf5_local_map.cpp:120-198): one pass per 64^3 chunk the box touches
    def _area(self, start, end, save: bool):
        cs = GlobalMap.CHUNK_SIZE
        start, end = np.minimum(start, end).astype(np.int64), np.maximum(start, end).astype(np.int64)
        s, p, o = self.size.astype(np.int64), self.pos.astype(np.int64), self.offset.astype(np.int64)
        c0, c1 = np.floor_divide(start, cs), np.floor_divide(end, cs)
        for cx in range(c0[0], c1[0] + 1):
            for cy in range(c0[1], c1[1] + 1):
                for cz in range(c0[2], c1[2] + 1):
                    chunk = self.map_.activate_chunk(cx, cy, cz)
                    base = np.array([cx, cy, cz], dtype=np.int64) * cs
                    lo = np.maximum(start, base) - base
                    hi = np.minimum(end, base + cs - 1) - base
                    d = [np.arange(lo[k], hi[k] + 1, dtype=np.int64) for k in range(3)]
                    g = [d[k] + base[k] for k in range(3)]
                    r = [(g[k] - p[k] + o[k] + s[k]) % s[k] for k in range(3)]
                    ring = ((r[0][:, None, None] * s[1] + r[1][None, :, None]) * s[2] + r[2][None, None, :]).reshape(-1)
                    loc = (d[0][:, None, None] * cs * cs + d[1][None, :, None] * cs + d[2][None, None, :]).reshape(-1)
                    if save:
                        chunk[loc] = self.data[ring]
                    else:
                        self.data[ring] = chunk[loc]

    def shift(self, new_pos):
        """HDF5LocalMap::shift (hdf5_local_map.cpp:53-118), axis by axis."""
        new_pos = np.asarray(new_pos, dtype=np.int64)
        diff = new_pos - self.pos
        assert np.all(np.abs(diff) <= self.size)
        for axis in range(3):
            if diff[axis] == 0:
                continue
            start = self.pos.astype(np.int64) - self.size // 2
            end = self.pos.astype(np.int64) + self.size // 2
            if diff[axis] > 0:
                end[axis] = start[axis] + diff[axis] - 1
            else:
                start[axis] = end[axis] + diff[axis] + 1
            self._area(start, end, save=True)
            self.pos[axis] += diff[axis]
            self.offset[axis] = (self.offset[axis] + diff[axis] + self.size[axis]) % self.size[axis]
            start = self.pos.astype(np.int64) - self.size // 2
            end = self.pos.astype(np.int64) + self.size // 2
            if diff[axis] > 0:
                start[axis] = end[axis] - (diff[axis] - 1)
            else:
                end[axis] = start[axis] - diff[axis] - 1
            self._area(start, end, save=False)

    def window(self):
        """(lo, hi) of the window in world voxels, every ring cell once: pos - size/2 .. pos - size/2 + size - 1"""
        lo = self.pos.astype(np.int64) - self.size.astype(np.int64) // 2
        return lo, lo + self.size.astype(np.int64) - 1

    def follow(self, new_pos):
        """pos / offset after a shift the device has made (the data, if any, is not touched)"""
        new_pos = np.asarray(new_pos, dtype=np.int64)
        self.offset[:] = (self.offset + (new_pos - self.pos)) % self.size  # (numpy's % is >= 0 for a negative d)
        self.pos[:] = new_pos

    def write_back(self):
        """hdf5_local_map.cpp:210-217: save the whole window to the global map."""
        self._area(self.pos.astype(np.int64) - self.size // 2, self.pos.astype(np.int64) + self.size // 2, save=True)


class DeviceMapMemWrapper:
    """Device copy of one map (device_map_wrapper.h:10-36); owned by a TSDFCuda."""

    def __init__(self, tsdf: "TSDFCuda", which: int):
        self._t = tsdf
        self._which = which

    def to_device(self, existing_map: DeviceMap):
        t = self._t
        check(t._L.ws_map_upload(t.handle, self._which, _ptr(_i3(existing_map.size_)), _ptr(_i3(existing_map.pos_)),
                                 _ptr(_i3(existing_map.offset_)), _ptr(existing_map.data_)), "ws_map_upload")

    def update_params(self, existing_map: DeviceMap):
        t = self._t
        check(t._L.ws_map_set_params(t.handle, self._which, _ptr(_i3(existing_map.size_)),
                                     _ptr(_i3(existing_map.pos_)), _ptr(_i3(existing_map.offset_))), "ws_map_set_params")

    def to_host(self, existing_map: DeviceMap):
        t = self._t
        size, pos, off = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
        check(t._L.ws_map_download(t.handle, self._which, _ptr(size), _ptr(pos), _ptr(off), _ptr(existing_map.data_)),
              "ws_map_download")
        existing_map.size_[:] = size
        existing_map.pos_[:] = pos
        existing_map.offset_[:] = off

    def extract_box(self, lo, hi) -> np.ndarray:
        """Voxels of the inclusive world-voxel box [lo, hi] (x major, z fastest) — ws_map_extract_box."""
        t = self._t
        lo, hi = _i3(lo), _i3(hi)
        out = np.empty(int(np.prod((hi - lo + 1).astype(np.int64))), dtype=np.uint32)
        check(t._L.ws_map_extract_box(t.handle, self._which, _ptr(lo), _ptr(hi), _ptr(out)), "ws_map_extract_box")
        return out

    def insert_box(self, lo, hi, data):
        t = self._t
        lo, hi = _i3(lo), _i3(hi)
        data = np.ascontiguousarray(data, dtype=np.uint32)
        assert data.size == int(np.prod((hi - lo + 1).astype(np.int64)))
        check(t._L.ws_map_insert_box(t.handle, self._which, _ptr(lo), _ptr(hi), _ptr(data)), "ws_map_insert_box")

    def surface(self, lo=None, hi=None, band=None, marker=False, device=False):
        """The surface cloud of this map — publish_local_map (include/warpsense/visualization/map.h:14-121) on the device
        (ws_map_surface): every voxel of the inclusive world-voxel box [lo, hi] (both None: the whole window) with
        weight > 0 and abs(value) < band (None: tau), in ascending world (x, y, z), z fastest.

        Returns the records as a numpy array of dtype SURFACE_RECORD (x, y, z in world voxels, raw entry); with `marker`
        a pair (records, (n, 7) float32: x y z in metres, r g b a as the reference computes them).
        device=True: torch tensors on the GPU instead — (n, 4) int32 and (n, 7) float32 — that ALIAS the library's buffers:
        valid until the next surface() on this TSDFCuda, copy them (.clone()) to keep them."""
        return _surface_call(self._t._L, "ws_map_surface", self._t, (self._which,), lo, hi, band, (), marker, device)

    def mesh(self, lo=None, hi=None, any_weight=False, device=False):
        """A triangle mesh of this map by naive surface nets on the device (ws_map_mesh; the rules are stated in
        include/warpsense_hip.h): one vertex per active cell of the inclusive world-voxel box [lo, hi] (both None: the whole
        window), two triangles per crossing lattice edge whose four cells are valid.  any_weight: voxels with a negative weight
        count as observed too (the rule of the registration).

        Returns (vertices, faces): a numpy array of dtype VERT (x_mm, y_mm, z_mm, weight) in ascending cell order and an (n, 3)
        uint32 array of vertex indices, normals towards the outside.
        device=True: torch tensors on the GPU instead -- (n, 4) int32 and (n, 3) int32 -- that ALIAS the library's buffers: valid
        until the next mesh() on this TSDFCuda, copy them (.clone()) to keep them."""
        return _mesh_call(self._t._L, "ws_map_mesh", self._t, (self._which,), lo, hi, (), any_weight, device)

    def raycast(self, origin_mm, dirs, max_range_mm, any_weight=False, gradient=False, targets=False):
        """Ray cast of this map on the device (ws_map_raycast; the rules are stated in include/warpsense_hip.h): per ray the first
        crossing of the surface from the outside within max_range_mm.  origin_mm: three int32 (map frame, millimetres); dirs:
        (n, 3) int32 directions of any length (|component| < 2^30), a numpy array or a device array (a CUDA tensor, DevicePoints);
        targets=True: `dirs` holds map-frame points in mm instead and every ray runs from the origin towards its point.
        any_weight: voxels with a negative weight count as observed too (the rule of the registration).

        Returns (records, gradient): a numpy array of dtype RAY (x_mm, y_mm, z_mm, range_mm; no hit: 0, 0, 0, -1) in ray order
        and, with gradient=True, an (n, 3) int32 array of central differences of the TSDF value at the hit (towards the outside,
        not normalised; zeros where a neighbour is unobserved), else None.  `last_hits` keeps the call's number of hits."""
        rec, grad, self.last_hits = _raycast_call(self._t._L, "ws_map_raycast", self._t.handle, (self._which,), origin_mm, dirs, max_range_mm, (),
                                                  any_weight, gradient, targets)
        return rec, grad

    def sample(self, points, band_mm=None, any_weight=False, gradient=False, select=None, device=False):
        """What this map says at `points` (ws_map_sample; the rules are stated in include/warpsense_hip.h): (n, 3) int32 map-frame
        points in millimetres, a numpy array or a device array (a CUDA tensor, DevicePoints).  band_mm: the half-width of the SURFACE
        class (None: the map's tau).  any_weight: voxels with a negative weight count as observed too (the rule of the registration).
        select: class names out of SAMPLE_CLASSES ("unknown", "free", "surface", "inside"); the input points of those classes come
        back in input order.

        Returns (records, counts, gradient, selection): a numpy array of dtype SAMPLE (d_mm, weight, cls, raw) in input order; the
        number of points per class (uint64 [4]); with gradient=True an (n, 3) int32 array of central differences of the TSDF value
        at the nearest voxel (zeros where a neighbour is unobserved), else None; with `select` the (k, 3) int32 selected points, else
        None.  device=True: records and gradient are torch tensors on the GPU ((n, 4) / (n, 3) int32) and the selection is a
        DevicePoints that update_tsdf and prepare_registration accept; all three ALIAS the library's buffers and are valid until the
        next sample() on this TSDFCuda."""
        return _sample_call(self._t._L, "ws_map_sample", self._t, (self._which,), points, 0 if band_mm is None else band_mm, (), any_weight, gradient, select,
                            device)

    def distance(self, lo=None, hi=None, max_dist_vox=20, unknown_occupied=False, columns=False, any_weight=False, device=False):
        """The distance field of this map on the device (ws_map_distance; the rules are stated in include/warpsense_hip.h): per
        voxel of the inclusive world-voxel box [lo, hi] (both None: the whole window) the squared Euclidean distance in voxels to
        the nearest occupied voxel of the box (valid and value < 0; unknown_occupied: or never observed), clamped at
        max_dist_vox squared (1 .. 255).  columns: the 2-D field over the (x, y) columns of the box.  any_weight: voxels with a
        negative weight count as observed too (the rule of the registration).

        Returns the records as a uint32 array shaped (nx, ny, nz), or (nx, ny) with columns: bits 0..23 the squared distance,
        bits 30..31 the class (distance_d2, distance_class, distance_mm take them apart).  `last_sites` keeps the call's number
        of site voxels / columns.
        device=True: a torch int32 tensor of that shape on the GPU instead that ALIASES the library's buffer: valid until the next
        distance() on this TSDFCuda, copy it (.clone()) to keep it."""
        def window_shape():
            size = np.zeros(3, np.int32)
            check(self._t._L.ws_map_get_params(self._t.handle, self._which, _ptr(size), None, None), "ws_map_get_params")
            return tuple(int(v) for v in size)
        rec, self.last_sites = _distance_call(self._t._L, "ws_map_distance", self._t, (self._which,), lo, hi, max_dist_vox, unknown_occupied, columns,
                                              any_weight, device, window_shape)
        return rec

    def ground(self, lo=None, hi=None, clear_vox=20, any_weight=False, unknown_headroom=False, top=False, device=False):
        """The ground layer of this map on the device (ws_map_ground; the rules are stated in include/warpsense_hip.h): per (x, y)
        column of the inclusive world-voxel box [lo, hi] (both None: the whole window) the lowest (top: the highest) occupied voxel
        with a free voxel right above it and clear_vox (1 .. 64) free voxels of headroom (unknown_headroom: unknown ones count above
        the first), its sub-voxel height and the largest height step to the neighbouring ground columns.  any_weight: voxels with a
        negative weight count as observed too.  Returns a GroundResult (records shaped (nx, ny), lo, ext, counts per class).
        device=True: its records are a torch int32 tensor (nx, ny, 2) that ALIASES the library's buffer, valid until the next ground()
        on this TSDFCuda."""
        return _ground_call(self._t._L, "ws_map_ground", self._t, (self._which,), lo, hi, clear_vox, any_weight, unknown_headroom, top, device)

    def ground_distance(self, max_step_q8, max_dist_vox=20, unknown_occupied=False, device=False):
        """The column distance field over the LAST ground() result of this TSDFCuda (ws_map_ground_distance): a column is free iff it
        is ground and its step is at most max_step_q8 (1/256 voxel); blocked, void and steeper columns are sites, unknown ones with
        unknown_occupied.  It REPLACES the result of distance(): reach() then plans over it as over distance(columns=True).  Returns
        the uint32 records shaped (nx, ny); `last_sites` keeps the number of site columns."""
        rec, self.last_sites = _ground_distance_call(self._t._L, "ws_map_ground_distance", self._t, max_step_q8, max_dist_vox, unknown_occupied, device)
        return rec

    def ground_timing(self, enable: int = -1):
        """device milliseconds of pass 1 (levels) and pass 2 (steps) of the last ground() (ws_debug_ground_timing)"""
        return _timing(self._t._L, "ws_debug_ground_timing", self._t.handle, 2, enable)

    def frontier(self, lo=None, hi=None, min_value=0, any_weight=False, clusters=False, device=False):
        """The frontier of this map on the device (ws_map_frontier; the rules are stated in include/warpsense_hip.h): the voxels of
        the inclusive world-voxel box [lo, hi] (both None: the whole window) that are observed free (weight > 0, value >=
        min_value) and touch a never-observed voxel of the box, in ascending world (x, y, z), z fastest.  min_value: 0 for any
        non-negative value, the map's tau to stay a truncation distance away from surfaces.  any_weight: voxels with a negative
        weight count as observed too.  clusters: also the 26-connected patches of the records.

        Returns the records as a numpy array of dtype FRONTIER_RECORD (x, y, z in world voxels, mask of unknown neighbours); with
        `clusters` a triple (records, labels, table): one uint32 cluster number per record and the table of dtype FRONTIER_CLUSTER
        (first, count, lo, hi, sum), clusters numbered by their first record; frontier_goals(table, resolution) turns it into goals.
        device=True: torch int32 tensors on the GPU instead -- (n, 4), (n,) and (k, 16) -- that ALIAS the library's buffers: valid
        until the next frontier() on this TSDFCuda, copy them (.clone()) to keep them."""
        return _frontier_call(self._t._L, "ws_map_frontier", self._t, (self._which,), lo, hi, min_value, any_weight, clusters, device)

    def frontier_timing(self, enable: int = -1):
        """device milliseconds of the count pass, the scan, the emit pass and the clustering of the last frontier() (ws_debug_frontier_timing)"""
        return _timing(self._t._L, "ws_debug_frontier_timing", self._t.handle, 4, enable)

    def reach(self, seeds, clear_d2=0, unknown_free=False, max_rounds=0, device=False):
        """The geodesic field over the LAST distance() result of this TSDFCuda (either map's wrapper reaches it) (ws_map_reach; the rules are stated in
        include/warpsense_hip.h): per record the cost of the cheapest 26-connected (columns: 8-connected) path from `seeds` ((n, 3)
        int32 world voxels) over records that are free (unknown_free: or unknown) with d2 >= clear_d2; a face step weighs 10, an edge
        step 14, a corner step 17, unreachable is 0xFFFFFFFF (reach_mm turns costs into millimetres).  max_rounds: 0 for the default
        cap.  Returns the uint32 costs shaped like that distance result; `last_reach` keeps dict(seeded, reached, rounds).
        device=True: a torch int32 tensor on the GPU that ALIASES the library's buffer, valid until the next reach()."""
        cost, self.last_reach = _reach_call(self._t._L, "ws_map_reach", self._t, seeds, clear_d2, unknown_free, max_rounds, device)
        return cost

    def reach_lookup(self, points):
        """The costs of the last reach() at world voxels: an (n, 3) or (n, 4) int32 numpy array gives a uint32 numpy array; a CUDA
        tensor of such rows -- the records of frontier(device=True) -- gives an int32 CUDA tensor of the same bits.  Outside the box
        of the reach result: 0xFFFFFFFF."""
        return _reach_lookup_call(self._t._L, "ws_map_reach_lookup", self._t, points)

    def reach_paths(self, goals, cap_steps=0):
        """The paths of the last reach() from `goals` ((g, 3) int32 world voxels) back to a seed.  Returns (headers, records) of dtypes
        REACH_PATH_HEADER [g] (cost, steps, written, status: 0 reached, 1 not reachable, 2 outside) and REACH_PATH_RECORD
        [g, cap_steps] (x, y, z, cost; goal first); cap_steps = 0 asks for the headers alone."""
        return _reach_paths_call(self._t._L, "ws_map_reach_paths", self._t, goals, cap_steps)

    def reach_timing(self, enable: int = -1):
        """device milliseconds of the seeding, of all rounds as one span and of the count pass of the last reach() (ws_debug_reach_timing)"""
        return _timing(self._t._L, "ws_debug_reach_timing", self._t.handle, 3, enable)

    def view_gain(self, origins_mm, dirs, max_range_mm, lo=None, hi=None, min_value=0, any_weight=False, rays=False, device=False):
        """What the sensor would see from candidate poses (ws_map_view_gain; the rules are stated in include/warpsense_hip.h): for each
        of the (m, 3) int32 map-frame origins in millimetres and the one fan of (n, 3) int32 directions (view_fan makes one) the
        UNKNOWN and FREE samples its rays meet inside the inclusive world-voxel box [lo, hi] (both None: the whole window) before an
        occupied voxel (valid, value < min_value) blocks them, as counts and weighted by k^2.  any_weight: voxels with a negative
        weight count as observed too.

        Returns the records as a numpy array of dtype VIEW_GAIN_RECORD, one per origin; with `rays` a pair (records, (m, n) array of
        VIEW_GAIN_RAY).  `last_view_gain` keeps dict(best_unknown_k2, views, rays).  gain_volume_m3 and rank_views read the records.
        device=True: torch int32 tensors on the GPU instead -- (m, 8) and (m, n, 2) -- that ALIAS the library's buffers: valid until
        the next view_gain() on this TSDFCuda, copy them (.clone()) to keep them."""
        rec, ray, best = _view_gain_call(self._t._L, "ws_map_view_gain", self._t, (self._which,), lo, hi, origins_mm, dirs, max_range_mm, (), min_value,
                                         any_weight, rays, device)
        self.last_view_gain = dict(best_unknown_k2=best, views=int(rec.shape[0]), rays=int(np.asarray(dirs).reshape(-1, 3).shape[0]))
        return (rec, ray) if rays else rec

    def view_gain_timing(self, enable: int = -1):
        """device milliseconds of the upload, of the fan preparation with the march, and of the maximum pass of the last view_gain()
        (ws_debug_view_gain_timing)"""
        return _timing(self._t._L, "ws_debug_view_gain_timing", self._t.handle, 3, enable)

    def clearance(self, poses, body, soft_mm=0, per_pose=False, outside_ok=False, device=False):
        """Candidate trajectories against the LAST distance() or ground_distance() result of this TSDFCuda (ws_map_clearance; the rules
        are stated in include/warpsense_hip.h): poses (T, P, 12) int32 (trajectory_poses; a CUDA tensor takes the _dev form), body
        (k, 4) int32 (body_spheres), soft_mm the range of the soft cost.  per_pose: also one record per pose.  outside_ok: samples
        outside the box of the distance result do not disqualify a trajectory from `best`.  Returns a ClearanceResult; device=True:
        its arrays are torch tensors that ALIAS the library's buffers, valid until the next clearance() on this TSDFCuda."""
        return _clearance_call(self._t._L, "ws_map_clearance", self._t, poses, body, soft_mm, (), per_pose, outside_ok, device)

    def clearance_timing(self, enable: int = -1):
        """device milliseconds of the upload, of the trajectory pass and of the pass that finds the best of the last clearance()
        (ws_debug_clearance_timing)"""
        return _timing(self._t._L, "ws_debug_clearance_timing", self._t.handle, 3, enable)

    def dev(self):
        return self._t.handle

    def device_ptr(self) -> int:
        return int(self._t._L.ws_map_device_data(self._t.handle, self._which) or 0)


class TSDFCuda:
    """cuda::TSDFCuda (update_tsdf.h:9-34, update_tsdf.cu:130-221)."""

    n_max_points_ = 1_000_000

    def __init__(self, existing_map: DeviceMap, tau: int, max_weight: int, map_resolution: int, ctx: Context | None = None):
        self.ctx = ctx or Context.default()
        self._L = self.ctx._L
        self.tau_, self.max_weight_, self.map_resolution_ = int(tau), int(max_weight), int(map_resolution)
        self.n_voxels_ = existing_map.n_voxels()
        h = C.c_void_p()
        check(self._L.ws_map_create(self.ctx.handle, _ptr(_i3(existing_map.size_)), _ptr(_i3(existing_map.pos_)),
                                    _ptr(_i3(existing_map.offset_)), _ptr(existing_map.data_), self.tau_, self.max_weight_,
                                    self.map_resolution_, C.byref(h)), "ws_map_create")
        self.handle = h
        self._avg = DeviceMapMemWrapper(self, WS_MAP_AVG)
        self._new = DeviceMapMemWrapper(self, WS_MAP_NEW)
        self._scan_in_flight = None  # the device tensor of the last update (kept until the next one is enqueued behind it)

    # -- the three update_tsdf overloads of the reference (update_tsdf.cu:143-191)
    def update_tsdf(self, scan_points, scanner_pos, up, result: DeviceMap | None = None, latest_map: DeviceMap | None = None):
        n = int(scan_points.shape[0])
        sp, u = _i3c(scanner_pos), _i3c(up)
        if _is_device(scan_points):
            # ws_tsdf_update_dev returns after its launches: the tensor must not go back to torch's allocator before the kernels have
            # read it (torch's allocator only knows torch's streams) -- keep it until the next update has been enqueued behind it
            prev = self._scan_in_flight
            rc = self._L.ws_tsdf_update_dev(self.handle, _ptr(scan_points), n, _ptr(sp), _ptr(u))
            self._scan_in_flight = scan_points
            del prev
        else:
            pts = np.ascontiguousarray(scan_points, dtype=np.int32)
            rc = self._L.ws_tsdf_update(self.handle, _ptr(pts), n, _ptr(sp), _ptr(u))
        if rc == -3:
            # update_tsdf.cu:146-150: message on stderr, no work, no exception
            import sys
            print("HIP Error: " + self._L.ws_last_error().decode(), file=sys.stderr)
            return
        check(rc, "ws_tsdf_update")
        if result is not None:
            self._avg.to_host(result)
        if latest_map is not None:
            self._new.to_host(latest_map)

    def scatter(self, scan_points_dev, scanner_pos, up):
        """cu_min_tsdf_krnl alone (parity tests): leaves the resolved scan in new_map."""
        prev = self._scan_in_flight  # (see update_tsdf)
        check(self._L.ws_tsdf_scatter_dev(self.handle, _ptr(scan_points_dev), int(scan_points_dev.shape[0]),
                                          _ptr(_i3c(scanner_pos)), _ptr(_i3c(up))), "ws_tsdf_scatter_dev")
        self._scan_in_flight = scan_points_dev
        del prev

    def integrate(self):
        check(self._L.ws_tsdf_integrate(self.handle), "ws_tsdf_integrate")

    def set_integrate(self, mode: int):
        check(self._L.ws_tsdf_set_integrate(self.handle, int(mode)), "ws_tsdf_set_integrate")

    def set_capacity(self, records: int):
        check(self._L.ws_tsdf_set_capacity(self.handle, int(records)), "ws_tsdf_set_capacity")

    def debug_chunk_policy(self, budget_bytes: int, est_shift: int):
        """test entry: size the chunk buffer by estimate (see ws_debug_tsdf_chunk_policy)"""
        check(self._L.ws_debug_tsdf_chunk_policy(self.handle, int(budget_bytes), int(est_shift)), "ws_debug_tsdf_chunk_policy")

    def stats(self, raise_on_error: bool = False) -> dict:
        st = _lib.TsdfStats()
        rc = self._L.ws_tsdf_stats(self.handle, C.byref(st))
        out = {"contested_voxels": st.contested_voxels, "records": st.records, "tiles": st.tiles, "error_flags": st.error_flags,
               "runs": st.runs, "free_space_hits": st.free_space_hits, "record_slots": st.record_slots,
               "record_capacity": st.record_capacity, "hash_entries": st.hash_entries, "status": rc}
        if rc != 0 and raise_on_error:
            check(rc, "ws_tsdf_stats")
        return out

    def device_map(self):
        return self.handle

    def avg_map(self) -> DeviceMapMemWrapper:
        return self._avg

    def new_map(self) -> DeviceMapMemWrapper:
        return self._new

    def close(self):
        if self.handle:
            self._L.ws_map_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
