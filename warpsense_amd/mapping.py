"""The application classes: the parameters, TSDFMapping (update, queries, map shift, write-back) and TSDFRegistration."""
from __future__ import annotations

import contextlib
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._abi import WEIGHT_RESOLUTION, _i3, _is_device, _ptr
from ._lib import SAMPLE_CLASSES, WS_REG_ALL_POINTS, WsError, check
from .clearance import ClearanceQueries
from .context import Context
from .device_map import DeviceMap, LocalMap, TSDFCuda
from .global_map import GlobalMap
from .merge import FuseQueries
from .pyramid import PyramidQueries
from .gain import GainQueries
from .ground import GroundQueries
from .registration import RegistrationCuda, batch_best, candidate_poses
from .scan import to_int_mat, to_map
from .store import DeviceGlobalMap


class MapParams:
    """The hot-path knobs of params/params.yaml with the scaling rules of include/params/map_params.h:100-114."""

    def __init__(self, resolution=64, max_distance=1.0, max_weight=10, size=(40.0, 40.0, 25.0), shift=10.0, initial_weight=0):
        self.resolution = int(resolution)
        self.max_distance = float(max_distance)
        self.tau = int(max_distance * 1000)
        self.max_weight = int(max_weight * WEIGHT_RESOLUTION)
        self.size = tuple(int(s * 1000 / self.resolution) for s in size)
        self.shift = float(shift)
        self.initial_weight = int(initial_weight)

    def size_voxels(self):
        return self.size


class RegistrationParams:
    def __init__(self, max_iterations=200, it_weight_gradient=0.1, epsilon=0.03):
        self.max_iterations = int(max_iterations)
        self.it_weight_gradient = float(it_weight_gradient)
        self.epsilon = float(epsilon)


class Params:
    def __init__(self, map_params: MapParams | None = None, registration: RegistrationParams | None = None):
        self.map = map_params or MapParams()
        self.registration = registration or RegistrationParams()


def _points_to_host(points):
    """points as they lie (numpy, a CUDA tensor, DevicePoints), on the host"""
    if _is_device(points):
        return points.to_host() if hasattr(points, "to_host") else points.cpu().numpy()
    return points


def _range_residual(rec, points_mm, origin):
    """per ray cast record towards a point: the range the map shows minus the point's own distance from the origin (float64 mm; NaN: no hit)"""
    d = np.asarray(_points_to_host(points_mm), dtype=np.float64).reshape(-1, 3) - origin.astype(np.float64)
    return np.where(rec["range_mm"] >= 0, rec["range_mm"].astype(np.float64) - np.sqrt(np.sum(d * d, axis=1)), np.nan)


def _dirs_or_os1(dirs):
    """dirs, or for None the 128 x 1024 table of the OS1-128 pattern"""
    if dirs is None:
        from .synthetic import os1_128_dirs
        dirs = os1_128_dirs()
    return dirs


class TSDFMapping(GroundQueries, GainQueries, ClearanceQueries, FuseQueries, PyramidQueries):
    """cuda::TSDFMapping without ROS (the protected constructor path, tsdf_mapping.cpp:30-41)."""

    def __init__(self, params: Params, local_map: LocalMap, ctx: Context | None = None, device_global_map: "DeviceGlobalMap | None" = None):
        self.params_ = params
        self.local_map_ = local_map
        self.cuda_map_ = local_map.device_map()
        self.tsdf_ = TSDFCuda(self.cuda_map_, params.map.tau, params.map.max_weight, params.map.resolution, ctx)
        self.mutex_ = threading.RLock()  # the reference's shared_mutex: one writer or many readers
        # the global map in device memory: shift_map_device and write_back go through it (shift_map / shift_map_async do not)
        self.device_global_map_ = device_global_map

    def convert_pose_to_gpu(self, pose):
        """tsdf_mapping.cpp:77-85: pos = floor(t/res) voxels, up = (R_int * (0,0,MR)) / MR."""
        # (R_int * (0, 0, MR) + 0) / MR == third column of R_int exactly (|R_int| <= 32768, no int overflow)
        up = to_int_mat(pose)[:3, 2].astype(np.int32)
        return to_map(pose, self.params_.map.resolution), up

    def update_tsdf(self, scan_points, pose=None, pos_rm=None, up_rm=None, result: DeviceMap | None = None):
        if pose is not None:
            pos_rm, up_rm = self.convert_pose_to_gpu(pose)
        with self.mutex_:
            self.tsdf_.update_tsdf(scan_points, pos_rm, up_rm, result=result)

    def tsdf(self) -> TSDFCuda:
        return self.tsdf_

    def surface_cloud(self, **kw):
        """publish_local_map's cloud of the averaged map (visualization/map.h:14-121; the reference publishes it after every
        update, src/cpu/fastsense.cpp:115): DeviceMapMemWrapper.surface on avg_map(), under the mapping's lock like a reader."""
        with self.mutex_:
            return self.tsdf_.avg_map().surface(**kw)

    def surface_mesh(self, **kw):
        """A triangle mesh of the averaged map (DeviceMapMemWrapper.mesh on avg_map()), under the mapping's lock like a reader."""
        with self.mutex_:
            return self.tsdf_.avg_map().mesh(**kw)

    def distance_field(self, lo=None, hi=None, max_dist_m=1.0, unknown_occupied=False, columns=False, any_weight=False):
        """The distance field of the averaged map (DeviceMapMemWrapper.distance on avg_map()), under the mapping's lock like a
        reader: how far every voxel of the box (None: the window) is from the nearest obstacle, up to max_dist_m metres
        (rounded to whole millimetres, then ceil(mm / resolution) voxels, 1 .. 255).  columns: the 2-D cost map of a ground robot whose height band is the box's
        z range.  Returns the uint32 records shaped (nx, ny, nz) or (nx, ny); distance_mm(rec, resolution) gives millimetres."""
        vox = self._max_dist_vox(max_dist_m)
        with self.mutex_:
            return self.tsdf_.avg_map().distance(lo=lo, hi=hi, max_dist_vox=vox, unknown_occupied=unknown_occupied, columns=columns,
                                                 any_weight=any_weight)

    def _max_dist_vox(self, max_dist_m):
        """metres to voxels by the rule of distance_field: the nearest millimetre, then ceil(mm / resolution)"""
        mm = int(np.rint(float(max_dist_m) * 1000.0))
        return -(-mm // int(self.params_.map.resolution))

    @contextlib.contextmanager
    def _window_in_store(self, name):
        """What the global_* queries begin with: behind wait_shift and under the mapping's lock like a writer, the window goes into
        the chunks of device_global_map (ws_store_save_box); the body queries the store it is given under the same lock.  A mapping
        without a store refuses in the name of the query, before it waits."""
        if self.device_global_map_ is None:
            raise WsError(f"{name}: this TSDFMapping has no device_global_map")
        self.wait_shift()
        with self.mutex_:
            lo, hi = self.local_map_.window()
            self.device_global_map_.save_box(self.tsdf_, lo, hi)
            yield self.device_global_map_

    def global_mesh(self, level=0, **kw):
        """The mesh of everything the run has seen: the window goes into the chunks of device_global_map (ws_store_save_box, the
        first step of write_back, with its capacity refusals), then DeviceGlobalMap.mesh at the map's resolution -- under the
        mapping's lock like a writer, nothing leaves the device but the mesh.  Keywords: lo, hi, any_weight, device.
        level > 0: the mesh of that level of global_pyramid at its resolution (PyramidQueries._level_mesh)."""
        if level:
            return self._level_mesh(int(level), **kw)
        with self._window_in_store("global_mesh") as store:
            return store.mesh(int(self.params_.map.resolution), **kw)

    def global_surface_cloud(self, **kw):
        """The surface cloud of everything the run has seen, including what the window has left: the window goes into the chunks of
        device_global_map exactly as in global_mesh (ws_store_save_box behind wait_shift, under the mapping's lock like a writer),
        then DeviceGlobalMap.surface with the map's tau and resolution.  Keywords: lo, hi, band, marker, device."""
        with self._window_in_store("global_surface_cloud") as store:
            return store.surface(self.tsdf_.tau_, int(self.params_.map.resolution), **kw)

    def global_distance_field(self, lo=None, hi=None, max_dist_m=1.0, unknown_occupied=False, columns=False, any_weight=False, device=False):
        """The distance field of everything the run has seen: the window goes into the chunks of device_global_map exactly as in
        global_mesh (ws_store_save_box behind wait_shift, under the mapping's lock like a writer), then DeviceGlobalMap.distance.
        The box (None: the bounding box of the chunks) need not lie in the window; max_dist_m becomes voxels by the rule of
        distance_field (nearest millimetre, then ceil(mm / resolution), 1 .. 255).  The result is dense: 8 bytes of device memory
        per record of the box."""
        if self.device_global_map_ is None:  # (refused before max_dist_m is looked at, which is before _window_in_store waits)
            raise WsError("global_distance_field: this TSDFMapping has no device_global_map")
        vox = self._max_dist_vox(max_dist_m)
        with self._window_in_store("global_distance_field") as store:
            return store.distance(lo=lo, hi=hi, max_dist_vox=vox, unknown_occupied=unknown_occupied, columns=columns, any_weight=any_weight,
                                  device=device)

    def frontier(self, **kw):
        """The frontier of the averaged map (DeviceMapMemWrapper.frontier on avg_map()), under the mapping's lock like a reader: where
        the window's known free space ends.  Keywords: lo, hi, min_value, any_weight, clusters, device."""
        with self.mutex_:
            return self.tsdf_.avg_map().frontier(**kw)

    def global_frontier(self, lo=None, hi=None, **kw):
        """The frontier of everything the run has seen: the window goes into the chunks of device_global_map exactly as in global_mesh
        (ws_store_save_box behind wait_shift, under the mapping's lock like a writer), then DeviceGlobalMap.frontier.  The default box
        is the bounding box of the chunks GROWN BY ONE VOXEL on every side (cut to int32), so that the outer faces of the mapped volume are frontier
        too.  Keywords: min_value, any_weight, clusters, device."""
        with self._window_in_store("global_frontier") as store:
            if lo is None and hi is None:
                keys = np.asarray(store.keys(), dtype=np.int64).reshape(-1, 3)
                if len(keys):
                    lo = np.maximum(keys.min(axis=0) * store.CHUNK_SIZE - 1, -2 ** 31)  # (cut to int32 voxel space)
                    hi = np.minimum((keys.max(axis=0) + 1) * store.CHUNK_SIZE, 2 ** 31 - 1)
            return store.frontier(lo=lo, hi=hi, **kw)

    @staticmethod
    def raycast_rays(pose, dirs):
        """The integers of a ray cast from a pose, in float64 numpy: origin = the pose's translation in metres times 1000, rounded
        to nearest (ties to even); every direction (unit-free, sensor frame) is rotated by the pose's 3 x 3 block and scaled so
        that its longest component is 2^20 in magnitude, then rounded to nearest; a zero direction stays zero (a no-hit).
        Returns (origin_mm (3,) int32, dirs (n, 3) int32)."""
        pose = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        origin = np.rint(pose[:3, 3] * 1000.0).astype(np.int32)
        d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3) @ pose[:3, :3].T
        longest = np.max(np.abs(d), axis=1)
        d = d * (float(1 << 20) / np.where(longest > 0, longest, 1.0))[:, None]
        return origin, np.rint(d).astype(np.int32)

    def _diagonal_mm(self):
        size = np.asarray(self.local_map_.size, dtype=np.float64) * float(self.params_.map.resolution)
        return int(np.ceil(np.sqrt(np.sum(size * size))))

    def raycast(self, pose, dirs=None, max_range_mm=None, **kw):
        """The predicted scan of the averaged map from `pose` (4 x 4, metres): DeviceMapMemWrapper.raycast on avg_map(), under the
        mapping's lock like a reader.  dirs: (n, 3) float directions in the sensor frame (None: the 128 x 1024 table of the
        OS1-128 pattern, synthetic.os1_128_dirs); they and the pose become integers by the rule of raycast_rays.
        max_range_mm None: the window's diagonal.  Returns (records, gradient | None)."""
        origin, d = self.raycast_rays(pose, _dirs_or_os1(dirs))
        with self.mutex_:
            return self.tsdf_.avg_map().raycast(origin, d, self._diagonal_mm() if max_range_mm is None else max_range_mm, **kw)

    def scan_residual(self, points_mm, pose, **kw):
        """Per point of a scan in the map frame (n x 3 int32 millimetres, numpy or on the device as it lies: a CUDA tensor,
        DevicePoints) the range the averaged map shows along the ray from the pose's origin (raycast_rays) towards the point,
        minus the point's own distance |point - origin|, in millimetres (float64; NaN where the ray does not hit within the
        window's diagonal).  The median of its absolute value is the quality figure of a registration."""
        origin = self.raycast_rays(pose, np.zeros((0, 3)))[0]
        with self.mutex_:
            rec, _ = self.tsdf_.avg_map().raycast(origin, points_mm, self._diagonal_mm(), targets=True, **kw)
        return _range_residual(rec, points_mm, origin)

    def sample(self, points_mm, **kw):
        """DeviceMapMemWrapper.sample on avg_map() at map-frame points (n x 3 int32 millimetres, numpy or on the device), under the
        mapping's lock like a reader.  Returns (records, counts, gradient | None, selection | None)."""
        with self.mutex_:
            return self.tsdf_.avg_map().sample(points_mm, **kw)

    def global_sample(self, points_mm, band_mm=None, **kw):
        """sample against the chunks of device_global_map: the window goes into the chunks as in global_raycast, then
        DeviceGlobalMap.sample at the map's resolution.  band_mm None: the map's tau.  Keywords: lo, hi, any_weight, gradient, select,
        device."""
        with self._window_in_store("global_sample") as store:
            return store.sample(int(self.params_.map.resolution), points_mm, int(self.params_.map.tau) if band_mm is None else band_mm, **kw)

    def scan_consistency(self, points_mm, pose=None, band_mm=None):
        """How a scan agrees with the averaged map, in one pass over its points: points_mm are the scan in the map frame (n x 3 int32
        millimetres, numpy or on the device); with `pose` (4 x 4, translation in mm) they are in the sensor frame and are moved by it
        first (on the host, rounded to nearest).  Returns a dict: the fractions "unknown", "free", "surface", "inside" of the points
        per class of sample() at band_mm (None: tau), and "mean_abs_d_mm", the mean |d_mm| over the SURFACE class (NaN without
        one)."""
        if pose is not None:
            P = np.asarray(pose, dtype=np.float64).reshape(4, 4)
            points_mm = np.rint(np.asarray(_points_to_host(points_mm), dtype=np.float64).reshape(-1, 3) @ P[:3, :3].T + P[:3, 3]).astype(np.int32)
        rec, counts, _, _ = self.sample(points_mm, band_mm=band_mm)
        n = max(int(counts.sum()), 1)
        out = {name: float(counts[c]) / n for c, name in enumerate(SAMPLE_CLASSES)}
        surf = rec["cls"] == 2
        out["mean_abs_d_mm"] = float(np.mean(np.abs(rec["d_mm"][surf].astype(np.float64)))) if surf.any() else float("nan")
        return out

    def _global_range_mm(self, origin):
        """the diagonal of the bounding box of the present chunks in mm, capped so that |origin| + range + 2 res fits int32"""
        res = int(self.params_.map.resolution)
        keys = np.asarray(self.device_global_map_.keys(), dtype=np.float64).reshape(-1, 3)
        ext = (keys.max(axis=0) - keys.min(axis=0) + 1.0) * 64.0 * res if len(keys) else np.ones(3)
        cap = 2 ** 31 - 1 - 2 * res - int(np.max(np.abs(np.asarray(origin, dtype=np.int64))))
        return int(max(1, min(cap, np.ceil(np.sqrt(np.sum(ext * ext))))))

    def global_raycast(self, pose, dirs=None, max_range_mm=None, **kw):
        """The predicted scan from `pose` through everything the run has seen, not only the window: the window goes into the
        chunks of device_global_map exactly as in global_mesh (ws_store_save_box behind wait_shift, under the mapping's lock like a
        writer), then DeviceGlobalMap.raycast at the map's resolution with the integers of raycast_rays.  dirs None: the OS1-128
        table; max_range_mm None: the diagonal of the bounding box of the present chunks (capped to what the range check admits).
        Keywords: lo, hi, any_weight, gradient, targets.  Returns (records, gradient | None)."""
        if self.device_global_map_ is None:  # (refused before the rays are made, which is before _window_in_store waits)
            raise WsError("global_raycast: this TSDFMapping has no device_global_map")
        if kw.get("targets"):
            origin, d = self.raycast_rays(pose, np.zeros((0, 3)))[0], dirs
        else:
            origin, d = self.raycast_rays(pose, _dirs_or_os1(dirs))
        with self._window_in_store("global_raycast") as store:
            rng = self._global_range_mm(origin) if max_range_mm is None else max_range_mm
            return store.raycast(int(self.params_.map.resolution), origin, d, rng, **kw)

    def global_scan_residual(self, points_mm, pose, **kw):
        """scan_residual against the chunks of device_global_map (global_raycast with the points as targets): the pose may lie
        anywhere the run has been.  NaN where the ray does not hit within the diagonal of the present chunks' bounding box."""
        rec, _ = self.global_raycast(pose, points_mm, targets=True, **kw)
        return _range_residual(rec, points_mm, self.raycast_rays(pose, np.zeros((0, 3)))[0])

    def shift_map(self, new_pos):
        """TSDFMapping::map_shift (tsdf_mapping.cpp:109-126) with the window moved ON THE DEVICE: per axis, the slab
        that leaves is packed and saved to the global map, pos/offset move, the slab that enters is loaded and
        unpacked (the three steps of HDF5LocalMap::shift, hdf5_local_map.cpp:53-118).  The reference copies the whole
        map device -> host -> device instead.  The host LocalMap only follows pos/offset; its voxel array is stale
        until avg_map().to_host() is called."""
        self.wait_shift()
        lm, avg, new = self.local_map_, self.tsdf_.avg_map(), self.tsdf_.new_map()
        with self.mutex_:
            plan = _lib.ShiftPlan()  # per axis that moves: the boxes that leave and enter
            check(self.tsdf_._L.ws_shift_plan(_ptr(_i3(lm.size)), _ptr(_i3(lm.pos)), _ptr(_i3(lm.offset)), _ptr(_i3(new_pos)), C.byref(plan)),
                  "ws_shift_plan")
            for i in range(plan.n):
                lo, hi = np.array(plan.leave_lo[i], dtype=np.int64), np.array(plan.leave_hi[i], dtype=np.int64)
                lm.map_.save_box(lo, hi, avg.extract_box(lo, hi))
                step = lm.pos.copy()
                step[plan.axis[i]] += plan.d[i]
                lm.follow(step)
                view = lm.device_map()
                avg.update_params(view)
                new.update_params(view)  # new_map is (tau, 0) everywhere: only its window moves
                lo, hi = np.array(plan.enter_lo[i], dtype=np.int64), np.array(plan.enter_hi[i], dtype=np.int64)
                avg.insert_box(lo, hi, lm.map_.load_box(lo, hi))

    # ---- the same shift off the scan path ---------------------------------------------------------------
    def shift_map_async(self, new_pos):
        """TSDFMapping::map_shift as the reference runs it — on its own thread, the scans only wait for the swap
        (tsdf_mapping.cpp:97-136).  On the scan path: ws_shift_begin (device kernels: pack the leaving slabs into a staging
        buffer, move the window, fill the entering slabs with the default entry — stream-ordered, no waiting) and, only for
        revisited space, the upload of the chunks the global map already holds for the entering slabs.  The leaving slabs
        travel to the host on a second stream and a worker thread files them into the global map.  Same result as
        shift_map(); wait_shift() joins the worker (write_back() and the next shift do that themselves)."""
        self.wait_shift()  # one shift in flight; its slabs must be in the global map before entering data is looked up
        lm, avg = self.local_map_, self.tsdf_.avg_map()
        new_pos = _i3(new_pos)
        L = self.tsdf_._L
        ticket = C.c_void_p()
        n = 0
        self._shift_error = None

        def file_slabs():
            # the ticket is closed whatever happens, and a failure travels to wait_shift() (a daemon thread's traceback
            # would be the only trace of slabs that never reached the global map)
            try:
                file_slabs_body()
            except BaseException as exc:  # noqa: BLE001 - re-raised by wait_shift()
                self._shift_error = exc
            finally:
                L.ws_shift_end(ticket)

        def file_slabs_body():
            check(L.ws_shift_wait(ticket), "ws_shift_wait")
            slo, shi = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
            elo, ehi = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
            for i in range(n):
                data = C.c_void_p()
                check(L.ws_shift_slab(ticket, i, _ptr(slo), _ptr(shi), C.byref(data)), "ws_shift_slab")
                ext = shi.astype(np.int64) - slo + 1
                buf = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint32)), shape=(int(np.prod(ext)),))
                box = buf.reshape(int(ext[0]), int(ext[1]), int(ext[2]))
                # A corner that ENTERED with an earlier axis of this shift and leaves again with this one was packed as
                # default fill; the synchronous route would have loaded it from the global map and saved it back
                # unchanged.  Put the global map's own data there, so the save below changes nothing for it.
                for j in range(i):
                    check(L.ws_shift_entering(ticket, j, _ptr(elo), _ptr(ehi)), "ws_shift_entering")
                    a, b = np.maximum(slo, elo).astype(np.int64), np.minimum(shi, ehi).astype(np.int64)
                    if np.all(a <= b):
                        e = b - a + 1
                        sl = tuple(slice(int(a[k] - slo[k]), int(b[k] - slo[k]) + 1) for k in range(3))
                        box[sl] = lm.map_.load_box(a, b).reshape(int(e[0]), int(e[1]), int(e[2]))
                lm.map_.save_box(slo.copy(), shi.copy(), buf)

        with self.mutex_:
            check(L.ws_shift_begin(self.tsdf_.handle, _ptr(new_pos), int(lm.map_.default_raw), C.byref(ticket)), "ws_shift_begin")
            n = L.ws_shift_count(ticket)
            try:
                self._shift_enter(L, ticket, n, new_pos, lm, avg)
            except BaseException:
                # the window has moved on the device: the leaving slabs are still filed and the ticket is closed (an open
                # ticket makes every later ws_shift_begin fail); the failure itself goes to the caller
                file_slabs()
                raise
        self._shift_worker = threading.Thread(target=file_slabs, name="warpsense-map-shift", daemon=True)
        self._shift_worker.start()

    def _shift_enter(self, L, ticket, n, new_pos, lm, avg):
        """the host side of an asynchronous shift between ws_shift_begin and the start of the worker"""
        lm.follow(new_pos)  # the host view of the window
        # revisited space: chunks the global map already has overwrite the default fill
        cs = GlobalMap.CHUNK_SIZE
        lo, hi = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
        for i in range(n):
            check(L.ws_shift_entering(ticket, i, _ptr(lo), _ptr(hi)), "ws_shift_entering")
            # a later axis step moves the window again: only the part of the slab still inside the FINAL window counts
            wlo, whi = lm.window()
            a, b = np.maximum(lo.astype(np.int64), wlo), np.minimum(hi.astype(np.int64), whi)
            if np.any(a > b):
                continue
            c0, c1 = np.floor_divide(a, cs), np.floor_divide(b, cs)
            for cx in range(int(c0[0]), int(c1[0]) + 1):
                for cy in range(int(c0[1]), int(c1[1]) + 1):
                    for cz in range(int(c0[2]), int(c1[2]) + 1):
                        if not lm.map_.has_chunk(cx, cy, cz):
                            continue
                        base = np.array([cx, cy, cz], dtype=np.int64) * cs
                        sa, sb = np.maximum(a, base), np.minimum(b, base + cs - 1)
                        avg.insert_box(sa, sb, lm.map_.load_box(sa, sb))

    def shift_map_device(self, new_pos):
        """TSDFMapping::map_shift with the global map in device memory (ws_shift_device): per axis the leaving slab goes into
        the chunks of device_global_map, pos / offset of both maps move, and the entering slab comes out of them -- revisited
        space and corners included -- as device-to-device copies in stream order.  Nothing is transferred, staged or filed on the
        host; the call returns after enqueueing.  The host LocalMap follows pos / offset."""
        if self.device_global_map_ is None:
            raise WsError("shift_map_device: this TSDFMapping has no device_global_map")
        self.wait_shift()
        lm = self.local_map_
        new_pos = _i3(new_pos)
        with self.mutex_:
            self._pyramid_touch(*lm.window())  # (the leaving slabs go into chunks that global_pyramid has to refresh)
            check(self.tsdf_._L.ws_shift_device(self.tsdf_.handle, self.device_global_map_.handle, _ptr(new_pos)), "ws_shift_device")
            lm.follow(new_pos)

    def reserve_shift(self, shift_voxels: int):
        """staging for asynchronous shifts of up to `shift_voxels` per axis (plus slack), allocated now instead of inside
        the first shift (a pinned allocation of that size takes tens of milliseconds)"""
        s = self.local_map_.size.astype(np.int64)
        d = int(shift_voxels) + 8
        total = int(d * (s[0] * s[1] + s[1] * s[2] + s[0] * s[2]))
        check(self.tsdf_._L.ws_shift_reserve(self.tsdf_.handle, total), "ws_shift_reserve")

    def wait_shift(self):
        w = getattr(self, "_shift_worker", None)
        if w is not None:
            w.join()
            self._shift_worker = None
            err, self._shift_error = getattr(self, "_shift_error", None), None
            if err is not None:
                raise WsError(f"asynchronous map shift: the leaving slabs were not filed into the global map ({err!r})") from err

    def write_back(self, box_lo=None, box_hi=None):
        """HDF5LocalMap::write_back + HDF5GlobalMap::write_back (hdf5_local_map.cpp:210-217, app.cpp:220) from the
        DEVICE map: every 64^3 chunk the window overlaps is gathered out of the ring buffer by the GPU
        (ws_map_extract_box: chunk layout, x major / z fastest), merged into the global map's chunk and written to
        its file.  The reference downloads the whole window and copies voxel by voxel on the host.
        box_lo / box_hi (inclusive world voxels) restrict the export to a part of the window.
        With a device_global_map: ws_store_save_box of the (clipped) window, DeviceGlobalMap.flush_to the host global map, its
        write_back -- the same chunks and the same file."""
        self.wait_shift()
        lm, avg = self.local_map_, self.tsdf_.avg_map()
        cs = GlobalMap.CHUNK_SIZE
        with self.mutex_:
            lo, hi = lm.window()
            if box_lo is not None:
                lo = np.maximum(lo, np.asarray(box_lo, dtype=np.int64))
            if box_hi is not None:
                hi = np.minimum(hi, np.asarray(box_hi, dtype=np.int64))
            if self.device_global_map_ is not None:
                # the window goes into the device chunks in one launch, and the chunks into the host map and its file
                self.device_global_map_.save_box(self.tsdf_, lo, hi)
                self.device_global_map_.flush_to(lm.map_)
                lm.map_.write_back()
                return
            # one gather per 64-voxel-thick x slab of chunks (a few large device->host copies instead of one small one
            # per chunk); save_box cuts the slab into its chunks
            for cx in range(int(np.floor_divide(lo[0], cs)), int(np.floor_divide(hi[0], cs)) + 1):
                a, b = lo.copy(), hi.copy()
                a[0], b[0] = max(lo[0], cx * cs), min(hi[0], cx * cs + cs - 1)
                lm.map_.save_box(a, b, avg.extract_box(a, b))
            lm.map_.write_back()


class TSDFRegistration(TSDFMapping):
    """cuda::TSDFRegistration (tsdf_registration.cpp:22-96)."""

    def __init__(self, params: Params, local_map: LocalMap, ctx: Context | None = None, flags: int = WS_REG_ALL_POINTS,
                 device_global_map: "DeviceGlobalMap | None" = None):
        super().__init__(params, local_map, ctx, device_global_map)
        self.reg_ = RegistrationCuda(self.cuda_map_, ctx, flags)
        self.last_iterations = 0

    def register_cloud(self, cloud, pretransform):
        """Returns total_transform (4x4 float32); Gauss-Newton loop on the device."""
        self.reg_.prepare_registration(cloud)
        r, m = self.params_.registration, self.params_.map
        with self.mutex_:
            T, it = self.reg_.register_cloud(self.tsdf_.device_map(), pretransform, r.max_iterations, r.it_weight_gradient,
                                             r.epsilon, m.resolution)
        self.last_iterations = it
        return T

    def register_candidates(self, cloud, poses):
        """register_cloud from every pose of `poses` (k, 4, 4) in one launch: (T[k, 4, 4], iterations[k], e[k], c[k]); rank them
        with batch_best(e, c, min_count)."""
        self.reg_.prepare_registration(cloud)
        r, m = self.params_.registration, self.params_.map
        with self.mutex_:
            return self.reg_.register_cloud_batch(self.tsdf_.device_map(), poses, r.max_iterations, r.it_weight_gradient, r.epsilon,
                                                  m.resolution)

    def relocalize(self, cloud, guess, radius_m, step_m, yaw_range_deg=0.0, yaw_step_deg=0.0, min_fraction=0.5):
        """Re-localise inside the map: register `cloud` from every pose of candidate_poses(guess, ...) and keep the one whose final
        mean error is smallest among those that matched at least min_fraction of the points.
        Returns (best_pose 4x4 float32, best_index, table) with table = dict(start=, pose=, iterations=, e=, c=) over all candidates;
        raises WsError if no candidate reaches min_fraction."""
        poses = candidate_poses(guess, radius_m, step_m, yaw_range_deg, yaw_step_deg)
        T, it, e, c = self.register_candidates(cloud, poses)
        n = int(cloud.shape[0])
        min_count = max(1, int(np.ceil(float(min_fraction) * n)))
        best = batch_best(e, c, min_count)
        table = {"start": poses, "pose": T, "iterations": it, "e": e, "c": c}
        if best < 0:
            raise WsError(f"relocalize: none of the {len(poses)} candidates matched {min_count} of {n} points (best count {int(c.max()) if len(c) else 0})")
        self.last_iterations = int(it[best])
        return T[best].copy(), best, table
