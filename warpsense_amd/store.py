"""The global map in device memory (ws_store_*): DeviceGlobalMap, the device twin of GlobalMap, and its queries."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import _i3, _i3c, _ptr, pack_entry, unpack_entry
from ._lib import WS_MAP_AVG, check
from .context import Context
from .changes import ChangeResult, _changes_call
from .fuse import FuseStats, _fuse_call, fuse_pose
from .global_map import GlobalMap
from .pack import PackedMap, _pack_call, _unpack_call
from .pyramid import CoarsenStats, _coarsen_call
from .clearance import _clearance_call
from .ground import _ground_call, _ground_distance_call
from .queries import _box_ptrs, _distance_call, _frontier_call, _reach_call, _reach_lookup_call, _reach_paths_call, _mesh_call, _raycast_call, _sample_call, _surface_call, _timing, _view_gain_call


class DeviceGlobalMap:
    """The global map in device memory (ws_store, include/warpsense_hip.h): the device twin of GlobalMap.  64^3-voxel chunks of raw
    uint32 entries in HBM, index x*4096 + y*64 + z, keyed by floor(world voxel / 64); chunks never seen hold the default entry.  The
    key -> slot directory is the host's.  TSDFMapping(..., device_global_map=this).shift_map_device saves the leaving slabs into
    it and loads the entering ones from it in stream order; flush_to() merges it into a host GlobalMap (and its .h5 file)."""

    CHUNK_SIZE = 64
    CHUNK_WORDS = 64 ** 3

    def __init__(self, default_value, default_weight=0, max_chunks: int = 0, segment_chunks: int = 0, ctx: Context | None = None):
        self.ctx = ctx or Context.default()
        self._L = self.ctx._L
        self.default_raw = int(pack_entry(default_value, default_weight))
        h = C.c_void_p()
        check(self._L.ws_store_create(self.ctx.handle, self.default_raw, int(max_chunks), int(segment_chunks), C.byref(h)), "ws_store_create")
        self.handle = h

    def count(self) -> int:
        n = C.c_uint64(0)
        check(self._L.ws_store_count(self.handle, C.byref(n), None), "ws_store_count")
        return int(n.value)

    def capacity(self) -> int:
        n = C.c_uint64(0)
        check(self._L.ws_store_count(self.handle, None, C.byref(n)), "ws_store_count")
        return int(n.value)

    def reserve(self, n: int):
        """segments for n chunks now, so that no shift has to allocate (and wait for the device)"""
        check(self._L.ws_store_reserve(self.handle, int(n)), "ws_store_reserve")

    def keys(self) -> list:
        """the chunk keys, ascending (cx, cy, cz)"""
        n = C.c_size_t(0)
        check(self._L.ws_store_keys(self.handle, None, 0, C.byref(n)), "ws_store_keys")
        keys = np.zeros((n.value, 3), dtype=np.int32)
        check(self._L.ws_store_keys(self.handle, _ptr(keys), n.value, C.byref(n)), "ws_store_keys")
        return [tuple(int(v) for v in k) for k in keys[:n.value]]

    def has_chunk(self, cx, cy, cz) -> bool:
        return bool(self._L.ws_store_has(self.handle, _i3c((cx, cy, cz))))

    def chunk(self, key):
        """a host copy of one chunk (262 144 uint32), None if the store does not hold it"""
        out = np.empty(self.CHUNK_WORDS, dtype=np.uint32)
        found = C.c_int32(0)
        check(self._L.ws_store_get_chunk(self.handle, _i3c(tuple(key)), _ptr(out), C.byref(found)), "ws_store_get_chunk")
        return out if found.value else None

    def put_chunk(self, key, data):
        data = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1)
        assert data.size == self.CHUNK_WORDS
        check(self._L.ws_store_put_chunk(self.handle, _i3c(tuple(key)), _ptr(data)), "ws_store_put_chunk")

    def drop_chunk(self, key):
        check(self._L.ws_store_drop_chunk(self.handle, _i3c(tuple(key))), "ws_store_drop_chunk")

    def save_box(self, tsdf: "TSDFCuda", lo, hi, which: int = WS_MAP_AVG):
        """the box [lo, hi] of the window of `tsdf` into the chunks (ws_store_save_box; stream-ordered, no wait)"""
        check(self._L.ws_store_save_box(self.handle, tsdf.handle, int(which), _ptr(_i3(lo)), _ptr(_i3(hi))), "ws_store_save_box")

    def load_box(self, tsdf: "TSDFCuda", lo, hi, which: int = WS_MAP_AVG):
        """the chunks into the box [lo, hi] of the window of `tsdf`, the default entry where there is no chunk (ws_store_load_box)"""
        check(self._L.ws_store_load_box(self.handle, tsdf.handle, int(which), _ptr(_i3(lo)), _ptr(_i3(hi))), "ws_store_load_box")

    def timing(self, enable: int = -1):
        """device milliseconds of the save and of the load launches of the last call (ws_debug_store_timing)"""
        return _timing(self._L, "ws_debug_store_timing", self.handle, 2, enable)

    def surface(self, tau, resolution, lo=None, hi=None, band=None, marker=False, device=False):
        """The surface cloud of the chunks on the device (ws_store_surface; the rules are those of ws_map_surface, stated in
        include/warpsense_hip.h): every voxel of a present chunk inside the inclusive world-voxel box [lo, hi] (both None: every
        present chunk) with weight > 0 and abs(value) < band (None: tau), in ascending world (x, y, z), z fastest, across chunk
        borders.  Voxels of absent chunks never qualify.  tau, resolution: the map's (the store knows neither); they decide the
        marker's colour and point.

        Returns the same forms as DeviceMapMemWrapper.surface: the records, or with `marker` (records, (n, 7) float32);
        device=True: torch tensors that ALIAS the store's buffers, valid until the next surface() on this store."""
        return _surface_call(self._L, "ws_store_surface", self, (), lo, hi, band, (int(tau), int(resolution)), marker, device)

    def surface_timing(self, enable: int = -1):
        """device milliseconds of the count passes, the scan and the emit pass of the last surface() (ws_debug_store_surface_timing)"""
        return _timing(self._L, "ws_debug_store_surface_timing", self.handle, 3, enable)

    def mesh(self, resolution, lo=None, hi=None, any_weight=False, device=False):
        """The mesh of the chunks on the device (ws_store_mesh; the rules are those of ws_map_mesh, stated in
        include/warpsense_hip.h): the surface of everything the store holds inside the inclusive world-voxel box [lo, hi] (both
        None: the bounding box of the present chunks), in the order of DeviceMapMemWrapper.mesh across chunk borders.  Voxels of
        absent chunks are not valid.  resolution: the map's, in mm per voxel (the store does not know it).

        Returns (vertices, faces) like DeviceMapMemWrapper.mesh; device=True: torch tensors that ALIAS the store's buffers, valid
        until the next mesh() on this store."""
        return _mesh_call(self._L, "ws_store_mesh", self, (), lo, hi, (int(resolution),), any_weight, device)

    def mesh_timing(self, enable: int = -1):
        """device milliseconds of the count passes, the scan and the emit passes of the last mesh() (ws_debug_store_mesh_timing)"""
        return _timing(self._L, "ws_debug_store_mesh_timing", self.handle, 3, enable)

    def raycast(self, resolution, origin_mm, dirs, max_range_mm, lo=None, hi=None, any_weight=False, gradient=False, targets=False):
        """Ray cast of the chunks on the device (ws_store_raycast; the rules are those of ws_map_raycast, stated in
        include/warpsense_hip.h): per ray the first crossing of the surface from the outside within max_range_mm, through
        everything the store holds inside the inclusive world-voxel box [lo, hi] (both None: everything).  Voxels of absent chunks
        are not valid.  resolution: the map's, in mm per voxel.  origin_mm, dirs, targets, any_weight, gradient and the returned
        (records, gradient | None) are those of DeviceMapMemWrapper.raycast; `last_hits` keeps the call's number of hits."""
        box = _box_ptrs("raycast", lo, hi)
        rec, grad, self.last_hits = _raycast_call(self._L, "ws_store_raycast", self.handle, box, origin_mm, dirs, max_range_mm, (int(resolution),),
                                                  any_weight, gradient, targets)
        return rec, grad

    def sample(self, resolution, points, band_mm, lo=None, hi=None, any_weight=False, gradient=False, select=None, device=False):
        """What the chunks on the device say at `points` (ws_store_sample; the rules are those of ws_map_sample, stated in
        include/warpsense_hip.h), through everything the store holds inside the inclusive world-voxel box [lo, hi] (both None:
        everything).  Voxels of absent chunks are not valid.  resolution: the map's, in mm per voxel; band_mm > 0.  The other arguments
        and the returned (records, counts, gradient | None, selection | None) are those of DeviceMapMemWrapper.sample."""
        box = _box_ptrs("sample", lo, hi)
        return _sample_call(self._L, "ws_store_sample", self, box, points, band_mm, (int(resolution),), any_weight, gradient, select, device)

    def sample_timing(self, enable: int = -1):
        """device milliseconds of the upload, the sample pass and the select passes of the last sample() (ws_debug_store_sample_timing)"""
        return _timing(self._L, "ws_debug_store_sample_timing", self.handle, 3, enable)

    def raycast_timing(self, enable: int = -1):
        """device milliseconds of the upload, the march and the gradient pass of the last raycast() (ws_debug_store_raycast_timing)"""
        return _timing(self._L, "ws_debug_store_raycast_timing", self.handle, 3, enable)

    def distance(self, lo=None, hi=None, max_dist_vox=20, unknown_occupied=False, columns=False, any_weight=False, device=False):
        """The distance field of the chunks on the device (ws_store_distance; the rules are those of ws_map_distance, stated in
        include/warpsense_hip.h): per voxel of the inclusive world-voxel box [lo, hi] (both None: the bounding box of the present
        chunks) the squared Euclidean distance in voxels to the nearest occupied voxel of the box, clamped at max_dist_vox squared
        (1 .. 255).  Voxels of absent chunks are unknown: with unknown_occupied they are sites.  columns, any_weight, the returned
        uint32 records shaped (nx, ny, nz) or (nx, ny) and `last_sites` are those of DeviceMapMemWrapper.distance.  Unlike mesh()
        and raycast() the result is dense: 8 bytes of device memory per record of the box.
        device=True: a torch int32 tensor of that shape on the GPU that ALIASES the store's buffer, valid until the next distance()
        on this store."""
        def bounding_shape():
            keys = np.asarray(self.keys(), dtype=np.int64).reshape(-1, 3)
            return tuple(int(v) for v in (keys.max(axis=0) - keys.min(axis=0) + 1) * self.CHUNK_SIZE) if len(keys) else (0, 0, 0)
        rec, self.last_sites = _distance_call(self._L, "ws_store_distance", self, (), lo, hi, max_dist_vox, unknown_occupied, columns, any_weight,
                                              device, bounding_shape)
        return rec

    def distance_timing(self, enable: int = -1):
        """device milliseconds of pass 0 and of the x, y and z passes of the last distance() (ws_debug_store_distance_timing)"""
        return _timing(self._L, "ws_debug_store_distance_timing", self.handle, 4, enable)

    def ground(self, lo=None, hi=None, clear_vox=20, any_weight=False, unknown_headroom=False, top=False, device=False):
        """The ground layer of the chunks on the device (ws_store_ground; the rules are those of ws_map_ground, stated in
        include/warpsense_hip.h) over the inclusive world-voxel box [lo, hi] (both None: the bounding box of the present chunks).
        Voxels of absent chunks are unknown.  The arguments and the returned GroundResult are those of DeviceMapMemWrapper.ground;
        device=True: its records ALIAS the store's buffer, valid until the next ground() on this store."""
        return _ground_call(self._L, "ws_store_ground", self, (), lo, hi, clear_vox, any_weight, unknown_headroom, top, device)

    def ground_distance(self, max_step_q8, max_dist_vox=20, unknown_occupied=False, device=False):
        """The column distance field over the LAST ground() result of this store (ws_store_ground_distance), as
        DeviceMapMemWrapper.ground_distance: it REPLACES the result of distance(), and reach() plans over it."""
        rec, self.last_sites = _ground_distance_call(self._L, "ws_store_ground_distance", self, max_step_q8, max_dist_vox, unknown_occupied, device)
        return rec

    def ground_timing(self, enable: int = -1):
        """device milliseconds of pass 1 (levels) and pass 2 (steps) of the last ground() (ws_debug_store_ground_timing)"""
        return _timing(self._L, "ws_debug_store_ground_timing", self.handle, 2, enable)

    def frontier(self, lo=None, hi=None, min_value=0, any_weight=False, clusters=False, device=False):
        """The frontier of the chunks on the device (ws_store_frontier; the rules are those of ws_map_frontier, stated in
        include/warpsense_hip.h): the observed-free voxels of the inclusive world-voxel box [lo, hi] (both None: the bounding box of
        the present chunks) that touch a never-observed voxel of the box, across chunk borders.  Voxels of absent chunks are unknown.
        The faces of the box are no frontier: pass a box one voxel larger than the bounding box to get the outer faces of the mapped
        volume.  The arguments and the returned records or (records, labels, table) are those of DeviceMapMemWrapper.frontier;
        device=True: torch tensors that ALIAS the store's buffers, valid until the next frontier() on this store."""
        return _frontier_call(self._L, "ws_store_frontier", self, (), lo, hi, min_value, any_weight, clusters, device)

    def frontier_timing(self, enable: int = -1):
        """device milliseconds of the count passes, the scan, the emit pass and the clustering of the last frontier() (ws_debug_store_frontier_timing)"""
        return _timing(self._L, "ws_debug_store_frontier_timing", self.handle, 4, enable)

    def view_gain(self, resolution, origins_mm, dirs, max_range_mm, lo=None, hi=None, min_value=0, any_weight=False, rays=False, device=False):
        """What the sensor would see from candidate poses, through the chunks on the device (ws_store_view_gain; the rules are those of
        ws_map_view_gain, stated in include/warpsense_hip.h) inside the inclusive world-voxel box [lo, hi] (both None: the bounding box
        of the present chunks).  Voxels of absent chunks are unknown: they count, and block nothing.  resolution: the map's, in mm
        per voxel.  The other arguments, the returned records or (records, rays) and `last_view_gain` are those of
        DeviceMapMemWrapper.view_gain; device=True: torch tensors that ALIAS the store's buffers, valid until the next view_gain() on
        this store."""
        rec, ray, best = _view_gain_call(self._L, "ws_store_view_gain", self, (), lo, hi, origins_mm, dirs, max_range_mm, (int(resolution),), min_value,
                                         any_weight, rays, device)
        self.last_view_gain = dict(best_unknown_k2=best, views=int(rec.shape[0]), rays=int(np.asarray(dirs).reshape(-1, 3).shape[0]))
        return (rec, ray) if rays else rec

    def view_gain_timing(self, enable: int = -1):
        """device milliseconds of the upload, of the fan preparation with the march, and of the maximum pass of the last view_gain()
        (ws_debug_store_view_gain_timing)"""
        return _timing(self._L, "ws_debug_store_view_gain_timing", self.handle, 3, enable)

    def clearance(self, resolution, poses, body, soft_mm=0, per_pose=False, outside_ok=False, device=False):
        """Candidate trajectories against the LAST distance() or ground_distance() result of this store (ws_store_clearance; the rules
        are those of ws_map_clearance, stated in include/warpsense_hip.h).  resolution: the map's, in mm per voxel.  The other
        arguments and the returned ClearanceResult are those of DeviceMapMemWrapper.clearance; device=True: tensors that ALIAS the
        store's buffers, valid until the next clearance() on this store."""
        return _clearance_call(self._L, "ws_store_clearance", self, poses, body, soft_mm, (int(resolution),), per_pose, outside_ok, device)

    def clearance_timing(self, enable: int = -1):
        """device milliseconds of the upload, of the trajectory pass and of the pass that finds the best of the last clearance()
        (ws_debug_store_clearance_timing)"""
        return _timing(self._L, "ws_debug_store_clearance_timing", self.handle, 3, enable)

    def reach(self, seeds, clear_d2=0, unknown_free=False, max_rounds=0, device=False):
        """The geodesic field over the LAST distance() result of this store (ws_store_reach; the rules are stated in
        include/warpsense_hip.h): per record the cost of the cheapest 26-connected (columns: 8-connected) path from `seeds` ((n, 3)
        int32 world voxels) over records that are free (unknown_free: or unknown) with d2 >= clear_d2; a face step weighs 10, an edge
        step 14, a corner step 17, unreachable is 0xFFFFFFFF (reach_mm turns costs into millimetres).  max_rounds: 0 for the default
        cap.  Returns the uint32 costs shaped like that distance result; `last_reach` keeps dict(seeded, reached, rounds).
        device=True: a torch int32 tensor on the GPU that ALIASES the library's buffer, valid until the next reach()."""
        cost, self.last_reach = _reach_call(self._L, "ws_store_reach", self, seeds, clear_d2, unknown_free, max_rounds, device)
        return cost

    def reach_lookup(self, points):
        """The costs of the last reach() at world voxels: an (n, 3) or (n, 4) int32 numpy array gives a uint32 numpy array; a CUDA
        tensor of such rows -- the records of frontier(device=True) -- gives an int32 CUDA tensor of the same bits.  Outside the box
        of the reach result: 0xFFFFFFFF."""
        return _reach_lookup_call(self._L, "ws_store_reach_lookup", self, points)

    def reach_paths(self, goals, cap_steps=0):
        """The paths of the last reach() from `goals` ((g, 3) int32 world voxels) back to a seed.  Returns (headers, records) of dtypes
        REACH_PATH_HEADER [g] (cost, steps, written, status: 0 reached, 1 not reachable, 2 outside) and REACH_PATH_RECORD
        [g, cap_steps] (x, y, z, cost; goal first); cap_steps = 0 asks for the headers alone."""
        return _reach_paths_call(self._L, "ws_store_reach_paths", self, goals, cap_steps)

    def reach_timing(self, enable: int = -1):
        """device milliseconds of the seeding, of all rounds as one span and of the count pass of the last reach() (ws_debug_store_reach_timing)"""
        return _timing(self._L, "ws_debug_store_reach_timing", self.handle, 3, enable)

    def fuse(self, other: "DeviceGlobalMap", T_src_to_dst, max_weight, count_only=False, pivot_src_mm=None, *, resolution) -> FuseStats:
        """`other` resampled on this map's voxel lattice under a rigid pose and integrated into it with the weighted average of the
        TSDF update, on the device (ws_store_fuse; the rules are stated in include/warpsense_hip.h).  T_src_to_dst: the 4 x 4
        float64 transform in mm from the frame of `other` into this map's (fuse_pose makes the integer pull transform from it,
        around pivot_src_mm), or the 15 int32 of a ws_fuse_pose as they are.  resolution: the maps', in mm per voxel (a store does
        not know it); max_weight: 1 .. 32767.  count_only: the statistics of the call without a change to this map --
        FuseStats.disagreement_mm then says how well the two maps agree under the pose.  `other` is only read."""
        pose = np.asarray(T_src_to_dst)
        pose = pose if pose.size == 15 else fuse_pose(pose, pivot_src_mm)
        return _fuse_call(self._L, self, other, pose, resolution, max_weight, count_only)

    @property
    def last_fuse_timing(self):
        """device milliseconds of the plan's upload, the count pass and the write pass of the last fuse() into this map (zeros unless
        fuse_timing(1) switched the events on before it)"""
        return self.fuse_timing()

    def fuse_timing(self, enable: int = -1):
        """ws_debug_store_fuse_timing: read the last call's three spans; enable 1 / 0 switches the events on / off"""
        return _timing(self._L, "ws_debug_store_fuse_timing", self.handle, 3, enable)

    def changes(self, ref: "DeviceGlobalMap", pose=None, pivot_ref_mm=None, *, resolution, band, free_value, min_weight=1, lo=None, hi=None, kinds="both",
                clusters=False) -> ChangeResult:
        """Where this map ("now") differs from `ref` ("before"), on the device (ws_store_changes; the rule is stated in
        include/warpsense_hip.h): on this map's voxel lattice, inside the inclusive world-voxel box [lo, hi] (both None: the bounding
        box of the present chunks), a voxel whose entry has weight >= min_weight is compared with the fuse's sample of `ref` at its
        place.  abs(value) < band is occupied, value >= free_value is free (raw values; band <= free_value); occupied here and free
        there has APPEARED (kind 1), free here and occupied there has VANISHED (kind 2); unknown on either side is never a change.
        pose: None for the identity, the 4 x 4 float64 transform in mm from the frame of `ref` into this map's (fuse_pose makes the
        integer pull transform from it, around pivot_ref_mm), or the 15 int32 of a ws_fuse_pose.  resolution: the maps', in mm per
        voxel.  kinds: "both", "appeared" or "vanished" become records; clusters: 26-connected clusters of the records as in
        frontier().  Both maps are only read.  Returns a ChangeResult."""
        pose = np.eye(4) if pose is None else np.asarray(pose)
        pose = pose if pose.size == 15 else fuse_pose(pose, pivot_ref_mm)
        return _changes_call(self._L, self, ref, pose, resolution, lo, hi, band, free_value, min_weight, kinds, clusters)

    def changes_timing(self, enable: int = -1):
        """device milliseconds of the uploads with the count pass, the scan, the emit pass and the clustering of the last changes()
        (ws_debug_store_changes_timing)"""
        return _timing(self._L, "ws_debug_store_changes_timing", self.handle, 4, enable)

    def coarsen(self, dst: "DeviceGlobalMap", keys=None, min_observed=8, stats=True) -> CoarsenStats | None:
        """This map at half the resolution into `dst`, on the device (ws_store_coarsen; the rule is stated in
        include/warpsense_hip.h): every voxel of `dst` is 2 x 2 x 2 voxels of this map, the floor of the mean of the observed
        ones (weight > 0) with the smallest of their weights where at least min_observed (1 .. 8) are observed, the default entry
        of `dst` elsewhere.  keys: the (n, 3) chunks of `dst` to rebuild whole (None: the parents of every chunk of this map);
        every other chunk of `dst` keeps its bytes.  stats=False returns None after enqueueing, without a wait.  This map is only
        read; `dst` is queried with twice this map's resolution."""
        return _coarsen_call(self._L, self, dst, keys, min_observed, stats)

    def coarsen_timing(self, enable: int = -1):
        """device milliseconds of the plan's upload and of the pass of the last coarsen() INTO this map (ws_debug_store_coarsen_timing)"""
        return _timing(self._L, "ws_debug_store_coarsen_timing", self.handle, 2, enable)

    def pack(self, keys=None, device=False, direct=False) -> PackedMap:
        """Chunks of this map in packed form, made on the device (ws_store_pack; the format is stated in include/warpsense_hip.h):
        the (n, 3) chunks `keys` names (None: every chunk), in ascending key order whatever the order given, as 40-word headers
        and one payload stream in which a brick of 8^3 words that is all default takes nothing and one that repeats one word takes
        one word.  A key the map does not hold, or one named twice, raises.  device=True: the payload is an int32 torch tensor
        that ALIASES the store's buffer, valid until the next pack() on this store (the headers always come to the host).
        direct: the emit pass without its LDS staging (measurement; the bytes are the same).  This map is only read."""
        return _pack_call(self._L, self, keys, device, direct)

    def unpack(self, packed: PackedMap):
        """The chunks of `packed` created or overwritten whole (ws_store_unpack, or ws_store_unpack_dev for a payload on the device);
        default bricks get packed.fill, whatever this map's default is.  Chunks that are not listed keep their bytes.  A stream
        that fails ws_pack_check, or more chunks than max_chunks allows, raises and leaves the map unchanged."""
        _unpack_call(self._L, self, packed)

    def clone(self, ctx: Context | None = None) -> "DeviceGlobalMap":
        """A byte-exact copy of this map as a new DeviceGlobalMap with the same default: pack(), then unpack from the payload where
        it lies on the device; only the headers visit the host.  Returns after the copy has run."""
        value, weight = (int(v) for v in unpack_entry(self.default_raw))
        other = DeviceGlobalMap(value, weight, ctx=ctx or self.ctx)
        other.unpack(self.pack(device=True))
        check(self._L.ws_sync(other.ctx.handle), "ws_sync")
        return other

    def save_packed(self, path, **meta) -> PackedMap:
        """this map packed into a `.wspk` file (PackedMap.save); meta: resolution=, tau= and whatever else the file should say"""
        packed = self.pack()
        packed.resolution, packed.tau = meta.pop("resolution", None), meta.pop("tau", None)
        packed.save(path, **meta)
        return packed

    def load_packed(self, path) -> PackedMap:
        """the chunks of a `.wspk` file into this map (PackedMap.load, unpack); returns the PackedMap with the file's metadata"""
        packed = PackedMap.load(path)
        self.unpack(packed)
        return packed

    def pack_timing(self, enable: int = -1):
        """device milliseconds of the classify pass, the scan and the emit pass of the last pack(), or of the last unpack()'s launch
        and zeros if that came later (ws_debug_store_pack_timing)"""
        return _timing(self._L, "ws_debug_store_pack_timing", self.handle, 3, enable)

    def flush_to(self, global_map: GlobalMap):
        """every chunk merged into a host GlobalMap: into its chunk cache (activate_chunk), or, for a map with a file, straight
        into the file (GlobalMap._write_chunk) unless the chunk is active in the cache"""
        for key in self.keys():
            data = self.chunk(key)
            with global_map.lock:
                if global_map._file is not None and key not in global_map.chunks:
                    global_map._write_chunk(key, data)
                else:
                    global_map.activate_chunk(*key)[:] = data

    def load_from(self, global_map: GlobalMap, keys=None):
        """chunks of a host GlobalMap (None: all it holds, in memory and in its file) into the store, to continue a saved map"""
        if keys is None:
            keys = set(global_map.chunks) | (set(global_map._in_file) if global_map._file is not None else set())
        for key in sorted(tuple(int(v) for v in k) for k in keys):
            if not global_map.has_chunk(*key):
                continue
            with global_map.lock:
                self.put_chunk(key, global_map.activate_chunk(*key))

    def close(self):
        if self.handle:
            self._L.ws_store_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chunks_of_box(lo, hi) -> np.ndarray:
    """host only: the (n, 3) chunk keys an inclusive world-voxel box overlaps, ascending (ws_store_chunks_of_box)"""
    L = _lib.load()
    n = C.c_size_t(0)
    lo, hi = _i3(lo), _i3(hi)
    check(L.ws_store_chunks_of_box(_ptr(lo), _ptr(hi), None, 0, C.byref(n)), "ws_store_chunks_of_box")
    keys = np.zeros((n.value, 3), dtype=np.int32)
    check(L.ws_store_chunks_of_box(_ptr(lo), _ptr(hi), _ptr(keys), n.value, C.byref(n)), "ws_store_chunks_of_box")
    return keys
