"""The ground layer of the window map (ws_map_ground) and of the chunk store (ws_store_ground): the record, the result, the two calls
that DeviceMapMemWrapper and DeviceGlobalMap share, and the ground queries of TSDFMapping (mapping.py mixes them in).  The rules are
stated in include/warpsense_hip.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import _device_tensor, _ptr
from ._lib import WsError, check
from .queries import _box_ptrs
from .reach import ReachQueries

# one record of ws_map_ground / ws_store_ground: the level's voxel, and frac (bits 0..7), step (bits 8..23), class (bits 30..31)
GROUND_RECORD = np.dtype([("z", "<i4"), ("w", "<u4")])
GROUND_UNKNOWN, GROUND_GROUND, GROUND_BLOCKED, GROUND_VOID = range(4)


class GroundResult:
    """The ground layer of a box: `records` (GROUND_RECORD, shaped (nx, ny)), `lo` (the box's first world voxel, three ints), `ext`
    (its extent) and `counts` (columns per class: unknown, ground, blocked, void)."""

    def __init__(self, records, lo, ext, counts):
        self.records, self.lo, self.ext, self.counts = records, tuple(int(v) for v in lo), tuple(int(v) for v in ext), np.asarray(counts, dtype=np.uint64)

    @property
    def z(self):
        """the level's voxel per column (int32; 0 without a level)"""
        return self.records["z"]

    @property
    def cls(self):
        """the class per column (uint8): 0 unknown, 1 ground, 2 blocked, 3 void"""
        return (self.records["w"] >> np.uint32(30)).astype(np.uint8)

    @property
    def frac(self):
        """the zero crossing above the level's voxel in 1/256 voxel (uint8)"""
        return (self.records["w"] & np.uint32(0xFF)).astype(np.uint8)

    @property
    def step_q8(self):
        """the largest height step to a neighbouring ground column in 1/256 voxel (uint16, saturated)"""
        return ((self.records["w"] >> np.uint32(8)) & np.uint32(0xFFFF)).astype(np.uint16)

    @property
    def height_q8(self):
        """256 z + frac per column (int64); meaningful where cls == 1"""
        return self.z.astype(np.int64) * 256 + self.frac.astype(np.int64)

    def height_mm(self, resolution):
        """the height of the ground in millimetres between voxel centres (float64; NaN where the column has no level)"""
        h = self.height_q8.astype(np.float64) * (float(resolution) / 256.0)
        return np.where(self.cls == GROUND_GROUND, h, np.nan)

    def traversable(self, max_step_mm, resolution):
        """ground columns whose step stays within max_step_mm (bool): the FREE columns of ground_distance(max_step_q8(...))"""
        return (self.cls == GROUND_GROUND) & (self.step_q8 <= max_step_q8(max_step_mm, resolution))


def max_step_q8(max_step_mm, resolution) -> int:
    """millimetres to the step unit of a ground record: floor(256 mm / resolution), 0 .. 65535"""
    return int(min(65535, max(0, int(np.floor(float(max_step_mm) * 256.0 / float(resolution))))))


def _ground_call(L, name, owner, lead, lo, hi, clear_vox, any_weight, unknown_headroom, top, device):
    """The ground call `name` (ws_map_ground, ws_store_ground) on owner.handle and its result: `lead` are the arguments of the entry
    point before the box.  Returns a GroundResult; with device=True its records are a torch int32 tensor (nx, ny, 2) that ALIASES the
    library's buffer (owner keeps it alive), valid until the next ground call."""
    box = _box_ptrs("ground", lo, hi)
    flags = ((_lib.WS_GROUND_ANY_WEIGHT if any_weight else 0) | (_lib.WS_GROUND_UNKNOWN_HEADROOM if unknown_headroom else 0)
             | (_lib.WS_GROUND_TOP if top else 0))
    counts = np.zeros(4, dtype=np.uint64)
    check(getattr(L, name)(owner.handle, *lead, *box, int(clear_vox), flags, _ptr(counts)), name)
    blo, ext = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.uint32)
    check(getattr(L, name + "_box")(owner.handle, _ptr(blo), _ptr(ext)), name + "_box")
    shape = (int(ext[0]), int(ext[1]))
    n = shape[0] * shape[1]
    cnt = C.c_size_t(0)
    if device:
        ptr = getattr(L, name + "_dev")(owner.handle, C.byref(cnt))
        if int(cnt.value) != n:
            raise WsError("ground: another call replaced the result")
        return GroundResult(_device_tensor(ptr, shape + (2,), "<i4", owner), blo, ext, counts)
    rec = np.empty(n, dtype=GROUND_RECORD)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), n, C.byref(cnt)), name + "_download")
    if int(cnt.value) != n:
        raise WsError("ground: another call replaced the result before it was downloaded")
    return GroundResult(rec.reshape(shape), blo, ext, counts)


def _ground_distance_call(L, name, owner, max_step, max_dist_vox, unknown_occupied, device):
    """The bridge `name` (ws_map_ground_distance, ws_store_ground_distance) on owner.handle: the column distance field over the owner's
    last ground result, which replaces the owner's distance result.  Returns (records shaped (nx, ny), sites)."""
    flags = _lib.WS_DISTANCE_UNKNOWN_OCCUPIED if unknown_occupied else 0
    sites = C.c_size_t(0)
    check(getattr(L, name)(owner.handle, int(max_step), int(max_dist_vox), flags, C.byref(sites)), name)
    ext = np.zeros(3, dtype=np.uint32)
    box_name = name.replace("_distance", "_box")
    check(getattr(L, box_name)(owner.handle, None, _ptr(ext)), box_name)
    shape = (int(ext[0]), int(ext[1]))
    n = shape[0] * shape[1]
    dist = name.replace("_ground", "")
    cnt = C.c_size_t(0)
    if device:
        ptr = getattr(L, dist + "_dev")(owner.handle, C.byref(cnt))
        if int(cnt.value) != n:
            raise WsError("ground_distance: another call replaced the result")
        return _device_tensor(ptr, shape, "<i4", owner), int(sites.value)
    rec = np.empty(n, dtype=np.uint32)
    check(getattr(L, dist + "_download")(owner.handle, _ptr(rec), n, C.byref(cnt)), dist + "_download")
    if int(cnt.value) != n:
        raise WsError("ground_distance: another call replaced the result before it was downloaded")
    return rec.reshape(shape), int(sites.value)


class GroundQueries(ReachQueries):
    """TSDFMapping.ground, global_ground and ground_reach, on top of the reach queries whose seeds and clearance they share; uses the
    mapping's params_, mutex_, tsdf_, _max_dist_vox and _window_in_store."""

    def _clear_vox(self, robot_height_m):
        vox = self._max_dist_vox(robot_height_m)
        if not 1 <= vox <= 64:
            raise WsError("ground: the robot's height must be 1 .. 64 voxels")
        return vox

    def ground(self, robot_height_m=1.0, lo=None, hi=None, **kw):
        """The ground layer of the averaged map (DeviceMapMemWrapper.ground on avg_map()), under the mapping's lock like a reader.
        robot_height_m becomes clear_vox by the rule of distance_field (nearest millimetre, then ceil(mm / resolution), 1 .. 64).
        Keywords: any_weight, unknown_headroom, top, device."""
        vox = self._clear_vox(robot_height_m)
        with self.mutex_:
            return self.tsdf_.avg_map().ground(lo=lo, hi=hi, clear_vox=vox, **kw)

    def global_ground(self, robot_height_m=1.0, lo=None, hi=None, **kw):
        """ground() over everything the run has seen: the window goes into the chunks of device_global_map exactly as in global_mesh,
        then DeviceGlobalMap.ground (the box None: the bounding box of the chunks)."""
        if self.device_global_map_ is None:
            raise WsError("global_ground: this TSDFMapping has no device_global_map")
        vox = self._clear_vox(robot_height_m)
        with self._window_in_store("global_ground") as store:
            return store.ground(lo=lo, hi=hi, clear_vox=vox, **kw)

    def ground_reach(self, seeds=None, robot_height_m=1.0, max_step_m=0.1, clearance_m=0.0, pose=None, lo=None, hi=None, unknown_free=False,
                     unknown_occupied=False, unknown_headroom=False, top=False, max_rounds=0, device=False):
        """How far every column of the box (None: the window) is from the robot over ground it can stand and drive on: ground() with the
        robot's height, ground_distance() with the largest step it climbs, then the reach with its clearance -- over ramps and kerbs,
        where reach(columns=True) sees one flat height band.  seeds: (n, 3) map-frame millimetres, or the translation of `pose`.
        Returns the uint32 costs shaped (nx, ny); last_reach keeps seeded, reached, rounds and last_ground the GroundResult's counts."""
        seed_vox = self._reach_seeds(seeds, pose)
        clear_vox = self._clear_vox(robot_height_m)
        vox, clear_d2 = self._clearance(clearance_m)
        step = max_step_q8(float(max_step_m) * 1000.0, self.params_.map.resolution)
        with self.mutex_:
            avg = self.tsdf_.avg_map()
            g = avg.ground(lo=lo, hi=hi, clear_vox=clear_vox, unknown_headroom=unknown_headroom, top=top, device=True)
            self.last_ground = g.counts
            avg.ground_distance(step, max_dist_vox=vox, unknown_occupied=unknown_occupied, device=True)
            cost = avg.reach(seed_vox, clear_d2=clear_d2, unknown_free=unknown_free, max_rounds=max_rounds, device=device)
            self.last_reach = avg.last_reach
            return cost
