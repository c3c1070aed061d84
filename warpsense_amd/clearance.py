"""Clearance of candidate trajectories against the distance field (ws_map_clearance, ws_store_clearance; the rules are stated in
include/warpsense_hip.h): the body, the poses and the rollouts a caller hands over, the call shared by the window and the store, its
result, and the two methods of TSDFMapping (mapping.py mixes them in)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import _device_tensor, _is_device, _ptr
from ._lib import WsError, check

# one record of ws_map_clearance per trajectory (32 bytes), and with WS_CLEARANCE_POSES one per (trajectory, pose), trajectory-major
CLEARANCE_RECORD = np.dtype([("min_margin", "<i4"), ("first_hit", "<i4"), ("argmin", "<u4"), ("hits", "<u4"), ("outside", "<u4"), ("unknown", "<u4"),
                             ("cost", "<u8")])
CLEARANCE_POSE = np.dtype([("min_margin", "<i4"), ("hits", "<u2"), ("outside", "<u2")])
CLEARANCE_NONE = 0x7FFFFFFF  # the margin of a trajectory or pose without a sample inside the box


def body_spheres(offsets_m, radii_m) -> np.ndarray:
    """The body of a clearance call: (k, 3) sphere centres in the body frame and k radii (or one for all), in metres, as the (k, 4)
    int32 of the C call (off_mm[3], radius_mm), rounded to nearest."""
    off = np.asarray(offsets_m, dtype=np.float64).reshape(-1, 3)
    rad = np.broadcast_to(np.asarray(radii_m, dtype=np.float64).reshape(-1), (len(off),))
    if not 1 <= len(off) <= 64:
        raise WsError("body_spheres: a body has 1 .. 64 spheres")
    out = np.concatenate([np.rint(off * 1000.0), np.rint(rad * 1000.0)[:, None]], axis=1)
    if np.any(np.abs(out[:, :3]) > 2 ** 20) or np.any(out[:, 3] < 0) or np.any(out[:, 3] > 65535):
        raise WsError("body_spheres: an offset exceeds 2^20 mm or a radius leaves 0 .. 65535 mm")
    return np.ascontiguousarray(out.astype(np.int32))


def trajectory_poses(poses, rows=None) -> np.ndarray:
    """The pose records of a clearance call from (..., 4, 4) float matrices (body to map frame, translation in metres) or from
    (..., 4) rows (x, y, z in metres, yaw in radians): (..., 12) int32, rot_q30 = rint(R 2^30) row-major clipped to +-2^30, then
    pos_mm = rint(t 1000).  A (T, P, ...) input gives the (T, P, 12) array of the call.  rows: True for rows, False for matrices, None
    to tell by the shape (a trailing (4, 4) is taken for matrices: say rows=True for trajectories of four rows)."""
    a = np.asarray(poses, dtype=np.float64)
    if rows is not True and a.ndim >= 2 and a.shape[-2:] == (4, 4):
        rot, t = a[..., :3, :3], a[..., :3, 3]
    elif rows is not False and a.ndim >= 1 and a.shape[-1] == 4:
        c, s, z, o = np.cos(a[..., 3]), np.sin(a[..., 3]), np.zeros(a.shape[:-1]), np.ones(a.shape[:-1])
        rot = np.stack([np.stack([c, -s, z], axis=-1), np.stack([s, c, z], axis=-1), np.stack([z, z, o], axis=-1)], axis=-2)
        t = a[..., :3]
    else:
        raise WsError("trajectory_poses: give (..., 4, 4) matrices or (..., 4) rows of x, y, z, yaw")
    q = np.clip(np.rint(rot * float(1 << 30)), -(1 << 30), 1 << 30).reshape(rot.shape[:-2] + (9,))
    mm = np.rint(t * 1000.0)
    if np.any(np.abs(mm) >= 2 ** 30):
        raise WsError("trajectory_poses: a position leaves +-2^30 mm")
    return np.ascontiguousarray(np.concatenate([q, mm], axis=-1).astype(np.int32))


def arc_rollouts(pose, speeds, yaw_rates, steps, dt) -> np.ndarray:
    """A fan of constant-curvature rollouts from `pose` (a 4 x 4 float matrix, metres, or (x, y, z, yaw)): for every pair of a speed
    (m/s) and a yaw rate (rad/s), speed-major, `steps` poses at times dt, 2 dt, ... in the plane of the start pose's yaw.  Returns
    the (len(speeds) * len(yaw_rates), steps, 12) int32 records of the call (trajectory_poses of the rows x, y, z, yaw)."""
    p = np.asarray(pose, dtype=np.float64)
    if p.shape == (4, 4):
        x0, y0, z0, th0 = p[0, 3], p[1, 3], p[2, 3], np.arctan2(p[1, 0], p[0, 0])
    else:
        x0, y0, z0, th0 = p.reshape(4)
    v = np.asarray(speeds, dtype=np.float64).reshape(-1)
    w = np.asarray(yaw_rates, dtype=np.float64).reshape(-1)
    steps = int(steps)
    if steps < 1 or len(v) < 1 or len(w) < 1:
        raise WsError("arc_rollouts: at least one speed, one yaw rate and one step")
    vv, ww = [g.reshape(-1, 1) for g in np.meshgrid(v, w, indexing="ij")]
    t = (np.arange(1, steps + 1, dtype=np.float64) * float(dt))[None, :]
    th = th0 + ww * t
    straight = np.abs(ww) < 1e-9
    wsafe = np.where(straight, 1.0, ww)
    x = np.where(straight, x0 + vv * t * np.cos(th0), x0 + vv / wsafe * (np.sin(th) - np.sin(th0)))
    y = np.where(straight, y0 + vv * t * np.sin(th0), y0 - vv / wsafe * (np.cos(th) - np.cos(th0)))
    return trajectory_poses(np.stack([x, y, np.full_like(x, z0), th], axis=-1), rows=True)


class ClearanceResult:
    """What a clearance call returns: `records` (CLEARANCE_RECORD per trajectory), `poses` ((T, P) CLEARANCE_POSE, or None without
    per_pose) and `best` (the index of the trajectory without a hit -- and without an outside sample unless outside_ok -- whose
    (cost, index) is smallest, -1 for none).  With device=True the two arrays are torch int32 tensors (T, 8) and (T, P, 2) that ALIAS
    the library's buffers until the next clearance call on the same owner."""

    def __init__(self, records, poses, best):
        self.records, self.poses, self.best = records, poses, int(best)

    def collision_free(self):
        """the indices of the trajectories without a hit (host records)"""
        return np.flatnonzero(self.records["hits"] == 0)

    def __repr__(self):
        return f"ClearanceResult(trajectories={len(self.records)}, best={self.best})"


def _clearance_call(L, name, owner, poses, body, soft_mm, tail, per_pose, outside_ok, device):
    """The clearance call `name` (ws_map_clearance, ws_store_clearance) on owner.handle: `poses` a (T, P, 12) int32 numpy array or
    CUDA tensor (the _dev form), `body` (k, 4) int32, `tail` the arguments between soft_mm and the flags.  No trajectory: an empty
    result, nothing is called."""
    on_device = _is_device(poses)
    if on_device:
        if poses.dim() != 3 or poses.shape[2] != 12 or str(poses.dtype) != "torch.int32" or not poses.is_contiguous():
            raise WsError("clearance: device poses must be a contiguous (T, P, 12) int32 tensor")
    else:
        poses = np.ascontiguousarray(poses, dtype=np.int32)
        if poses.ndim != 3 or poses.shape[2] != 12:
            raise WsError("clearance: poses must be (T, P, 12) int32 (trajectory_poses makes them)")
    t, p = int(poses.shape[0]), int(poses.shape[1])
    b = np.ascontiguousarray(body, dtype=np.int32).reshape(-1, 4)
    if t == 0:
        return ClearanceResult(np.zeros(0, dtype=CLEARANCE_RECORD), np.zeros((0, p), dtype=CLEARANCE_POSE) if per_pose else None, -1)
    flags = (_lib.WS_CLEARANCE_POSES if per_pose else 0) | (_lib.WS_CLEARANCE_OUTSIDE_OK if outside_ok else 0)
    best = C.c_int64(-1)
    entry = name + "_dev" if on_device else name
    check(getattr(L, entry)(owner.handle, _ptr(poses), t, p, _ptr(b), len(b), int(soft_mm), *tail, flags, C.byref(best)), entry)
    cnt = C.c_size_t(0)
    if device:
        rec = _device_tensor(getattr(L, name + "_records_dev")(owner.handle, C.byref(cnt)), (t, 8), "<i4", owner)
        if int(cnt.value) != t:
            raise WsError("clearance: another call replaced the result")
        pr = _device_tensor(getattr(L, name + "_poses_dev")(owner.handle, C.byref(cnt)), (t, p, 2), "<i4", owner) if per_pose else None
        return ClearanceResult(rec, pr, best.value)
    rec = np.empty(t, dtype=CLEARANCE_RECORD)
    pr = np.empty((t, p), dtype=CLEARANCE_POSE) if per_pose else None
    got, got_p = C.c_size_t(0), C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), _ptr(pr), t, t * p if per_pose else 0, C.byref(got), C.byref(got_p)), name + "_download")
    if int(got.value) != t or (per_pose and int(got_p.value) != t * p):
        raise WsError("clearance: another call replaced the result before it was downloaded")
    return ClearanceResult(rec, pr, best.value)


def clearance_centres(poses, body, resolution) -> np.ndarray:
    """ws_clearance_centres (host only): the voxel of every sample, (..., k, 3) int32 for (..., 12) poses and a (k, 4) body"""
    L = _lib.load()
    ps = np.ascontiguousarray(poses, dtype=np.int32)
    flat = ps.reshape(-1, 12)
    b = np.ascontiguousarray(body, dtype=np.int32).reshape(-1, 4)
    out = np.zeros((len(flat), len(b), 3), dtype=np.int32)
    check(L.ws_clearance_centres(_ptr(flat), len(flat), _ptr(b), len(b), int(resolution), _ptr(out)), "ws_clearance_centres")
    return out.reshape(ps.shape[:-1] + (len(b), 3))


def clearance_margin(d2, resolution, radius_mm) -> int:
    """ws_clearance_margin (host only): isqrt(d2 res^2) - radius_mm"""
    return int(_lib.load().ws_clearance_margin(int(d2), int(resolution), int(radius_mm)))


class ClearanceQueries:
    """TSDFMapping.score_trajectories and global_score_trajectories; uses the mapping's params_, mutex_, tsdf_ and _window_in_store."""

    def score_trajectories(self, poses, body, soft_m=0.0, max_dist_m=None, columns=True, lo=None, hi=None, unknown_occupied=False, refresh=True, **kw):
        """Score candidate trajectories against the averaged map: a distance() call over the window (columns: the 2-D field of a ground
        robot; refresh=False: reuse the last distance result, whoever made it, e.g. ground_distance) and DeviceMapMemWrapper.clearance
        on it, under the mapping's lock like a reader.  poses: (T, P, 12) int32 (trajectory_poses) or what trajectory_poses takes;
        body: (k, 4) int32 (body_spheres).  max_dist_m: the clamp of the distance call (None: the largest radius + soft_m, plus a
        voxel).  Keywords: per_pose, outside_ok, device.  Returns a ClearanceResult."""
        ps, b, soft_mm = _score_args(poses, body, soft_m)
        with self.mutex_:
            avg = self.tsdf_.avg_map()
            if refresh:
                avg.distance(lo=lo, hi=hi, max_dist_vox=_score_range(self, b, soft_mm, max_dist_m), unknown_occupied=unknown_occupied, columns=columns, device=True)
            out = avg.clearance(ps, b, soft_mm, **kw)
            self.last_clearance = out
            return out

    def global_score_trajectories(self, poses, body, soft_m=0.0, max_dist_m=None, columns=True, lo=None, hi=None, unknown_occupied=False, refresh=True, **kw):
        """score_trajectories() through everything the run has seen: the window goes into the chunks of device_global_map exactly as in
        global_mesh, then DeviceGlobalMap.distance and .clearance at the map's resolution (the box None: the bounding box of the chunks)."""
        if self.device_global_map_ is None:
            raise WsError("global_score_trajectories: this TSDFMapping has no device_global_map")
        ps, b, soft_mm = _score_args(poses, body, soft_m)
        with self._window_in_store("global_score_trajectories") as store:
            if refresh:
                store.distance(lo=lo, hi=hi, max_dist_vox=_score_range(self, b, soft_mm, max_dist_m), unknown_occupied=unknown_occupied, columns=columns, device=True)
            out = store.clearance(int(self.params_.map.resolution), ps, b, soft_mm, **kw)
            self.last_clearance = out
            return out


def _score_args(poses, body, soft_m):
    ps = poses if _is_device(poses) or (isinstance(poses, np.ndarray) and poses.dtype == np.int32 and poses.shape[-1] == 12) else trajectory_poses(poses)
    return ps, np.ascontiguousarray(body, dtype=np.int32).reshape(-1, 4), int(np.rint(float(soft_m) * 1000.0))


def _score_range(mapping, body, soft_mm, max_dist_m):
    res = int(mapping.params_.map.resolution)
    need = (int(body[:, 3].max()) + soft_mm) if max_dist_m is None else int(np.rint(float(max_dist_m) * 1000.0))
    vox = -(-need // res) + (1 if max_dist_m is None else 0)
    if not 1 <= vox <= 255:
        raise WsError("score_trajectories: the distance range must be 1 .. 255 voxels (largest radius + soft_m, or max_dist_m)")
    return vox
