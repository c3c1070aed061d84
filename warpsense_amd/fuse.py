"""One device-resident global map fused into another under a rigid pose (ws_store_fuse, include/warpsense_hip.h): the pull transform
of a float pose, the statistics of a call, and the call itself behind DeviceGlobalMap.fuse."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._abi import _ptr
from ._lib import check

Q30 = 1 << 30


def fuse_pose(T_src_to_dst, pivot_src_mm=None) -> np.ndarray:
    """The 15 int32 of ws_fuse_pose (rot_q30[9] row-major, pivot_dst_mm[3], pivot_src_mm[3]) for a rigid 4 x 4 float64 transform in
    mm that takes points of the SRC map into the frame of DST: rot_q30 = rint(R^T 2^30), clipped to +-2^30; pivot_src is the given
    point (rounded) or zeros; pivot_dst = rint(R pivot_src + t).  The sub-millimetre remainder of the translation is dropped: the
    pivots are whole millimetres.  Choose pivot_src inside the map: voxels further than 2^24 mm from pivot_dst take no part in a
    fuse.  Raises ValueError on a matrix that is not 4 x 4 or not finite."""
    T = np.asarray(T_src_to_dst, dtype=np.float64)
    if T.shape != (4, 4) or not np.all(np.isfinite(T)):
        raise ValueError("fuse_pose: a finite 4 x 4 matrix is expected")
    R, t = T[:3, :3], T[:3, 3]
    ps = np.zeros(3) if pivot_src_mm is None else np.rint(np.asarray(pivot_src_mm, dtype=np.float64).reshape(3))
    pd = np.rint(R @ ps + t)
    if not (np.all(np.isfinite(ps)) and np.all(np.abs(ps) < 2.0 ** 31) and np.all(np.abs(pd) < 2.0 ** 31)):
        raise ValueError("fuse_pose: a pivot outside int32")
    out = np.empty(15, dtype=np.int32)
    out[:9] = np.clip(np.rint(R.T * Q30), -Q30, Q30).astype(np.int64).reshape(-1)
    out[9:12], out[12:15] = pd.astype(np.int64), ps.astype(np.int64)
    return out


def pose_transform(pose) -> np.ndarray:
    """the 4 x 4 float64 transform SRC -> DST that a ws_fuse_pose stands for (the inverse of fuse_pose up to its rounding)"""
    pose = np.asarray(pose, dtype=np.int64).reshape(15)
    R = (pose[:9].reshape(3, 3).astype(np.float64) / Q30).T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = pose[9:12] - R @ pose[12:15]
    return T


@dataclass(frozen=True)
class FuseStats:
    """stats[6] of ws_store_fuse"""
    candidates: int
    created: int
    averaged: int
    set: int
    sum_abs_diff: int
    sum_min_weight: int

    @property
    def disagreement_mm(self) -> float:
        """the mean |nv - ev| over the averaged voxels: how far the two maps are apart under the pose; nan without any"""
        return self.sum_abs_diff / self.averaged if self.averaged else float("nan")

    def as_tuple(self):
        return (self.candidates, self.created, self.averaged, self.set, self.sum_abs_diff, self.sum_min_weight)


def _fuse_call(L, dst, src, pose, resolution, max_weight, count_only) -> FuseStats:
    pose = np.ascontiguousarray(pose, dtype=np.int32).reshape(15)
    stats = np.zeros(6, dtype=np.uint64)
    flags = _lib.WS_FUSE_COUNT_ONLY if count_only else _lib.WS_FUSE_DEFAULT
    check(L.ws_store_fuse(dst.handle, src.handle, _ptr(pose), int(resolution), int(max_weight), flags, _ptr(stats)), "ws_store_fuse")
    return FuseStats(*(int(v) for v in stats))
