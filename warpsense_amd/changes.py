"""Change detection between two device-resident global maps (ws_store_changes, include/warpsense_hip.h): the statistics and the result
of a call, the call itself behind DeviceGlobalMap.changes, and the PLY of a result."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._abi import _ptr
from ._lib import WsError, check
from .queries import _box_ptrs
from .records import FRONTIER_CLUSTER

CHANGE_RECORD = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("ref_value", "<i2"), ("kind", "<u2")])
assert CHANGE_RECORD.itemsize == 16
APPEARED, VANISHED = 1, 2
_KINDS = {"both": _lib.WS_CHANGES_DEFAULT, "appeared": _lib.WS_CHANGES_APPEARED, "vanished": _lib.WS_CHANGES_VANISHED}


@dataclass(frozen=True)
class ChangeStats:
    """stats[6] of ws_store_changes; they cover both kinds whatever the call selected"""
    chunks: int
    known_both: int
    appeared: int
    vanished: int
    new_ground: int
    sum_abs_diff: int

    def changed_volume_m3(self, resolution) -> float:
        """the volume of the appeared and vanished voxels, in cubic metres"""
        return (self.appeared + self.vanished) * (float(resolution) / 1000.0) ** 3

    @property
    def disagreement_mm(self) -> float:
        """the mean |nv - ev| over the voxels known on both sides; nan without any"""
        return self.sum_abs_diff / self.known_both if self.known_both else float("nan")

    def as_tuple(self):
        return (self.chunks, self.known_both, self.appeared, self.vanished, self.new_ground, self.sum_abs_diff)


@dataclass(frozen=True)
class ChangeResult:
    """What DeviceGlobalMap.changes returns: `records` (CHANGE_RECORD [n]: x, y, z in world voxels of the current map, the value the
    reference map holds there, the kind: 1 appeared, 2 vanished) in ascending world (x, y, z); with clusters=True `labels` (uint32
    [n]) and `clusters` (FRONTIER_CLUSTER [k]: first, count, lo, hi, sum), else None; and the ChangeStats."""
    records: np.ndarray
    labels: np.ndarray | None
    clusters: np.ndarray | None
    stats: ChangeStats

    @property
    def kinds(self) -> np.ndarray:
        return self.records["kind"]

    @property
    def ref_values(self) -> np.ndarray:
        return self.records["ref_value"]

    def cluster_kinds(self) -> np.ndarray:
        """per cluster the kinds it holds as bits: 1 appeared, 2 vanished, 3 both (a moved object whose places touch)"""
        out = np.zeros(0 if self.clusters is None else len(self.clusters), dtype=np.uint8)
        if len(out):
            np.bitwise_or.at(out, self.labels, self.records["kind"].astype(np.uint8))
        return out


def _changes_call(L, cur, ref, pose, resolution, lo, hi, band, free_value, min_weight, kinds, clusters) -> ChangeResult:
    if kinds not in _KINDS:
        raise WsError("changes: kinds is 'both', 'appeared' or 'vanished'")
    box = _box_ptrs("changes", lo, hi)
    pose = np.ascontiguousarray(pose, dtype=np.int32).reshape(15)
    stats = np.zeros(6, dtype=np.uint64)
    n, k = C.c_size_t(0), C.c_size_t(0)
    flags = _KINDS[kinds] | (_lib.WS_CHANGES_CLUSTERS if clusters else 0)
    check(L.ws_store_changes(cur.handle, ref.handle, _ptr(pose), int(resolution), *box, int(band), int(free_value), int(min_weight), flags, C.byref(n), C.byref(k),
                             _ptr(stats)), "ws_store_changes")
    n, k = int(n.value), int(k.value)
    rec = np.empty(n, dtype=CHANGE_RECORD)
    labels = np.empty(n, dtype=np.uint32) if clusters else None
    table = np.empty(k, dtype=FRONTIER_CLUSTER) if clusters else None
    got, got_k = C.c_size_t(0), C.c_size_t(0)
    check(L.ws_store_changes_download(cur.handle, _ptr(rec), _ptr(labels), _ptr(table), n, k, C.byref(got), C.byref(got_k)), "ws_store_changes_download")
    if int(got.value) != n or (clusters and int(got_k.value) != k):
        raise WsError("changes: another call replaced the result before it was downloaded")
    return ChangeResult(rec, labels, table, ChangeStats(*(int(v) for v in stats)))


def write_changes_ply(path, result: ChangeResult, resolution):
    """the records of a ChangeResult as an ASCII PLY point cloud in metres, voxel centres: appeared green, vanished red"""
    rec = result.records
    xyz = (np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64) + 0.5) * float(resolution) / 1000.0
    colour = np.where((rec["kind"] == APPEARED)[:, None], np.array([40, 200, 60]), np.array([220, 50, 40]))
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(rec))
        f.write("property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        for p, c in zip(xyz, colour):
            f.write("%.4f %.4f %.4f %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))
