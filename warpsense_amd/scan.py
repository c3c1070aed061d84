"""Scan pre-processing on the device (ws_scan_*, App::preprocess of the reference) and the sweep rules with their host model."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import MATRIX_RESOLUTION, _colmajor, _is_device, _ptr
from ._lib import WsError, check
from .context import Context


class DevicePoints:
    """(n, 3) int32 points resident on the device (what ScanPreprocessor returns); accepted wherever a CUDA
    tensor of points is (TSDFCuda.update_tsdf, RegistrationCuda.prepare_registration)."""

    is_cuda = True

    def __init__(self, ptr: int, n: int, owner):
        self._ptr, self.shape, self._owner = int(ptr), (int(n), 3), owner

    def data_ptr(self) -> int:
        return self._ptr

    def __len__(self):
        return self.shape[0]

    def to_host(self) -> np.ndarray:
        return self._owner.download()


class ScanPreprocessor:
    """App::preprocess on the device (src/warpsense/app.cpp:119-148): sensor cloud in float metres -> distinct
    voxel-centre points in int mm, transformed by the pose, in first-occurrence order."""

    def __init__(self, max_points: int = 128 * 1024, ctx: Context | None = None):
        self.ctx = ctx or Context.default()
        self._L = self.ctx._L
        h = C.c_void_p()
        check(self._L.ws_scan_create(self.ctx.handle, int(max_points), C.byref(h)), "ws_scan_create")
        self.handle = h
        self.n_out = 0

    def preprocess(self, cloud, pose, map_resolution: int) -> DevicePoints:
        """cloud: (n, k >= 3) float32, numpy or CUDA tensor (x y z first); pose: 4x4, translation in mm."""
        n, stride = int(cloud.shape[0]), int(cloud.shape[1])
        T = _colmajor(pose)
        out = C.c_size_t(0)
        if _is_device(cloud):
            check(self._L.ws_scan_preprocess_dev(self.handle, _ptr(cloud), n, stride, _ptr(T), int(map_resolution), C.byref(out)),
                  "ws_scan_preprocess_dev")
        else:
            a = np.ascontiguousarray(cloud, dtype=np.float32)
            check(self._L.ws_scan_preprocess(self.handle, _ptr(a), n, stride, _ptr(T), int(map_resolution), C.byref(out)),
                  "ws_scan_preprocess")
        self.n_out = int(out.value)
        return DevicePoints(self._L.ws_scan_points_dev(self.handle) or 0, self.n_out, self)

    def preprocess_sweep(self, cloud, poses, map_resolution: int, *, columns=None, ring_major: bool = True, time_field=None,
                         t_begin: float = 0.0, t_end: float = 1.0) -> DevicePoints:
        """preprocess with one sensor pose per time bin of the sweep (ws_scan_preprocess_sweep): poses (k, 4, 4), translation in
        mm, e.g. from sweep_poses.  The bin of point i follows its column -- `columns` firing columns (default: k), ring_major
        True for index = ring * columns + column -- or, with time_field, the float at that index of its record between t_begin
        and t_end.  De-duplicated over the whole sweep, first-occurrence order."""
        n, stride = int(cloud.shape[0]), int(cloud.shape[1])
        P = np.asarray(poses, dtype=np.float32)
        if P.ndim != 3 or P.shape[1:] != (4, 4):
            raise ValueError("preprocess_sweep: poses must be (k, 4, 4)")
        k = int(P.shape[0])
        Pc = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1)  # column-major rows of 16
        rule = _sweep_rule(k, columns, ring_major, time_field, t_begin, t_end)
        out = C.c_size_t(0)
        if _is_device(cloud):
            check(self._L.ws_scan_preprocess_sweep_dev(self.handle, _ptr(cloud), n, stride, _ptr(Pc) if k else None, k, C.byref(rule), int(map_resolution),
                                                       C.byref(out)), "ws_scan_preprocess_sweep_dev")
        else:
            a = np.ascontiguousarray(cloud, dtype=np.float32)
            check(self._L.ws_scan_preprocess_sweep(self.handle, _ptr(a), n, stride, _ptr(Pc) if k else None, k, C.byref(rule), int(map_resolution),
                                                   C.byref(out)), "ws_scan_preprocess_sweep")
        self.n_out = int(out.value)
        return DevicePoints(self._L.ws_scan_points_dev(self.handle) or 0, self.n_out, self)

    def download(self) -> np.ndarray:
        pts = np.zeros((max(self.n_out, 1), 3), dtype=np.int32)
        n = C.c_size_t(0)
        check(self._L.ws_scan_download(self.handle, _ptr(pts), pts.shape[0], C.byref(n)), "ws_scan_download")
        return pts[:int(n.value)].copy()

    def close(self):
        if self.handle:
            self._L.ws_scan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def to_int_mat(mat):
    """(mat * MATRIX_RESOLUTION).cast<int>() — include/util/util.h:8-11."""
    return (np.asarray(mat, dtype=np.float32) * np.float32(MATRIX_RESOLUTION)).astype(np.int32)


def _sweep_rule(k, columns, ring_major, time_field, t_begin, t_end) -> _lib.Sweep:
    if time_field is None:
        return _lib.Sweep(int(k if columns is None else columns), int(bool(ring_major)), -1, 0.0, 1.0)
    if int(time_field) < 0:
        raise ValueError("preprocess_sweep: time_field is the index of a float of the point record")
    return _lib.Sweep(0, 0, int(time_field), float(t_begin), float(t_end))


def sweep_poses(pose_end, motion, k: int) -> np.ndarray:
    """The k sensor poses of a sweep (ws_sweep_poses, host code in double; no GPU needed): pose_end is the pose at the end of the
    sweep (4x4, translation in mm), motion the sensor's pose at the end expressed in its frame at the beginning
    (inv(T_begin) @ T_end).  Pose b is the pose at s = (b + 0.5) / k.  Returns (k, 4, 4) float32."""
    k = int(k)
    out = np.zeros((max(k, 1), 16), dtype=np.float32)
    check(_lib.load().ws_sweep_poses(_ptr(_colmajor(pose_end)), _ptr(_colmajor(motion)), max(k, 0), _ptr(out)), "ws_sweep_poses")
    return np.ascontiguousarray(out[:k].reshape(k, 4, 4).transpose(0, 2, 1))


def sweep_bins(n: int, k: int, cloud=None, *, columns=None, ring_major: bool = True, time_field=None, t_begin: float = 0.0, t_end: float = 1.0):
    """The bin of every point of a sweep, as the kernel computes it (include/warpsense_hip.h): (n,) int64, -1 for a point whose
    time gives a NaN.  Raises ValueError for what the library refuses."""
    if not 1 <= int(k) <= _lib.WS_SWEEP_MAX_BINS:
        raise ValueError("sweep: 1 <= k <= 4096 poses")
    if time_field is None:
        columns = int(k if columns is None else columns)
        if columns < 1 or n % columns != 0:
            raise ValueError("sweep: the point count is not a multiple of the columns")
        i = np.arange(n, dtype=np.int64)
        col = i % columns if ring_major else i // max(n // columns, 1)
        return col * int(k) // columns
    a = np.asarray(cloud, dtype=np.float32)
    f = np.float32
    if not 3 <= int(time_field) < a.shape[1]:
        raise ValueError("sweep: time_field must index a float of the record after x y z")
    if not (np.isfinite(f(t_begin)) and np.isfinite(f(t_end))) or f(t_begin) == f(t_end):
        raise ValueError("sweep: t_begin and t_end must be finite and differ")
    with np.errstate(all="ignore"):
        s = (a[:, int(time_field)] - f(t_begin)) / f(f(t_end) - f(t_begin))  # float32, step by step
        v = s * f(k)
        b = np.where(v >= f(k), int(k) - 1, np.where(v > 0, np.minimum(v, f(k)).astype(np.int64), 0))
    return np.where(np.isnan(s), -1, b).astype(np.int64)


def preprocess_sweep_host(cloud, poses, map_resolution: int, *, columns=None, ring_major: bool = True, time_field=None, t_begin: float = 0.0,
                          t_end: float = 1.0) -> np.ndarray:
    """Host model of ScanPreprocessor.preprocess_sweep in plain numpy, the yardstick of its tests: float32 arithmetic step by step,
    wrapping int32 products, truncating division, a first-occurrence set over the whole sweep.  A coordinate beyond +-2^20 mm
    raises WsError (the library's WS_ERR_RANGE)."""
    f = np.float32
    a = np.asarray(cloud, dtype=np.float32)
    P = np.asarray(poses, dtype=np.float32)
    n, res = a.shape[0], int(map_resolution)
    b = sweep_bins(n, P.shape[0], a, columns=columns, ring_major=ring_major, time_field=time_field, t_begin=t_begin, t_end=t_end)
    M = to_int_mat(P).astype(np.int64)  # (k, 4, 4), math layout
    xyz = a[:, :3]
    with np.errstate(all="ignore"):
        keep = np.isfinite(xyz).all(axis=1) & ~(xyz.astype(np.float64) < 0.3).all(axis=1) & (b >= 0)
        idx = np.nonzero(keep)[0]
        p = xyz[idx]
        c = (np.floor((p * f(1000.0)) / f(res)) * f(res) + f(res // 2)).astype(np.int32).astype(np.int64)  # float32 throughout

    def wrap(v):
        return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31

    Mi = M[b[idx]]
    acc = np.zeros((len(idx), 3), dtype=np.int64)
    for j in range(3):
        acc = wrap(acc + wrap(Mi[:, :3, j] * c[:, j:j + 1]))
    acc = wrap(acc + Mi[:, :3, 3])
    q = np.sign(acc) * (np.abs(acc) // MATRIX_RESOLUTION)  # C division truncates toward zero
    if np.any(np.abs(q) >= 2 ** 20):
        raise WsError("preprocess_sweep_host: a transformed coordinate is beyond +-2^20 mm")
    _, first = np.unique(q, axis=0, return_index=True)
    return q[np.sort(first)].astype(np.int32).reshape(-1, 3)


def to_map(pose, map_resolution: int):
    """floor(translation / resolution) in float — include/util/util.h:52-56."""
    t = np.asarray(pose, dtype=np.float32)[:3, 3]
    return np.floor(t / np.float32(map_resolution)).astype(np.int32)
