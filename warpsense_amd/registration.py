"""Point-to-TSDF registration on the device (ws_reg_*): RegistrationCuda, and the ranking and the pose lattice of a batch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import _colmajor, _is_device, _ptr
from ._lib import WS_REG_ALL_POINTS, check
from .context import Context
from .device_map import DeviceMap


class RegistrationCuda:
    """cuda::RegistrationCuda (registration.h:10-45, registration.cu:259-368)."""

    def __init__(self, map_: DeviceMap | None = None, ctx: Context | None = None, flags: int = WS_REG_ALL_POINTS):
        self.ctx = ctx or Context.default()
        self._L = self.ctx._L
        self.flags = int(flags)
        h = C.c_void_p()
        check(self._L.ws_reg_create(self.ctx.handle, 128 * 1024, C.byref(h)), "ws_reg_create")
        self.handle = h
        self.curr_n_points = 0

    def prepare_registration(self, points):
        n = int(points.shape[0])
        self.curr_n_points = n
        if _is_device(points):
            # (an asynchronous device-to-device copy on the context's stream: like TSDFCuda.update_tsdf, keep the tensor away from
            # torch's allocator until the next cloud's copy has been enqueued behind it)
            prev = getattr(self, "_cloud_in_flight", None)
            check(self._L.ws_reg_prepare_dev(self.handle, _ptr(points), n), "ws_reg_prepare_dev")
            self._cloud_in_flight = points
            del prev
        else:
            pts = np.ascontiguousarray(points, dtype=np.int32)
            check(self._L.ws_reg_prepare(self.handle, _ptr(pts), n), "ws_reg_prepare")

    def perform_registration(self, map_dev, pretransform, map_resolution: int):
        """Returns (h 6x6 int64 math layout, g[6] int64, e, c) — the out-parameters of the reference."""
        T = _colmajor(pretransform)
        h = np.zeros(36, dtype=np.int64)
        g = np.zeros(6, dtype=np.int64)
        e, c = C.c_int32(0), C.c_int32(0)
        check(self._L.ws_reg_iterate(self.handle, map_dev, _ptr(T), int(map_resolution), self.flags, _ptr(h), _ptr(g),
                                     C.byref(e), C.byref(c)), "ws_reg_iterate")
        return h.reshape(6, 6).T.copy(), g, e.value, c.value

    def register_cloud(self, map_dev, pretransform, max_iterations, it_weight_gradient, epsilon, map_resolution):
        # (two ctypes buffers kept for the life of the object: numpy's .ctypes costs 3 us per array, and this call sits in the gap
        # between the end of one registration and the first kernel of the next update)
        buf = getattr(self, "_rc_buf", None)
        if buf is None:
            buf = self._rc_buf = ((C.c_float * 16)(), (C.c_float * 16)(), C.c_int32(0))
        T_c, out_c, it = buf
        T_c[:] = np.asarray(pretransform, dtype=np.float32).reshape(4, 4).T.reshape(16).tolist()
        check(self._L.ws_register_cloud(self.handle, map_dev, T_c, int(max_iterations), C.c_float(it_weight_gradient),
                                        C.c_float(epsilon), int(map_resolution), self.flags, out_c, C.byref(it)),
              "ws_register_cloud")
        return np.array(out_c, dtype=np.float32).reshape(4, 4).T.copy(), it.value

    def register_cloud_batch(self, map_dev, poses, max_iterations, it_weight_gradient, epsilon, map_resolution):
        """K registrations of the prepared cloud, one per start pose, in one launch (ws_register_cloud_batch).
        poses: (k, 4, 4).  Returns (T[k, 4, 4] float32, iterations[k], e[k], c[k]): pose k and its iteration count are what
        register_cloud returns from poses[k] alone; e[k], c[k] are perform_registration's e and c at T[k]."""
        P = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
        k = int(P.shape[0])
        T_in = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(k, 16)
        T_out = np.zeros((k, 16), dtype=np.float32)
        it, e, c = (np.zeros(k, dtype=np.int32) for _ in range(3))
        check(self._L.ws_register_cloud_batch(self.handle, map_dev, _ptr(T_in), k, int(max_iterations), C.c_float(it_weight_gradient),
                                              C.c_float(epsilon), int(map_resolution), self.flags, _ptr(T_out), _ptr(it), _ptr(e), _ptr(c)),
              "ws_register_cloud_batch")
        return np.ascontiguousarray(T_out.reshape(k, 4, 4).transpose(0, 2, 1)), it, e, c

    def last_sums(self):
        """(h 6x6 int64, g[6], e, c) the last Gauss-Newton update of the last register_cloud was made from (test entry)"""
        out = np.empty(44, dtype=np.int64)
        check(self._L.ws_debug_reg_sums(self.handle, _ptr(out)), "ws_debug_reg_sums")
        return out[:36].reshape(6, 6).T.copy(), out[36:42].copy(), int(out[42]), int(out[43])

    def set_loop(self, mode: int):
        """WS_REG_LOOP_RESIDENT (one launch, grid barrier; default) or WS_REG_LOOP_LAUNCHES (one launch per iteration)."""
        check(self._L.ws_reg_set_loop(self.handle, int(mode)), "ws_reg_set_loop")

    def close(self):
        if self.handle:
            self._L.ws_reg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def batch_best(e, c, min_count: int = 1) -> int:
    """Index of the best hypothesis of a batch (ws_reg_batch_best): among those with c[i] >= min_count the smallest mean error
    e[i] / c[i], compared exactly; ties: larger c, then lower index.  -1 if none qualifies."""
    e = np.ascontiguousarray(e, dtype=np.int32).reshape(-1)
    c = np.ascontiguousarray(c, dtype=np.int32).reshape(-1)
    if e.shape != c.shape:
        raise ValueError("batch_best: e and c differ in length")
    best = C.c_int64(-1)
    check(_lib.load().ws_reg_batch_best(_ptr(e), _ptr(c), int(e.shape[0]), int(min_count), C.byref(best)), "ws_reg_batch_best")
    return int(best.value)


def candidate_poses(guess, radius_m: float, step_m: float, yaw_range_deg: float = 0.0, yaw_step_deg: float = 0.0) -> np.ndarray:
    """The local pose lattice of TSDFRegistration.relocalize around `guess` (4x4, translation in mm): (n, 4, 4) float32.

    x and y offsets i * step_m, |i| <= floor(radius_m / step_m), on a square grid in the map frame; yaw offsets j * yaw_step_deg,
    |j| <= floor(yaw_range_deg / yaw_step_deg), about the map's z axis through the guess's own position (the rotation is
    multiplied from the left, the translation keeps its place).  A step <= 0 leaves that axis at the guess.  Candidate 0 is the
    guess itself, unchanged; the others follow row-major (x slowest, then y, yaw fastest, each from its most negative offset
    upwards) without the node of all-zero offsets, whose place the guess has taken: (2 nx + 1)(2 ny + 1)(2 nyaw + 1) poses.
    Computed in float64, rounded once to float32."""
    G = np.asarray(guess, dtype=np.float64).reshape(4, 4)
    n_xy = int(np.floor(radius_m / step_m + 1e-9)) if step_m > 0 and radius_m > 0 else 0
    n_yaw = int(np.floor(yaw_range_deg / yaw_step_deg + 1e-9)) if yaw_step_deg > 0 and yaw_range_deg > 0 else 0
    out = [G.copy()]
    for ix in range(-n_xy, n_xy + 1):
        for iy in range(-n_xy, n_xy + 1):
            for iw in range(-n_yaw, n_yaw + 1):
                if ix == 0 and iy == 0 and iw == 0:
                    continue
                a = np.deg2rad(iw * float(yaw_step_deg))
                Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
                Tc = G.copy()
                Tc[:3, :3] = Rz @ G[:3, :3]
                Tc[0, 3] = G[0, 3] + ix * float(step_m) * 1000.0
                Tc[1, 3] = G[1, 3] + iy * float(step_m) * 1000.0
                out.append(Tc)
    return np.stack(out).astype(np.float32)
