"""Synthetic OS1-128 scans of a box room — the workload BASELINE.json's metric is quoted on.

128 rings x 1024 azimuths = 131 072 rays in ring-major order (index = ring*1024 + azimuth); elevation
-22.5deg .. +22.5deg, sensor at `sensor_mm` inside an axis-aligned room with half extents
(10 000, 8 000, 2 500) mm centred on the map origin; range = ray/box intersection plus integer noise
((s >> 8) % 21) - 10 mm from the LCG s <- s*1664525 + 1013904223 (mod 2^32), seed 12345, one draw per ray;
point = trunc(d * dir) per axis, in integer millimetres (the hot path's unit, include/warpsense/consts.h).

Pure numpy; used by bench.py, __graft_entry__.smoke() and the tests.  No reference code involved.
"""
from __future__ import annotations

import numpy as np

RINGS = 128
AZIMUTHS = 1024
HALF_EXTENTS_MM = (10_000.0, 8_000.0, 2_500.0)


def lcg_noise(n: int, seed: int = 12345) -> np.ndarray:
    """((s >> 8) % 21) - 10 for n successive LCG states (uint32 arithmetic)."""
    # s_k = a^k s_0 + c (a^k - 1)/(a - 1) evaluated iteratively in blocks to stay vectorised
    a = np.uint64(1664525)
    c = np.uint64(1013904223)
    mask = np.uint64(0xFFFFFFFF)
    out = np.empty(n, dtype=np.int64)
    s = np.uint64(seed)
    # plain loop in chunks; 131 072 iterations of python are ~50 ms with this jump-ahead trick:
    # precompute (A_j, C_j) for j = 1..B so that s_{k+j} = A_j s_k + C_j
    B = 4096
    A = np.empty(B, dtype=np.uint64)
    C = np.empty(B, dtype=np.uint64)
    aj, cj = np.uint64(1), np.uint64(0)
    for j in range(B):
        aj = (aj * a) & mask
        cj = (cj * a + c) & mask
        A[j], C[j] = aj, cj
    k = 0
    while k < n:
        m = min(B, n - k)
        block = (A[:m] * s + C[:m]) & mask
        out[k:k + m] = ((block >> np.uint64(8)) % np.uint64(21)).astype(np.int64) - 10
        s = block[m - 1]
        k += m
    return out


def os1_128_dirs(rings: int = RINGS, azimuths: int = AZIMUTHS, yaw_rad: float = 0.0) -> np.ndarray:
    """The pattern's (rings*azimuths, 3) float64 unit directions, ring-major."""
    i = np.arange(rings, dtype=np.float64)
    j = np.arange(azimuths, dtype=np.float64)
    el = np.deg2rad(-22.5 + 45.0 * i / max(rings - 1, 1))
    az = 2.0 * np.pi * j / azimuths + yaw_rad
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    ca, sa = np.cos(az)[None, :], np.sin(az)[None, :]
    return np.stack([ce * ca, ce * sa, np.broadcast_to(se, (rings, azimuths))], axis=-1).reshape(-1, 3)


def os1_128_scan(sensor_mm=(0.0, 0.0, 0.0), rings: int = RINGS, azimuths: int = AZIMUTHS, seed: int = 12345,
                 half_extents_mm=HALF_EXTENTS_MM, yaw_rad: float = 0.0) -> np.ndarray:
    """Return an (rings*azimuths, 3) int32 array of points in the MAP frame (mm)."""
    d = os1_128_dirs(rings, azimuths, yaw_rad)
    o = np.asarray(sensor_mm, dtype=np.float64)
    he = np.asarray(half_extents_mm, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_hi = (he - o) / d
        t_lo = (-he - o) / d
    t = np.where(d > 0, t_hi, np.where(d < 0, t_lo, np.inf)).min(axis=1)
    t = t + lcg_noise(rings * azimuths, seed).astype(np.float64)
    pts = o[None, :] + t[:, None] * d
    return np.trunc(pts).astype(np.int32)


def sweep_pose_at(pose_begin, pose_end, s) -> np.ndarray:
    """The sensor pose at the fraction s of a sweep from pose_begin (s = 0) to pose_end (s = 1), in double, with the interpolation
    of ws_sweep_poses (include/warpsense_hip.h): pose_end @ rel(s), the rotation of rel(s) = exp((1 - s) log(R_motion^T)), its
    translation (1 - s) (-R_motion^T t_motion), motion = inv(pose_begin) @ pose_end."""
    B, E = np.asarray(pose_begin, dtype=np.float64), np.asarray(pose_end, dtype=np.float64)
    motion = np.linalg.inv(B) @ E
    Q = motion[:3, :3].T
    u = -Q @ motion[:3, 3]
    v = 0.5 * np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    sn = float(np.linalg.norm(v))
    angle = np.arctan2(sn, 0.5 * (np.trace(Q) - 1.0))
    a = v / sn if sn > 0.0 else np.zeros(3)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    w = 1.0 - float(s)
    rel = np.eye(4)
    rel[:3, :3] = np.eye(3) + np.sin(w * angle) * K + (1.0 - np.cos(w * angle)) * (K @ K)
    rel[:3, 3] = w * u
    return E @ rel


def os1_128_sweep(pose_begin_mm, pose_end_mm, rings: int = RINGS, azimuths: int = AZIMUTHS, half_extents_mm=HALF_EXTENTS_MM, seed: int = 12345,
                  noise: bool = True, with_time: bool = False) -> np.ndarray:
    """One sweep of the pattern taken while the sensor moves from pose_begin_mm to pose_end_mm (4x4, map frame, mm): azimuth column
    j is cast from the pose at s = (j + 0.5) / azimuths (sweep_pose_at).  Returns the cloud as the sensor reports it: (rings *
    azimuths, 3) float32 METRES, every point in the sensor frame of its own column, ring-major; with_time appends s as a fourth
    float.  The range noise is that of os1_128_scan (noise=False: none)."""
    d = os1_128_dirs(rings, azimuths).reshape(rings, azimuths, 3)
    he = np.asarray(half_extents_mm, dtype=np.float64)
    s = (np.arange(azimuths, dtype=np.float64) + 0.5) / azimuths
    T = np.stack([sweep_pose_at(pose_begin_mm, pose_end_mm, sj) for sj in s])  # (azimuths, 4, 4)
    dw = np.einsum("jab,ijb->ija", T[:, :3, :3], d)  # ray directions in the map frame
    o = T[None, :, :3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t_hi = (he - o) / dw
        t_lo = (-he - o) / dw
    t = np.where(dw > 0, t_hi, np.where(dw < 0, t_lo, np.inf)).min(axis=2)
    if noise:
        t = t + lcg_noise(rings * azimuths, seed).astype(np.float64).reshape(rings, azimuths)
    pts = (t[:, :, None] * d / 1000.0).reshape(-1, 3)
    if with_time:
        pts = np.concatenate([pts, np.broadcast_to(s[None, :], (rings, azimuths)).reshape(-1, 1)], axis=1)
    return pts.astype(np.float32)


def perturbation(tx_mm: float = 100.0, ty_mm: float = 100.0, tz_mm: float = 0.0, rz_deg: float = 5.0) -> np.ndarray:
    """The known SE(3) of test/pcd_registration.cpp:30-34 as a 4x4 float32 (row-major numpy) matrix."""
    a = np.deg2rad(rz_deg)
    T = np.eye(4, dtype=np.float64)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    T[:3, 3] = (tx_mm, ty_mm, tz_mm)
    return T.astype(np.float32)


def transform_points_mm(points: np.ndarray, T: np.ndarray) -> np.ndarray:
    """Round-half-away transform of integer mm points (include/util/util.h:80-101 semantics)."""
    p = points.astype(np.float32)
    Tf = T.astype(np.float32)
    q = p @ Tf[:3, :3].T + Tf[:3, 3]
    q = np.where(q < 0, q - np.float32(0.5), q + np.float32(0.5))
    return q.astype(np.int32)
