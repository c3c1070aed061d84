"""The model of ws_map_clearance / ws_store_clearance (rules stated in include/warpsense_hip.h) in per-sample loops of Python integers
over the records of distance_model.py, and the scenes of its tests.  No GPU and no built library at import."""
import math

import numpy as np

RECORD = np.dtype([("min_margin", "<i4"), ("first_hit", "<i4"), ("argmin", "<u4"), ("hits", "<u4"), ("outside", "<u4"), ("unknown", "<u4"), ("cost", "<u8")])
POSE = np.dtype([("min_margin", "<i4"), ("hits", "<u2"), ("outside", "<u2")])
NONE = 0x7FFFFFFF
Q30 = 1 << 30


def centre(pose, off, a):
    """pos_a + floor((sum_j rot[a][j] off_j + 2^29) / 2^30); Python's // is the floor division"""
    s = sum(int(pose[3 * a + j]) * int(off[j]) for j in range(3))
    return int(pose[9 + a]) + (s + (1 << 29)) // Q30


def voxel(pose, off, res):
    return tuple(centre(pose, off, a) // int(res) for a in range(3))


def centres(poses, body, res):
    """the voxels of all samples: (n, k, 3) int64 for (n, 12) poses"""
    poses, body = np.asarray(poses).reshape(-1, 12), np.asarray(body).reshape(-1, 4)
    return np.array([[voxel(p, b[:3], res) for b in body] for p in poses], dtype=np.int64).reshape(len(poses), len(body), 3)


def margin(d2, res, radius):
    return math.isqrt(int(d2) * int(res) * int(res)) - int(radius)


def sample(rec, lo, columns, v):
    """the record at world voxel v, None OUTSIDE"""
    idx = tuple(int(v[a]) - int(lo[a]) for a in range(2 if columns else 3))
    if any(i < 0 or i >= n for i, n in zip(idx, rec.shape)):
        return None
    return int(rec[idx])


def score(rec, lo, columns, res, poses, body, soft, outside_ok=False):
    """(RECORD [T], POSE [T, P], best) for poses (T, P, 12) and body (K, 4) over the distance records `rec` whose first voxel is lo"""
    poses, body = np.asarray(poses), np.asarray(body).reshape(-1, 4)
    T, P = poses.shape[:2]
    out, per_pose = np.zeros(T, dtype=RECORD), np.zeros((T, P), dtype=POSE)
    best = (None, -1)
    for t in range(T):
        mn, arg, first, hits, outside, unknown, cost = NONE, 0xFFFFFFFF, -1, 0, 0, 0, 0
        any_inside = False
        for p in range(P):
            pm, ph, po, p_inside = NONE, 0, 0, False
            for k, b in enumerate(body):
                r = sample(rec, lo, columns, voxel(poses[t, p], b[:3], res))
                if r is None:
                    outside, po = outside + 1, po + 1
                    continue
                m = margin(r & 0xFFFFFF, res, b[3])
                if not any_inside or m < mn:
                    mn, arg, any_inside = m, p * 64 + k, True
                if not p_inside or m < pm:
                    pm, p_inside = m, True
                if m < 0:
                    hits, ph = hits + 1, ph + 1
                    first = p if first < 0 else first
                if (r >> 30) == 0:
                    unknown += 1
                cost += max(0, int(soft) - m) ** 2
            per_pose[t, p] = (pm, ph, po)
        out[t] = (mn, first, arg, hits, outside, unknown, cost)
        if hits == 0 and (outside_ok or outside == 0) and (best[0] is None or cost < best[0]):
            best = (cost, t)
    return out, per_pose, best[1]


# ------------------------------------------------------------------------------------------------ scenes
def rotation_q30(rng, kind):
    """a rotation as rot_q30: 'generic' a random orthonormal matrix, 'quarter' a signed permutation (quarter turns), 'yaw' about z"""
    if kind == "quarter":
        m = np.zeros((3, 3))
        for r, c in enumerate(rng.permutation(3)):
            m[r, c] = rng.choice([-1.0, 1.0])
    elif kind == "yaw":
        a = rng.uniform(-np.pi, np.pi)
        m = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    else:
        m, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return np.clip(np.rint(m * Q30), -Q30, Q30).astype(np.int64).reshape(9)


def draw_body(rng, k, res, max_radius):
    """k spheres within about two voxels of the body's origin, radii up to max_radius mm, the first at the origin"""
    body = np.zeros((k, 4), dtype=np.int32)
    body[:, :3] = rng.integers(-2 * res, 2 * res + 1, size=(k, 3))
    body[0, :3] = 0
    body[:, 3] = rng.integers(0, max_radius + 1, size=k)
    return body


def draw_poses(rng, T, P, lo, ext, res, walk_vox=1.5):
    """T trajectories of P poses: a random walk of about walk_vox voxels per pose from a start inside the box [lo, lo + ext) (world
    voxels; negative coordinates where the box has them).  Every fourth trajectory turns by quarter turns, the rest generically.  Then
    planted on trajectory 0, with the identity as rotation: its last pose is the last millimetre of the voxel one beyond the lo corner
    on every axis and the pose before it the first millimetre of the lo corner's voxel; with P >= 4 the two poses before those are
    the last millimetre of the hi corner's voxel and the first of the voxel beyond it.  With T >= 3 the last trajectory lies wholly
    outside the box."""
    lo, ext = np.asarray(lo, dtype=np.int64), np.asarray(ext, dtype=np.int64)
    poses = np.zeros((T, P, 12), dtype=np.int64)
    for t in range(T):
        pos = (lo + rng.uniform(0.1, 0.9, size=3) * ext) * res
        for p in range(P):
            poses[t, p, :9] = rotation_q30(rng, "quarter" if t % 4 == 3 else "generic")
            poses[t, p, 9:] = np.rint(pos)
            pos = pos + rng.normal(scale=walk_vox * res, size=3)
    ident = np.array([Q30, 0, 0, 0, Q30, 0, 0, 0, Q30], dtype=np.int64)
    hi = lo + ext - 1
    planted = ([lo * res - 1] if P >= 2 else []) + [lo * res] + ([(hi + 1) * res, hi * res + (res - 1)] if P >= 4 else [])
    for i, at in enumerate(planted[:P]):
        poses[0, P - 1 - i, :9] = ident
        poses[0, P - 1 - i, 9:] = at
    if T >= 3:
        poses[T - 1, :, 9:] += (ext + 5) * res  # wholly outside, beyond the hi faces (x and y count under columns)
    return poses.astype(np.int32)


def conditions(records, best, T):
    """on the MODEL, before the device is asked: a scene in which nothing or everything collides cannot pass"""
    share = float(np.count_nonzero(records["hits"])) / T
    assert 0.2 <= share <= 0.8, share
    assert np.any(records["outside"] > 0) and np.any(records["unknown"] > 0)
    assert np.any((records["hits"] > 0) | (records["outside"] > 0)) and best >= 0, best
