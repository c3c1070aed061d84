"""The scenes of the fuse's domain tests (test_fuse_domain_host.py on the model, test_gpu_fuse_domain.py on the device): random rigid
poses, and the edges of the call's position and value domain.  A scene is a dictionary: name, dst, src (chunks), pose, res, mw, and
optionally count_only, must (DST voxels that have to receive a sample), must_not with why ("dead": a component of q of magnitude
>= 2^30; "outside": a component of |p - pivot_dst| >= 2^24) and covered (all eight corners of every must_not voxel's cell are
observed voxels of SRC, so nothing but the stated reason keeps the voxel from receiving), nothing (no voxel receives), and
keys_created.  Every scene's expectation is fuse_model.fuse_at over fuse_model.receivers: voxel by voxel, without the chunk plan.

Random poses, seeds 0 .. 23 (RANDOM_SEEDS), as test_fuse_domain_host.py asserts and measured there: 24 of 24 cases set a voxel, 24
receive into 4 or more DST chunks, 22 have a receiving DST chunk with fewer than 8 receiving voxels, 24 average a voxel."""
import numpy as np

import fuse_model as F
import fuse_scenes as S
from edge_domain_scenes import BOTTOM_KEY, TOP_KEY
from fuse_scenes import FILL, MW, TAU

Q30, REACH = F.Q30, F.REACH
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
RANDOM_SEEDS = tuple(range(24))
RANDOM_RES = (1, 7, 64, 1000)
IDENTITY = (Q30, 0, 0, 0, Q30, 0, 0, 0, Q30)
QUARTER_Z = (0, Q30, 0, -Q30, 0, 0, 0, 0, Q30)  # the pull of a map turned by 90 degrees about z


def make_pose(rot, pd=(0, 0, 0), ps=(0, 0, 0)):
    return np.array([*rot, *pd, *ps], dtype=np.int64).astype(np.int32)


def general_rot(yaw=17.0, pitch=3.0, roll=0.0):
    return tuple(int(v) for v in np.clip(np.rint(S.rot(yaw, pitch, roll)[:3, :3].T * Q30), -Q30, Q30).reshape(-1))


def sparse_chunk(rng):
    """2^3 blocks of observed voxels at the corners, edges, faces and the centre of a chunk, the rest unobserved"""
    data = np.full(F.CW, F.pack(TAU, 0), dtype=np.uint32)
    idx = np.stack(np.meshgrid(*(np.array([0, 1, 31, 32, 62, 63]),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    data[idx[:, 0] * 4096 + idx[:, 1] * 64 + idx[:, 2]] = F.pack(rng.integers(-TAU, TAU + 1, len(idx)), rng.choice([1, 9, 700], len(idx)))
    return data


def pull_exact(pose, res, voxels):
    """q (n, 3) and d = p - pivot_dst (n, 3) of DST world voxels by the rule's formula alone: no reach, no dead points.  int64
    suffices: |d| < 2^33 here and |rot| <= 2^30, three products below 2^63 / 3 as long as |d| < 2^31; larger levers are not used"""
    pose = np.asarray(pose, dtype=np.int64)
    d = np.asarray(voxels, dtype=np.int64).reshape(-1, 3) * res + res // 2 - pose[9:12]
    assert np.abs(d).max() < 2 ** 31
    return ((d @ pose[:9].reshape(3, 3).T + (1 << 29)) >> 30) + pose[12:15], d


def src_covering(pose, res, voxels, rng, entry=None):
    """chunks of SRC in which all eight corners of the cell of every given DST voxel are observed (random value, weight from
    {1, 9, 700}, or `entry`), whatever the reach and the dead rule say about the voxel; corners beyond int32 voxels are left out"""
    q, _ = pull_exact(pose, res, voxels)
    b = (q - res // 2) // res
    corners = np.unique((b[:, None, :] + np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.int64)[None]).reshape(-1, 3), axis=0)
    corners = corners[np.all((corners >= I32_MIN) & (corners <= I32_MAX), axis=1)]
    out = {}
    for v in corners:
        key = tuple(int(c) >> 6 for c in v)
        data = out.setdefault(key, np.full(F.CW, F.pack(TAU, 0), dtype=np.uint32))
        l = v & 63
        data[l[0] * 4096 + l[1] * 64 + l[2]] = entry if entry is not None else F.pack(int(rng.integers(-TAU, TAU + 1)), int(rng.choice([1, 9, 700])))
    return out


def block(lo, hi):
    """the voxels of the box [lo, hi) (n, 3) int64"""
    return np.stack(np.meshgrid(*(np.arange(a, b, dtype=np.int64) for a, b in zip(lo, hi)), indexing="ij"), axis=-1).reshape(-1, 3)


def expect(scene):
    """fuse_at over receivers, once per scene"""
    if "want_at" not in scene:
        scene["voxels"] = F.receivers(scene["src"], scene["pose"], scene["res"])
        scene["want_at"] = F.fuse_at(scene["dst"], scene["src"], scene["pose"], scene["res"], scene["mw"], FILL, scene["voxels"])
    return scene["want_at"]


def expect_plan(scene):
    """the model that goes through the plan, once per scene"""
    if "want" not in scene:
        scene["want"] = F.fuse(scene["dst"], scene["src"], scene["pose"], scene["res"], scene["mw"], FILL)
    return scene["want"]


# ---- random rigid poses
def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    res = RANDOM_RES[seed % 4]
    u = rng.normal(size=4)
    w, x, y, z = u / np.linalg.norm(u)  # a uniformly random rotation SRC -> DST
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = rng.uniform(-2.0 ** 23, 2.0 ** 23, 3)
    pd = rng.integers(-2 ** 22, 2 ** 22 + 1, 3)
    ps = np.rint(R.T @ (pd - t)).astype(np.int64)  # pivot_dst = R pivot_src + t up to the rounding
    pose = make_pose(np.clip(np.rint(R.T * Q30), -Q30, Q30).astype(np.int64).reshape(-1), pd, ps)
    k0 = (ps // (64 * res)) + rng.integers(-3, 4, 3)
    if (seed // 4) % 2 == 0:
        k1 = k0.copy()
        k1[int(rng.integers(3))] += int(rng.choice([-1, 1]))  # face neighbours
    else:
        k1 = k0 + np.array([40, -25, 13]) * rng.choice([-1, 1], 3)  # far apart, still within the reach at every resolution
    src = {tuple(int(c) for c in k0): sparse_chunk(rng), tuple(int(c) for c in k1): sparse_chunk(rng)}
    scene = {"name": "random%02d" % seed, "src": src, "dst": {}, "pose": pose, "res": res, "mw": MW, "far": (seed // 4) % 2 == 1}
    # DST: one random chunk where most lands, so that averaging occurs
    v = F.receiving(src, pose, res, F.receivers(src, pose, res))[0]
    if len(v):
        keys, n = np.unique(v >> 6, axis=0, return_counts=True)
        scene["dst"] = {tuple(int(c) for c in keys[int(np.argmax(n))]): S.draw(2000 + seed, False)}
    return scene


# ---- the dead boundary: along one row of the DST chunk (0, 0, 0), indices 24 .. 39, q crosses 2^30 - 1 | beyond (or the mirror)
def dead_scene(name, rot, res, axis, src_axis, sign, negative, at_limit):
    lo, hi = [8, 20, 12], [12, 24, 16]
    lo[axis], hi[axis] = 24, 40
    row = block(lo, hi)
    # index i along `axis`: q = sign (i res + h) + ps.  The last live index is 31 or 32; at_limit puts the first dead q at +-2^30
    # itself instead of the last live one at +-(2^30 - 1) (the same thing at res = 1)
    h = res // 2
    edge = (Q30 - 1) if not at_limit else (Q30 - res)
    if not negative:
        live_i = 31 if sign > 0 else 32
        ps_k = edge - sign * (live_i * res + h)
    else:
        live_i = 32 if sign > 0 else 31
        ps_k = -edge - sign * (live_i * res + h)
    ps = [0, 0, 0]
    ps[src_axis] = ps_k
    pose = make_pose(rot, (0, 0, 0), ps)
    rng = np.random.default_rng(77 + res + 10 * axis + (100 if negative else 0))
    live_side = (row[:, axis] <= live_i) if (sign > 0) != negative else (row[:, axis] >= live_i)
    return {"name": name, "src": src_covering(pose, res, row, rng), "dst": {(0, 0, 0): S.draw(300 + res + axis, False)}, "pose": pose, "res": res, "mw": MW,
            "must": row[live_side], "must_not": row[~live_side], "why": "dead", "covered": True}


def dead_scenes():
    out = []
    for res in (1, 64):
        for negative in (False, True):
            for at_limit in ((False,) if res == 1 else (False, True)):
                tag = "%s_res%d%s" % ("neg" if negative else "pos", res, "_limit" if at_limit else "")
                out.append(dead_scene("dead_identity_z_" + tag, IDENTITY, res, 2, 2, 1, negative, at_limit))
                out.append(dead_scene("dead_quarter_z_" + tag, QUARTER_Z, res, 2, 2, 1, negative, at_limit))
                out.append(dead_scene("dead_quarter_x_" + tag, QUARTER_Z, res, 0, 1, -1, negative, at_limit))  # q_y = -(p_x - pivot_dst_x) + pivot_src_y
    return out


# ---- pivot_src beyond +-2^30: the lever p - pivot_dst brings q back inside; with the pivot at the end of int32 it cannot
def pivot_scenes():
    out, res = [], 64
    for sign in (1, -1):
        ps_x = sign * (Q30 + 2 ** 23)
        i0 = -sign * (2 ** 23 // res + 100)  # q_x = sign (2^30 - 100 res) or so
        voxels = block((i0 - 2, 4, 4), (i0 + 2, 8, 8))
        pose = make_pose(IDENTITY, (0, 0, 0), (ps_x, 0, 0))
        rng = np.random.default_rng(500 + sign)
        src = src_covering(pose, res, voxels, rng)
        dst = {tuple(int(c) >> 6 for c in voxels[0]): S.draw(510 + sign, False)}
        out.append({"name": "pivot_src_beyond_%s" % ("pos" if sign > 0 else "neg"), "src": src, "dst": dst, "pose": pose, "res": res, "mw": MW, "must": voxels})
        far = make_pose(IDENTITY, (0, 0, 0), (I32_MAX if sign > 0 else I32_MIN, 0, 0))
        out.append({"name": "pivot_src_at_int32_%s" % ("max" if sign > 0 else "min"), "src": src, "dst": dst, "pose": far, "res": res, "mw": MW, "nothing": True,
                    "must_not": voxels, "why": "dead", "covered": False})
    return out


# ---- DST at the ends of int32 voxels, res = 1: SRC near its own origin goes on beyond the last voxel of DST
def int32_end_scene(top, count_only=False):
    pd_x = I32_MAX - 100 if top else I32_MIN + 100
    pose = make_pose(IDENTITY, (pd_x, 0, 0), (0, 0, 0))
    x_lo, x_hi = (I32_MAX - 140, I32_MAX + 20) if top else (I32_MIN - 20, I32_MIN + 140)
    voxels = block((x_lo, 0, 0), (x_hi + 1, 2, 2))  # (voxels beyond int32 among them: SRC is observed there too)
    rng = np.random.default_rng(600 + int(top))
    src = src_covering(pose, 1, voxels, rng)
    real = voxels[(voxels[:, 0] >= I32_MIN) & (voxels[:, 0] <= I32_MAX)]
    near = (TOP_KEY - 1, 0, 0) if top else (BOTTOM_KEY + 1, 0, 0)
    return {"name": "int32_%s%s" % ("top" if top else "bottom", "_count_only" if count_only else ""), "src": src, "dst": {near: S.draw(610 + int(top), False)}, "pose": pose,
            "res": 1, "mw": MW, "must": real, "keys_created": [(TOP_KEY if top else BOTTOM_KEY, 0, 0)], "count_only": count_only}


# ---- the reach under a rotation, res = 1 and pivot_dst = 0: p - pivot_dst is the voxel index itself
def reach_scene(name, rot):
    rows = []
    for axis in range(3):
        for sign in (1, -1):
            lo, hi = [5, 9, 3], [7, 11, 5]
            a, b = sign * (REACH - 2), sign * (REACH + 1)
            lo[axis], hi[axis] = min(a, b), max(a, b) + 1
            rows.append(block(lo, hi))
    voxels = np.concatenate(rows)
    pose = make_pose(rot, (0, 0, 0), (0, 0, 0))
    inside = np.all(np.abs(voxels) < REACH, axis=1)
    src = src_covering(pose, 1, voxels, np.random.default_rng(700))
    dst = {tuple(int(c) >> 6 for c in voxels[0]): S.draw(710, False)}
    return {"name": name, "src": src, "dst": dst, "pose": pose, "res": 1, "mw": MW, "must": voxels[inside], "must_not": voxels[~inside], "why": "outside", "covered": True}


# ---- value and weight extremes through the whole call
def extreme_scene(mw):
    src_e = [(-32768, 32767), (32767, 32767), (-32768, 1)]
    dst_e = [(-32768, 32767), (32767, 32767), (32767, -32768), (0, 0)]
    src, dst = np.full(F.CW, F.pack(TAU, 0), dtype=np.uint32), np.full(F.CW, FILL, dtype=np.uint32)
    must = []
    for i, s in enumerate(src_e):
        for j, d in enumerate(dst_e):
            for k in range(4):
                at = (10 + 2 * i) * 4096 + (20 + 2 * j) * 64 + 30 + k
                src[at], dst[at] = F.pack(*s), F.pack(*d)
                must.append((10 + 2 * i, 20 + 2 * j, 30 + k))
    return {"name": "extremes_mw%d" % mw, "src": {(0, 0, 0): src}, "dst": {(0, 0, 0): dst}, "pose": make_pose(IDENTITY), "res": 1 if mw == 1 else 64, "mw": mw,
            "must": np.array(must, dtype=np.int64)}


def half_voxel_scene(res, value):
    """a translation by half a voxel on every axis: f = res / 2 on every axis, all eight corners take part; all of them hold `value`,
    so T is +-2^15 res^3 or so: the shifted numerator of fuse_sample is 0 (value -32768) or at its maximum (32767)"""
    pose = make_pose(IDENTITY, (0, 0, 0), (res // 2,) * 3)
    voxels = block((60, 60, 60), (66, 66, 66))  # across the corner where eight chunks meet
    src = src_covering(pose, res, voxels, None, entry=F.pack(value, 5))
    return {"name": "half_voxel_res%d_%d" % (res, value), "src": src, "dst": {(0, 0, 0): S.draw(800 + res, False)}, "pose": pose, "res": res, "mw": MW, "must": voxels,
            "value": value}


_SCENES = {}


def random_scenes():
    if "random" not in _SCENES:
        _SCENES["random"] = [random_case(seed) for seed in RANDOM_SEEDS]
    return _SCENES["random"]


def edge_scenes():
    if "edge" not in _SCENES:
        dead = dead_scenes()
        count_dead = dict(dead_scene("dead_quarter_x_pos_res64", QUARTER_Z, 64, 0, 1, -1, False, False), count_only=True)
        count_dead["name"] += "_count_only"
        _SCENES["edge"] = (dead + pivot_scenes() + [int32_end_scene(True), int32_end_scene(False)]
                           + [reach_scene("reach_quarter_z", QUARTER_Z), reach_scene("reach_general", general_rot())]
                           + [extreme_scene(1), extreme_scene(32767)] + [half_voxel_scene(r, v) for r in (2, 645) for v in (-32768, 32767)]
                           + [count_dead, int32_end_scene(True, count_only=True)])
    return _SCENES["edge"]


def scenes():
    return random_scenes() + edge_scenes()
