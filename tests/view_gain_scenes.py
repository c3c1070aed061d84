"""The scenes of the view-gain tests: hand-checkable boxes, the random windows with their views and fans, the chunk scenes, and the
conditions every scene must meet on the MODEL's output before the device is asked.

A scene of the random windows is (window size, n): the 70 views and the first n rays of the fan at max_range 3000.  The cases with
fewer views (1, 3) and with max_range 20 (K = 0: every ray of a view samples the one voxel of its origin) are prefixes of it; the
conditions on sample counts are asserted on the scene, where they can hold, not on a prefix of 63 rays that all end two voxels from
their origin."""
import numpy as np

import mesh_model as M
import surface_model as G
import view_gain_model as VM
from query_model import window

RES, TAU, MW = G.RES, G.TAU, 640
SIZES = G.SIZES
POS = (3, -2, 5)
OFFSET = (5, 11, 9)  # every axis of the ring wraps inside the window (the smallest size is 13)
M_VALUES, N_VALUES, RANGES, MIN_VALUES = (1, 3, 70), (1, 63, 64, 65, 1034), (20, 3000), (0, 1000)
DEFAULT, ANY_WEIGHT, RAYS = 0, 1, 2
FLAG_SETS = (DEFAULT, ANY_WEIGHT, RAYS)
DEAD_DIRS = {5: (0, 0, 0), 62: (2 ** 30, 1, 1), 64: (-2 ** 31, 0, 0), 1033: (1, -2 ** 30, 0)}  # a partial last wave and lane 0 among them


def pack(value, weight):
    import warpsense_amd as W
    return W.pack_entry(np.asarray(value).reshape(-1), np.asarray(weight).reshape(-1)).astype(np.uint32).reshape(np.shape(value))


def filled(shape, value, weight):
    return pack(np.full(shape, value, dtype=np.int64), np.full(shape, weight, dtype=np.int64))


def window_boxes(size):
    """the world-order boxes of both maps of a random window"""
    return [M.draw_entries(size, M.seeds_for(size, which)).reshape(size) for which in (0, 1)]


def views(size, pos=POS, res=RES, seed=11):
    """70 origins drawn inside the window; every third one is then moved up to 400 mm outside it along one axis (the first stays inside)"""
    lo, hi = window(size, pos)
    rng = np.random.default_rng(seed + sum(size))
    o = rng.integers(lo * res, (hi + 1) * res, (70, 3))
    for j in range(2, 70, 3):
        axis, out = int(rng.integers(0, 3)), int(rng.integers(1, 401))
        o[j, axis] = lo[axis] * res - out if rng.integers(0, 2) else (hi[axis] + 1) * res - 1 + out
    o[0] = (lo + np.asarray(size) // 2) * res + (7, 13, 21)
    return o.astype(np.int32)


def fan(seed=5):
    """1034 directions uniform in [-32768, 32768]^3, the dead rays of test_gpu_raycast.py planted"""
    d = np.random.default_rng(seed).integers(-32768, 32769, (1034, 3))
    for i, v in DEAD_DIRS.items():
        d[i] = v
    return d.astype(np.int32)


def check_scene(w, n, outside_origins=True):
    """the conditions on the model's march of a scene with n >= 63"""
    unknown, free = int(w["unknown"][:, :n].sum()), int(w["free"][:, :n].sum())
    blocked, open_ = int((w["stop"][:, :n] >= 0).sum()), int((w["stop"][:, :n] == VM.OPEN).sum())
    assert unknown >= 100 and free >= 100 and blocked >= 10 and open_ >= 10, (n, unknown, free, blocked, open_)
    if outside_origins:
        assert int(w["outside"][:, :n].sum()) >= 1
    if w["stop"].shape[0] >= 70:
        assert len(set(w["unknown_k2"][:, :n].sum(axis=1).tolist())) >= 2
    return unknown, free, blocked, open_


# ------------------------------------------------------------------------------------------------ the chunk scenes
def absent_ray_count(w, chunks, lo, hi, res, origins, dirs, max_range):
    """rays of a march over the box [lo, hi] of `chunks` with at least one counted sample whose voxel lies in an absent chunk (such a
    voxel is UNKNOWN); the samples are walked again, one by one"""
    import math
    from raycast_model import tdiv
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 1, 3)
    d = np.asarray(dirs, dtype=np.int64).reshape(1, -1, 3)
    L = np.array([max(math.isqrt(int(x) ** 2 + int(y) ** 2 + int(z) ** 2), 1) for x, y, z in d[0]], dtype=np.int64).reshape(1, -1, 1)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    code = lambda c: ((c[..., 0] + 2 ** 20) * 2 ** 21 + (c[..., 1] + 2 ** 20)) * 2 ** 21 + (c[..., 2] + 2 ** 20)  # |key| < 2^20
    present = code(np.asarray(sorted(chunks), dtype=np.int64).reshape(-1, 3))
    step = max(res // 2, 1)
    found = np.zeros(w["stop"].shape, dtype=bool)
    for k in range(max_range // step + 1):
        v = (o + tdiv(d * (k * step), L)) // res
        counted = ((w["stop"] == VM.OPEN) | (w["stop"] > k)) & np.all((v >= lo) & (v <= hi), axis=2)
        found |= counted & ~np.isin(code(v // 64), present)
    return int(found.sum())


def store_scenes():
    """(name, chunks, lo, hi, origins, dirs, max_range): the seam store under a box that is not aligned to its chunks and under one
    larger than their bounding box (the chunk (0, 0, -1) is absent inside both), a far chunk at negative keys with absent space around
    it inside the box, the gap rows (one absent chunk between two present ones) and the range row (twelve absent chunks in a row).
    The scenes with fewer than 63 rays are exempt from the count conditions."""
    import store_raycast_scenes as SR
    import store_scenes as SM
    rng = np.random.default_rng(23)
    d = rng.integers(-32768, 32769, (200, 3)).astype(np.int32)
    d[7], d[64] = (0, 0, 0), (2 ** 30, 0, 1)
    near = np.array([[40, -35, 120], [-900, 700, -1500], [1500, 1400, -1600], [-2050, -1500, 1000], [3300, 200, 100]], dtype=np.int32)  # the third in the absent chunk, the last outside
    out = [("seam, cut box", SM.seam_chunks(), *SM.CUT_BOXES[0], near, d, 3000),
           ("seam, larger box", SM.seam_chunks(), (-100, -90, -70), (90, 100, 130), near, d, 3000)]
    key = np.asarray(SM.FAR_KEYS[0], dtype=np.int64)
    far_o = ((key * 64 + np.concatenate([rng.integers(0, 64, (9, 3)), [[-4, 20, 70]]])) * RES + 9).astype(np.int32)  # nine in the chunk, one beside it
    out.append(("far, negative keys", SM.far_chunks(), tuple(key * 64 - 10), tuple(key * 64 + 73), far_o, d, 2500))
    gap_o = np.stack([SR.GAP_ORIGIN, SR.GAP_ORIGIN + (64 * RES, 0, 0)]).astype(np.int32)  # in the middle chunk; in the absent one beside it
    out.append(("gap rows", SR.gap_chunks(), (-128,) * 3, (191,) * 3, gap_o, SR.gap_dirs().astype(np.int32), 200 * RES))
    case = SR.range_case()
    rlo, rhi = SM.bounding_box(SR.RANGE_KEYS)
    out.append(("range row", SR.range_chunks(), tuple(rlo), tuple(rhi), np.stack([case["origin"], case["origin"] + (5000, 7, -9)]).astype(np.int32),
                case["dirs"].astype(np.int32), int(case["range"])))
    return out


def edge_scene(res, sign):
    """an origin with |o| + max_range + 2 res == INT32_MAX exactly on x, in the centre voxel of the window of query_domain_scenes
    around it, and eleven more at that x up to eight voxels away in y and z (some outside the window); the fan holds the special
    directions of the ray cast tests.  Returns (pos, box, lo, origins, dirs, max_range)."""
    import query_domain_scenes as QD
    pos, origin, rng = QD.edge_case(res, sign)
    ring = QD.ring(pos)
    ax = [(np.arange(ring.lo[k], ring.hi[k] + 1) - ring.pos[k] + ring.offset[k] + ring.size[k]) % ring.size[k] for k in range(3)]
    g = np.random.default_rng(res)
    o = origin + np.concatenate([np.zeros((1, 3), dtype=np.int64), g.integers(-8 * res, 8 * res + 1, (11, 3)) * (0, 1, 1)])
    d = np.concatenate([QD.SPECIAL, g.integers(-32768, 32769, (118, 3))])
    return pos, np.asarray(ring.data)[np.ix_(*ax)], ring.lo, o, d, rng


# ------------------------------------------------------------------------------------------------ the scanned room
ROOM_SIZE = (81, 61, 41)        # the walls in y and z are inside the window, the room runs on beyond it in x
ROOM_SEED_MM = (200, 25, 25)    # the sensor's own voxel is never observed: the robot seeds the free space 200 mm in front of pose A
ROOM_CLEARANCE_M, ROOM_RANGE_MM, ROOM_MIN_SIZE = 0.05, 2000, 4


def room_scan():
    import store_scenes as SM
    return SM.walk_scan(0)  # pose A: the sensor at the origin of the room


def room_fan():
    import warpsense_amd as W
    return W.view_fan(8, 64, 40.0)  # the scan's own pattern, decimated: 32 rings x 256 azimuths over the same vertical span


def oracle_room():
    """(box, lo): the window after the oracle's update with the scan from pose A, in world order"""
    import oracle_lib as O
    avg, new = O.OracleMap(ROOM_SIZE, TAU, 0), O.OracleMap(ROOM_SIZE, TAU, 0)
    O.update_tsdf(avg, new, room_scan(), (0, 0, 0), (0, 0, 32768), TAU, MW, RES)
    lo, hi = window(ROOM_SIZE, (0, 0, 0))
    ax = [(np.arange(lo[k], hi[k] + 1) - avg.pos[k] + avg.offset[k] + avg.size[k]) % avg.size[k] for k in range(3)]
    return avg.data.reshape(ROOM_SIZE)[np.ix_(*ax)], lo


def next_view_model(box, lo, res=RES):
    """TSDFMapping.next_best_view restated on the models: the clustered frontier, the distance field of a one-voxel clearance, the reach
    from the seed, the cheapest member of every cluster (the first among equals), the gain at the voxel centres of the reachable
    clusters of at least ROOM_MIN_SIZE voxels, and the rank without a cost term.  Returns (record at A, candidates, goals, records,
    order)."""
    import distance_model as DM
    import frontier_model as FM
    import reach_model as RM
    rec, labels, table = FM.frontier(box, lo)
    dist, _ = DM.model_box(box, 2)
    cost, kept, _ = RM.field(dist, lo, [np.asarray(ROOM_SEED_MM) // res], 1)
    assert kept == 1
    at = RM.lookup(cost, lo, np.stack([rec["x"], rec["y"], rec["z"]], axis=1))
    cand, goals = [], []
    for c in range(len(table)):
        members = np.flatnonzero(labels == c)
        best = at[members].min()
        if best != RM.INF and table["count"][c] >= ROOM_MIN_SIZE:
            first = members[np.flatnonzero(at[members] == best)[0]]
            cand.append(c)
            goals.append([int(rec[n][first]) for n in "xyz"])
    goals = np.asarray(goals, dtype=np.int64).reshape(-1, 3)
    fan = room_fan()
    a = VM.model(box, lo, res, [[0, 0, 0]], fan, ROOM_RANGE_MM)[0]
    records = VM.model(box, lo, res, goals * res + res // 2, fan, ROOM_RANGE_MM)[0]
    order = np.argsort(-records["unknown_k2"].astype(np.float64), kind="stable")
    return a, np.asarray(cand, dtype=np.int64), goals, records, order


# ------------------------------------------------------------------------------------------------ the store at 1 mm and beyond 32 bits
def store_edge_scene(where):
    """Resolution 1 mm (step = max(res / 2, 1) = 1) at the edge of int32: the "gap" rays of query_domain_scenes, whose origin has
    |o| + max_range + 2 res == INT32_MAX exactly on x and which cross the absent chunks towards the isolated chunk.  The box is the
    row of chunks from the origin's to the isolated one.  Returns (chunks, lo, hi, origins, dirs, max_range)."""
    import query_domain_scenes as QD
    chunks = QD.store_chunks(1, where)
    o, d, rng = QD.store_rays(1, where)["gap"]
    K, x_lone = QD.store_keys(1, where)
    xs = sorted([int(o[0]) // 64, x_lone])
    lo = np.array([xs[0] * 64, K[1] * 64, K[2] * 64], dtype=np.int64)
    hi = np.array([xs[1] * 64 + 63, K[1] * 64 + 63, K[2] * 64 + 63], dtype=np.int64)
    assert int(np.abs(o).max()) + rng + 2 == 2 ** 31 - 1 and rng <= 8191
    return chunks, lo, hi, np.stack([o, o + (0, 7, -11)]), d, rng


def big_sum_scene():
    """Sums beyond 32 bits: a box of 2601 x 3 x 3 voxels along x with one present chunk, FREE everywhere, around the origin and
    nothing else, so that every other voxel of the box is UNKNOWN; 1000 rays close to +-x, K = 2400.  The ray along an axis alone sums
    k^2 beyond 2^32.  Returns (chunks, lo, hi, origins, dirs, max_range)."""
    g = np.random.default_rng(3)
    d = np.concatenate([np.full((1000, 1), 2 ** 20, dtype=np.int64) * g.choice((-1, 1), (1000, 1)), g.integers(-600, 601, (1000, 2))], axis=1)
    d[::10, 1:] = g.integers(-2 ** 14, 2 ** 14, (100, 2))  # every tenth leaves the box early
    d[0], d[1] = (2 ** 20, 0, 0), (-2 ** 20, 0, 0)
    chunks = {(0, 0, 0): filled((64 ** 3,), 500, 64)}
    return chunks, np.array([-1300, -1, -1]), np.array([1300, 1, 1]), np.array([[25, 25, 25]]), d, 2400 * (RES // 2)
