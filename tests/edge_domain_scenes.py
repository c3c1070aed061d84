"""The windows, boxes, seeds, goals, sample points and chunk stores at the two ends of int32 voxel space on which frontier, reach,
sample and the store's frontier, surface, distance and reach are tested (tests/test_gpu_edge_domain.py on the device,
tests/test_edge_domain_host.py on the models alone).  All arithmetic here is int64; a cast to int32 happens only at the ABI.  No
GPU and no built library at import."""
import numpy as np

import distance_model as DM
import frontier_model as FM
import frontier_scenes as FS
import query_domain_scenes as Q
import query_model as QM
import raycast_model as R
import reach_model as RM
import reach_scenes as RS
import sample_model as H
import store_scenes as SM

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
TOP_KEY, BOTTOM_KEY = 2 ** 25 - 1, -2 ** 25  # the last and the first chunk key of int32 voxel space
CS, CW = 64, 64 ** 3
TAU, RES, MW = FS.TAU, FS.RES, FS.MW
FREE, WALL = FM.pack(TAU, 1), FM.pack(-TAU // 2, 3)

# ------------------------------------------------------------------------------------------------ bases
NEAR = (3, -2, 5)     # the pos of test_gpu_frontier.ROTATED and test_gpu_reach.ROTATED
OFFSET = (7, 4, 9)    # their ring offset: non-zero on every axis, the seam lies inside the window
BASES = ("near", "far0", "far1", "far2", "top", "bottom", "mixed")
EDGES = ("top", "bottom", "mixed")


def base_pos(size, name):
    """pos of a window of `size` at base `name`; its first and last voxel are asserted here"""
    s = np.asarray(size, dtype=np.int64)
    top, bottom = I32_MAX - (s - 1) + s // 2, I32_MIN + s // 2  # last voxel INT32_MAX / first voxel INT32_MIN
    if name == "near":
        pos = np.asarray(NEAR, dtype=np.int64)
    elif name.startswith("far"):
        pos = np.asarray(Q.FAR_ROWS[int(name[3:])][1], dtype=np.int64)
    else:
        pos = {"top": top, "bottom": bottom, "mixed": np.array([top[0], bottom[1], top[2]])}[name]
    lo, hi = QM.window(s, pos)
    assert np.all(lo >= I32_MIN) and np.all(hi <= I32_MAX) and np.all(hi - lo + 1 == s)
    want = {"top": (None, [I32_MAX] * 3), "bottom": ([I32_MIN] * 3, None), "mixed": ([None, I32_MIN, None], [I32_MAX, None, I32_MAX])}.get(name, (None, None))
    for got, end in zip((lo, hi), want):
        for k in range(3):
            assert end is None or end[k] is None or int(got[k]) == end[k], (name, size, lo, hi)
    assert all(0 < OFFSET[k] < s[k] for k in range(3))
    return pos


def shift(size, name):
    """whole voxels from the near window to the window at base `name`"""
    return base_pos(size, name) - base_pos(size, "near")


def moved_records(rec, s):
    out = rec.copy()
    for k, n in enumerate("xyz"):
        out[n] = rec[n].astype(np.int64) + int(s[k])
    return out


def moved_table(table, s):
    out = table.copy()
    s = np.asarray(s, dtype=np.int64)
    out["lo"], out["hi"] = table["lo"].astype(np.int64) + s, table["hi"].astype(np.int64) + s
    out["sum"] = table["sum"] + table["count"].astype(np.int64)[:, None] * s
    return out


def moved_frontier(res3, s):
    return moved_records(res3[0], s), res3[1], moved_table(res3[2], s)


# ------------------------------------------------------------------------------------------------ frontier
FRONTIER_SIZES = ((25, 23, 27), (24, 26, 24))  # one odd, one even: the even window ends at pos + size/2 - 1
_FRONTIER = {}


def frontier_box(size):
    """frontier_scenes.random_box with a plate of free voxels in the first and in the last x plane of the window, each in front of a
    plane of unknown voxels: every record of such a plate is one cluster, consecutive in the record order, whose x is the window's
    end; the plates reach the first and last plane of y and z too, and the random entries between them give the other clusters"""
    if size not in _FRONTIER:
        raw = FS.random_box(size, seed=sum(size)).copy()
        raw[1], raw[-2] = 0, 0
        raw[0], raw[-1] = FREE, FREE
        _FRONTIER[size] = raw
    return _FRONTIER[size]


def frontier_boxes(size, name):
    """(name, lo, hi) of the boxes asked for: NULL, the explicit window and an inner box; lo None stands for NULL"""
    lo, hi = QM.window(size, base_pos(size, name))
    return [("null", None, None, lo, hi), ("window", lo, hi, lo, hi), ("inner", lo + (2, 1, 1), hi - (1, 2, 1), lo + (2, 1, 1), hi - (1, 2, 1))]


def frontier_model(size, name, a, b, min_value=0, any_weight=False):
    lo, _ = QM.window(size, base_pos(size, name))
    sub = frontier_box(size)[tuple(slice(int(a[k] - lo[k]), int(b[k] - lo[k]) + 1) for k in range(3))]
    return FM.frontier(sub, a, min_value, any_weight)


def mixed_waves(labels):
    """per wave of 64 records: True where the wave is not a full wave of one label (its members are added one by one)"""
    n = len(labels)
    out = np.ones((n + 63) // 64, dtype=bool)
    for w in range(n // 64):
        out[w] = len(np.unique(labels[64 * w:64 * w + 64])) > 1
    return out


def check_frontier_scene(size, name):
    """conditions (a) to (f) on the whole-window result of the model at base `name`; returns what it counted"""
    lo, hi = QM.window(size, base_pos(size, name))
    rec, labels, table = frontier_model(size, name, lo, hi)
    FS.check_scene(rec, labels, table)                                                   # (f)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.int64)
    planes = {}
    for k in range(3):
        for side, end in ((0, lo[k]), (1, hi[k])):
            on = xyz[:, k] == end
            planes[(k, side)] = int(on.sum())
            assert on.sum() >= 8, (size, name, k, side, int(on.sum()))                   # (a)
            big = [c for c in np.unique(labels[on]) if table["count"][c] >= 3]
            assert big, (size, name, k, side)                                            # (b): a cluster with further members there
    mixed = mixed_waves(labels)
    assert np.any(~mixed) and np.all(labels[:64] == labels[0])                           # (c): a full wave of one label, at record 0
    split = [c for c in range(len(table)) if table["count"][c] >= 3 and len(np.unique(np.flatnonzero(labels == c) // 64)) >= 2
             and np.count_nonzero(mixed[np.unique(np.flatnonzero(labels == c) // 64)]) >= 2]
    assert split, (size, name)                                                           # (d)
    heavy = 0
    if name in ("top", "bottom"):
        sign = 1 if name == "top" else -1
        heavy = int(np.count_nonzero(np.all(sign * table["sum"] > 2 ** 33, axis=1)))
        assert heavy >= 1, (size, name)                                                  # (e)
    return dict(records=len(rec), clusters=len(table), planes=planes, split=len(split), heavy=heavy)


# ------------------------------------------------------------------------------------------------ reach
REACH_SHAPES = {"random_odd": (21, 19, 23), "random_even": (20, 18, 22), "rooms": (24, 13, 12)}
_REACH = {}


def reach_box(kind):
    if kind not in _REACH:
        _REACH[kind] = RS.two_rooms(REACH_SHAPES[kind]) if kind == "rooms" else RS.random_box(REACH_SHAPES[kind], seed=1)
    return _REACH[kind]


def outside_one(lo, hi, axes=3):
    """the voxel one outside each face of the box [lo, hi], where it exists in int32"""
    mid = (lo + hi) // 2
    out = []
    for k in range(axes):
        for end, step in ((lo[k], -1), (hi[k], 1)):
            if I32_MIN <= end + step <= I32_MAX:
                p = mid.copy()
                p[k] = end + step
                out.append(p)
    return out


def opposite_ends(lo, hi):
    """per axis a voxel at the end of int32 that is farther from the box: its difference from lo needs 33 bits at an edge base"""
    mid = (lo + hi) // 2
    out = []
    for k in range(3):
        p = mid.copy()
        p[k] = I32_MIN if abs(int(lo[k]) - I32_MIN) >= abs(I32_MAX - int(hi[k])) else I32_MAX
        out.append(p)
    return out


def reach_scene(kind, name, columns=False):
    """(box, lo, hi, distance records, kept seeds, dropped seeds) of a reach scene at base `name`.  The kept seeds are those of
    test_gpu_reach (three voxels that keep a clearance of three, low in x) for the random boxes and its one seed for the two rooms"""
    box = reach_box(kind)
    lo, hi = QM.window(box.shape, base_pos(box.shape, name))
    if columns:  # a height band without the unknown top layer, as in test_gpu_reach; a seed's z does not count
        box, lo, hi = box[:, :, 2:7], lo + (0, 0, 2), np.array([hi[0], hi[1], lo[2] + 6])
    rec, _ = DM.model_box(box, RS.R, columns=columns)
    if kind == "rooms":
        kept = [lo + (3, 6, 6)]
        on_site = lo + (12, 3, 3)  # in the wall
    else:
        strict = np.argwhere(RM._volume(RM.traversable(rec, 9, False)) & (np.arange(box.shape[0])[:, None, None] < 6))
        kept = list(strict[[0, len(strict) // 2, -1]] + lo)
        on_site = lo + (7, 3, 3)   # on the baffle
    two = opposite_ends(lo, hi)[:2]
    dropped = [on_site] + outside_one(lo, hi, 2 if columns else 3) + two
    return box, lo, hi, rec, np.asarray(kept, dtype=np.int64), np.asarray(dropped, dtype=np.int64)


def reach_goals(cost, lo, hi, trav, columns=False):
    """goals: a reached voxel on every outer plane of the box that has one (a record coordinate is then the window's end), the reached
    voxel farthest from the seeds, an unreachable traversable voxel if there is one, and voxels outside at the ends of int32; under
    columns the z of the first goal is INT32_MIN: it is echoed"""
    vol = RM._volume(cost)
    reached = np.argwhere(vol != RM.INF)
    goals = []
    for k in range(2 if columns else 3):
        for end in (0, vol.shape[k] - 1):
            on = reached[reached[:, k] == end]
            if len(on):
                goals.append(on[len(on) // 2])
    goals.append(reached[np.argmax(vol[tuple(reached.T)])])
    pocket = np.argwhere(RM._volume(trav) & (vol == RM.INF))
    goals += [p for p in pocket[:1]]
    goals = [np.asarray(g, dtype=np.int64) + (lo if not columns else np.array([lo[0], lo[1], 0])) for g in goals]
    if columns:
        for g in goals:
            g[2] = lo[2] + 1
        goals[0][2] = I32_MIN
    goals += opposite_ends(lo, hi)
    return np.asarray(goals, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ sample
SAMPLE_SIZE = Q.SIZE  # 21 x 17 x 13
SAMPLE_NEAR = Q.NEAR
SAMPLE_CASES = [(res, sign, axes) for res in (2, 50, 1024) for sign in (1, -1) for axes in ((0,), (1, 2))]
BAND = H.TAU // 2
LIMIT = 2 ** 30
_SAMPLE = {}


def sample_id(case):
    return f"res{case[0]}{'+' if case[1] > 0 else '-'}{''.join('xyz'[k] for k in case[2])}"


def sample_case(case):
    """(pos, Ring, points, indices of the 2^30 - 1 points, indices of the 2^30 points) of a window that the plane |coordinate| = 2^30
    mm cuts near its middle on the axes of the case"""
    if case in _SAMPLE:
        return _SAMPLE[case]
    res, sign, axes = case
    pos = np.asarray(SAMPLE_NEAR, dtype=np.int64).copy()
    for k in axes:
        pos[k] = (sign * LIMIT) // res
    data = H.draw_storage(SAMPLE_SIZE, seed=11 + res)
    ring = R.Ring(data, SAMPLE_SIZE, pos, Q.OFF)
    lo, hi = QM.window(SAMPLE_SIZE, pos)
    for k in axes:
        assert lo[k] + 4 < (sign * LIMIT) // res < hi[k] - 4  # the plane lies well inside the window
    rng = np.random.default_rng(1000 + res)
    pts = [H.window_points(lo, hi, res, seed=res + 3, n=8192 * len(axes))]  # (a half or three quarters of them lie beyond the plane: dead)
    live, dead = [], []
    n = len(pts[0])
    for k in axes:
        # lattice points of interior voxels on the other axes; of those whose cell is valid at 2^30 - 1 the first eight
        cand = (rng.integers(lo + 1, hi - 1, (400, 3))) * res + res // 2
        cand[:, k] = sign * (LIMIT - 1)
        ok = H.model(ring, res, cand, BAND)[0]["cls"] != H.UNKNOWN
        assert ok.sum() >= 8, (case, k, int(ok.sum()))
        a = cand[ok][:8]
        b = a.copy()
        b[:, k] = sign * LIMIT
        pts += [a, b]
        live += list(range(n, n + 8))
        dead += list(range(n + 8, n + 16))
        n += 16
        # random points within two voxels of the plane, 256 on each side
        for is_dead in (False, True):
            q = rng.integers(lo * res, (hi + 1) * res, (256, 3))
            q[::2] = (q[::2] // res) * res + res // 2  # half of them on the sample lattice of the other axes
            off = rng.integers(1, 2 * res + 1, 256)
            q[:, k] = sign * (LIMIT + off - 1) if is_dead else sign * (LIMIT - off)
            pts.append(q)
            n += 256
    pts = np.concatenate(pts).astype(np.int64)
    assert np.all(np.abs(pts) <= I32_MAX)
    _SAMPLE[case] = (pos, ring, pts, np.asarray(live), np.asarray(dead))
    return _SAMPLE[case]


def sample_near(case):
    """the same entries in a window at SAMPLE_NEAR and the points moved there by whole voxels: (Ring, points, shift in voxels)"""
    pos, ring, pts, _, _ = sample_case(case)
    s = pos - np.asarray(SAMPLE_NEAR, dtype=np.int64)
    return R.Ring(ring.data, SAMPLE_SIZE, SAMPLE_NEAR, Q.OFF), pts - s * case[0], s


def live_in_both(case):
    _, _, pts, _, _ = sample_case(case)
    _, near_pts, _ = sample_near(case)
    return ~np.any(np.abs(pts) >= LIMIT, axis=1) & ~np.any(np.abs(near_pts) >= LIMIT, axis=1)


# ------------------------------------------------------------------------------------------------ the store
_STORE = {}


def block_world():
    """128^3 entries of a 2 x 2 x 2 block of chunks, unknown but for: frontier_scenes.random_box around the common corner of the
    eight chunks, reach_scenes.random_box in the first and in the last corner of the block (its voxels lie in the outer planes of the
    block: at the top corner their coordinates are INT32_MAX, at the bottom corner INT32_MIN)"""
    if "world" not in _STORE:
        w = np.zeros((2 * CS,) * 3, dtype=np.uint32)
        w[54:74, 54:74, 54:74] = FS.random_box((20, 20, 20), seed=60)
        corner = RS.random_box()
        sx, sy, sz = corner.shape
        w[:sx, :sy, :sz] = corner[::-1, ::-1, :]      # (its unknown layer is the last along z: towards the inside of the block)
        w[2 * CS - sx:, 2 * CS - sy:, 2 * CS - sz:] = corner[:, :, ::-1]
        _STORE["world"] = w
    return _STORE["world"]


CORNER_SHAPE = (20, 19, 21)  # of reach_scenes.random_box


def block_base(where):
    """key of the first chunk of the block"""
    return {"near": (-1, -1, -1), "top": (TOP_KEY - 1,) * 3, "bottom": (BOTTOM_KEY,) * 3}[where]


def block_chunks(where):
    """seven chunks of the block, the one at store_scenes.ABSENT missing, keyed at the corner `where`"""
    K = block_base(where)
    out = {}
    for c, data in SM.split(block_world()).items():
        if c != SM.ABSENT:
            out[tuple(K[k] + c[k] + 1 for k in range(3))] = data
    lo, hi = SM.bounding_box(out)
    assert where != "top" or np.all(hi == I32_MAX)
    assert where != "bottom" or np.all(lo == I32_MIN)
    return out


def block_boxes(where):
    """the default box (None) and the bounding box grown by one voxel per side where that stays in int32"""
    lo, hi = SM.bounding_box(block_chunks(where))
    return [(None, None, lo, hi), (np.maximum(lo - 1, I32_MIN), np.minimum(hi + 1, I32_MAX)) * 2]


def present_of(chunks, lo, hi):
    return SM.assemble({k: np.ones(CW, dtype=np.uint32) for k in chunks}, lo, hi) != 0


def store_frontier_model(chunks, lo, hi, min_value=0, any_weight=False):
    return FM.frontier(SM.assemble(chunks, lo, hi), lo, min_value, any_weight, present_of(chunks, lo, hi))


def corner_box(where):
    """the box of the reach corner that touches the last voxel of the block on every axis"""
    _, hi = SM.bounding_box(block_chunks(where))
    return hi - np.asarray(CORNER_SHAPE, dtype=np.int64) + 1, hi


# the adversarial chunks: two pairs at opposite ends of int32, one along x for the record masks, one along y for the clusters
PAIR_K = 3
X_TOP, X_BOTTOM = (TOP_KEY, PAIR_K, PAIR_K), (BOTTOM_KEY, PAIR_K, PAIR_K)
Y_TOP, Y_BOTTOM = (PAIR_K, TOP_KEY, PAIR_K), (PAIR_K, BOTTOM_KEY, PAIR_K)
ALL_INT32 = (np.full(3, I32_MIN, dtype=np.int64), np.full(3, I32_MAX, dtype=np.int64))


def pair_pattern():
    return np.random.default_rng(8).random((CS, CS)) < 0.5


def pair_chunks():
    """x pair: the plane x = INT32_MAX is FREE where the plane x = INT32_MIN is UNKNOWN at the same (y, z) and the other way round; the
    planes behind them are unknown, so every free voxel is a record.  y pair: a free plate in the plane y = INT32_MAX and one in the
    plane y = INT32_MIN, one voxel further along x: two clusters, which a search that wraps along y would find adjacent"""
    if "pairs" not in _STORE:
        a = pair_pattern()
        xt, xb, yt, yb = (np.zeros((CS,) * 3, dtype=np.uint32) for _ in range(4))
        xt[CS - 1][a] = FREE
        xb[0][~a] = FREE
        yt[10:30, CS - 1, 10:30] = FREE
        yb[11:31, 0, 10:30] = FREE
        _STORE["pairs"] = {X_TOP: xt.reshape(-1), X_BOTTOM: xb.reshape(-1), Y_TOP: yt.reshape(-1), Y_BOTTOM: yb.reshape(-1)}
    return _STORE["pairs"]


def pair_records(wrap=False):
    """the records of the four chunks in the box of all int32, in record order: chunk by chunk on the chunk's own box grown by one voxel
    (nothing lies next to any of them).  wrap: the +x neighbour of x = INT32_MAX is taken to be x = INT32_MIN and the other way round,
    as arithmetic that wraps would have it"""
    chunks = pair_chunks()
    parts = []
    for key, data in chunks.items():
        base = np.asarray(key, dtype=np.int64) * CS
        a, b = np.maximum(base - 1, I32_MIN), np.minimum(base + CS, I32_MAX)
        rec = store_frontier_model({key: data}, a, b)[0]
        if wrap and key in (X_TOP, X_BOTTOM):
            other = chunks[X_BOTTOM if key == X_TOP else X_TOP].reshape((CS,) * 3)
            plane_x, bit = (I32_MAX, 1) if key == X_TOP else (I32_MIN, 0)
            unknown = FM.classes(other[0 if key == X_TOP else CS - 1])[1]
            on = rec["x"] == plane_x
            ly, lz = rec["y"][on].astype(np.int64) - base[1], rec["z"][on].astype(np.int64) - base[2]
            rec["mask"][on] |= (unknown[ly, lz].astype(np.uint32) << np.uint32(bit))
        parts.append(rec)
    rec = np.concatenate(parts)
    return rec[np.lexsort((rec["z"], rec["y"], rec["x"]))]


def pair_model():
    rec = pair_records()
    labels, table = FM.clusters(rec)
    return rec, labels, table


def wrapped_y(rec):
    """the records with y turned by half of int32: INT32_MAX and INT32_MIN become neighbours, as they are for a search that wraps"""
    out = rec.copy()
    out["y"] = rec["y"].astype(np.int64) % 2 ** 32 - 2 ** 31  # INT32_MAX -> -1, INT32_MIN -> 0
    return out[np.lexsort((out["z"], out["y"], out["x"]))]
