"""The scenes of the frontier tests (test_gpu_frontier.py, test_gpu_store_frontier.py): world-order boxes of raw entries, and the
conditions a scene must meet on the CPU before the device is asked.  No GPU and no built library at import."""
import numpy as np

import frontier_model as FM

TAU, RES, MW = 1000, 50, 640


def check_scene(rec, labels, table, records=200, clusters=5, largest=50):
    """conditions on the INPUTS: enough records, every one of the six mask bits, enough clusters, one large cluster"""
    assert len(rec) >= records, len(rec)
    assert int(np.bitwise_or.reduce(rec["mask"])) == 0b111111 and not np.any(rec["mask"] >> 6)
    assert len(table) >= clusters and int(table["count"].max()) >= largest, (len(table), int(table["count"].max()))
    assert int(table["count"].sum()) == len(rec) == len(labels)


def random_box(shape, seed):
    """about 40 % weight 0, some negative weights, free space at tau and anywhere else, the int16 extremes among the values"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    weight = rng.choice(np.array([0, 0, 0, 0, 1, 3, 10, 32767, -1, -32768], dtype=np.int32), size=n)
    value = rng.choice(np.array([TAU, TAU, TAU, 0, 1, TAU - 1, TAU + 1, 32767, -32767, -32768, -1, -TAU], dtype=np.int32), size=n)
    # the upper half along x is mostly occupied where it is observed: its free voxels are few and far apart, so the scene holds many
    # small clusters next to the one large cluster of the lower half
    sparse = (np.arange(n) // (shape[1] * shape[2]) >= shape[0] // 2) & (rng.random(n) >= 0.12)
    value = np.where(sparse & (value >= 0), -TAU // 4, value)
    raw = FM.pack(value, weight).reshape(shape)
    assert 0.3 < np.mean(weight == 0) < 0.5 and np.any(weight < 0)
    for v in (32767, -32767, -32768):
        assert np.any((value == v) & (weight > 0)), v
    return raw


# ------------------------------------------------------------------------------------------------ the hollow room
ROOM_SHAPE = (21, 19, 23)
# holes per wall (axis, side): rectangles (first corner, extent) in the wall's two other axes, at least two voxels apart and away from
# the edges of the room, so that every hole is one cluster of as many frontier voxels as it has wall voxels
ROOM_HOLES = {(0, 0): [((2, 3), (8, 8))], (0, 1): [((3, 4), (7, 7))], (1, 0): [((4, 5), (6, 8))], (1, 1): [((3, 3), (5, 5)), ((11, 12), (3, 3))],
              (2, 0): [((5, 4), (4, 4))], (2, 1): [((6, 5), (3, 3))]}
ROOM_RECORDS = sum(e[0] * e[1] for holes in ROOM_HOLES.values() for _, e in holes)
ROOM_CLUSTERS = sum(len(holes) for holes in ROOM_HOLES.values())


def room_box():
    """free space (value tau, weight 1) in [3, size - 4] per axis, walls one voxel thick around it (value -tau / 2, weight 5), nothing
    observed beyond; a hole is a piece of wall that was never observed"""
    shape = ROOM_SHAPE
    value, weight = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    wall = tuple(slice(2, s - 2) for s in shape)
    room = tuple(slice(3, s - 3) for s in shape)
    value[wall], weight[wall] = -TAU // 2, 5
    value[room], weight[room] = TAU, 1
    for (axis, side), holes in ROOM_HOLES.items():
        others = [k for k in range(3) if k != axis]
        for (c0, c1), (e0, e1) in holes:
            idx = [None] * 3
            idx[axis] = 2 if side == 0 else shape[axis] - 3
            idx[others[0]], idx[others[1]] = slice(3 + c0, 3 + c0 + e0), slice(3 + c1, 3 + c1 + e1)
            assert 3 + c0 + e0 <= shape[others[0]] - 4 and 3 + c1 + e1 <= shape[others[1]] - 4  # away from the room's edges
            weight[tuple(idx)] = 0
    return FM.pack(value, weight)


# ------------------------------------------------------------------------------------------------ component shapes
def corner_blobs(gap):
    """two 3 x 3 x 3 free blobs in unknown that touch at one corner only (gap 0: one cluster) or lie one voxel apart (gap 1: two)"""
    shape = (14, 13, 15)
    value, weight = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    for c in (2, 5 + gap):
        blob = (slice(c, c + 3),) * 3
        value[blob], weight[blob] = TAU, 2
    return FM.pack(value, weight)


def tunnel_box(n=40):
    """a one-voxel-wide free tunnel through unknown: in every other x plane a serpentine of full z rows at every other y, the planes
    joined at alternating corners.  Returns the box and the tunnel's length in voxels"""
    free = np.zeros((n, n, n), dtype=bool)
    xs, ys = list(range(1, n - 2, 2)), list(range(1, n - 2, 2))
    for i, x in enumerate(xs):
        rows = ys if i % 2 == 0 else ys[::-1]
        for j, y in enumerate(rows):
            free[x, y, 1:n - 1] = True
            if j + 1 < len(rows):  # the turn to the next row, at alternating ends of z
                free[x, (y + rows[j + 1]) // 2, (n - 2) if j % 2 == 0 else 1] = True
        if i + 1 < len(xs):  # the step to the next plane: where this plane's serpentine ends
            end_z = (n - 2) if len(rows) % 2 == 1 else 1
            free[x + 1, rows[-1], end_z] = True
    value, weight = np.where(free, TAU, 0).astype(np.int32), free.astype(np.int32)
    return FM.pack(value, weight), int(free.sum())


def u_box():
    """a U of free voxels in unknown, open towards +y; a box that starts at world y = cut leaves its two arms.  Returns (box, cut) for a
    window at pos 0"""
    shape = (15, 16, 13)
    value, weight = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    for sl in [(3, slice(3, 12), 6), (slice(3, 10), 3, 6), (9, slice(3, 12), 6)]:
        value[sl], weight[sl] = TAU, 1
    lo_y = 0 - shape[1] // 2
    return FM.pack(value, weight), lo_y + 6
