"""The scenes of the reach tests (test_gpu_reach.py, test_gpu_store_reach.py): world-order boxes of raw entries, and the window that
holds one.  No GPU and no built library at import."""
import numpy as np

import frontier_model as FM
from frontier_scenes import MW, RES, TAU
from query_model import window

R = 4  # max_dist_vox of the distance calls: R^2 = 16 covers clear_d2 = 9


def make_window(box, pos=(0, 0, 0), offset=None):
    """a TSDFCuda whose avg_map window holds `box` (world order, first voxel window(size, pos)[0]) in a ring rotated by `offset`"""
    import warpsense_amd as W
    size = box.shape
    offset = tuple(s // 2 for s in size) if offset is None else offset
    lo, hi = window(size, pos)
    ax = [(np.arange(lo[k], hi[k] + 1, dtype=np.int64) - pos[k] + offset[k] + size[k]) % size[k] for k in range(3)]
    data = np.zeros(size, dtype=np.uint32)
    data[np.ix_(ax[0], ax[1], ax[2])] = box
    t = W.TSDFCuda(W.DeviceMap(size, offset, np.ascontiguousarray(data.reshape(-1)), pos), TAU, MW, RES)
    assert np.array_equal(t.avg_map().extract_box(lo, hi).reshape(size), box)  # the ring holds the box
    return t, lo, hi


def pack(free, unknown=None):
    """entries from a boolean array of free voxels (value tau, weight 1); `unknown` voxels keep weight 0, the rest is occupied"""
    value = np.where(free, TAU, -TAU // 2).astype(np.int32)
    weight = np.where(free, 1, 5).astype(np.int32)
    if unknown is not None:
        value, weight = np.where(unknown, 0, value), np.where(unknown, 0, weight)
    return FM.pack(value, weight)


def random_box(shape=(20, 19, 21), seed=1):
    """Free space with about 6 % occupied and 10 % unknown, in pieces large enough that a clearance of three voxels leaves room: a
    baffle across the lower half of y, two walls that seal the corner x >= 14, y >= 13 (a tenth of the box that no path enters), a few
    single occupied voxels; the top layer and 6 % of single voxels are unknown."""
    rng = np.random.default_rng(seed)
    occ = np.zeros(shape, dtype=bool)
    occ[7, 0:10, :] = True
    occ[13, 13:, :] = True
    occ[13:, 12, :] = True
    occ |= rng.random(shape) < 0.002
    unknown = rng.random(shape) < 0.06
    unknown[:, :, shape[2] - 1] = True
    unknown &= ~occ
    assert 0.04 < occ.mean() < 0.08 and 0.08 < unknown.mean() < 0.13, (occ.mean(), unknown.mean())
    return pack(~occ & ~unknown, unknown)


def serpentine_box(n=8):
    """a one-voxel-wide free corridor that fills an n^3 box plane by plane and row by row, everything else unknown; the box is one tile"""
    free = np.zeros((n, n, n), dtype=bool)
    xs, ys = list(range(0, n, 2)), list(range(0, n, 2))
    for i, x in enumerate(xs):
        rows = ys if i % 2 == 0 else ys[::-1]
        for j, y in enumerate(rows):
            free[x, y, :] = True
            if j + 1 < len(rows):
                free[x, (y + rows[j + 1]) // 2, (n - 1) if j % 2 == 0 else 0] = True
        if i + 1 < len(xs):
            free[x + 1, rows[-1], (n - 1) if len(rows) % 2 == 1 else 0] = True
    return pack(free, ~free)


def two_rooms(shape=(24, 13, 12)):
    """two rooms with a wall of sites at x = 12 between them and a one-voxel gap in it"""
    free = np.ones(shape, dtype=bool)
    free[12, :, :] = False
    free[12, 6, 5] = True
    return pack(free)


def sealed_room(shape=(22, 20, 9)):
    """free space in [2, size - 3] with walls around it, nothing observed beyond, two holes in the outer walls (frontier clusters that can
    be reached), and a pocket sealed by walls in one corner whose far wall has a hole too: a frontier cluster that cannot be reached"""
    value, weight = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    wall = tuple(slice(1, s - 1) for s in shape)
    room = tuple(slice(2, s - 2) for s in shape)
    value[wall], weight[wall] = -TAU // 2, 5
    value[room], weight[room] = TAU, 1
    value[14, 2:8, 2:-2], weight[14, 2:8, 2:-2] = -TAU // 2, 5   # the pocket: x in [15, 19], y in [2, 6]
    value[14:20, 7, 2:-2], weight[14:20, 7, 2:-2] = -TAU // 2, 5
    weight[1, 10:13, 3:6] = 0    # a hole in the wall at -x
    weight[8:11, 18, 3:6] = 0    # a hole in the wall at +y
    weight[20, 3:6, 3:6] = 0     # a hole in the pocket's outer wall
    return FM.pack(value, weight)
