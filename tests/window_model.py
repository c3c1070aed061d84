"""A world model of the sliding window, and deterministic walks for it (tests/test_map_window_host.py proves it on the CPU
against LocalMap.shift; tests/test_gpu_map_window.py holds the device routes to it).

The model knows nothing of rings, slabs or chunks.  `world` is a dense uint32 array over a bounding box of world voxels that
holds what every voxel's entry IS; `store` is what a global map that only ever receives voxels when they leave the window must
hold.  Moving the window is three lines of numpy: the voxels of the old window that the new one does not hold go to `store`."""
import numpy as np


def window(size, pos):
    """lo = pos - size/2, hi = lo + size - 1: every ring cell once (pos + size/2 for an odd size)"""
    size, pos = np.asarray(size, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    lo = pos - size // 2
    return lo, lo + size - 1


def model_offset(size, pos):
    """offset = size/2 at pos = 0 and it follows pos: (size/2 + pos) mod size"""
    size, pos = np.asarray(size, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    return (size // 2 + pos) % size


def ring_axes(size, pos, offset, lo, hi):
    """per axis the storage index of world voxels lo .. hi: HDF5LocalMap::get_index, (x - pos + offset + size) % size"""
    size, pos, offset = (np.asarray(v, dtype=np.int64) for v in (size, pos, offset))
    return [(np.arange(int(lo[k]), int(hi[k]) + 1, dtype=np.int64) - pos[k] + offset[k] + size[k]) % size[k] for k in range(3)]


def box_inter(alo, ahi, blo, bhi):
    lo, hi = np.maximum(alo, blo), np.minimum(ahi, bhi)
    return (lo, hi) if np.all(lo <= hi) else None


class World:
    def __init__(self, size, bb_lo, bb_hi, default_raw, pos=(0, 0, 0)):
        self.size = np.asarray(size, dtype=np.int64)
        self.bb_lo, self.bb_hi = np.asarray(bb_lo, dtype=np.int64), np.asarray(bb_hi, dtype=np.int64)
        shape = tuple(int(v) for v in self.bb_hi - self.bb_lo + 1)
        self.default_raw = np.uint32(default_raw)
        self.world = np.full(shape, self.default_raw, dtype=np.uint32)
        self.store = np.full(shape, self.default_raw, dtype=np.uint32)
        self.written = np.zeros(shape, dtype=bool)  # voxels a test has written (for the revisit count of the walks)
        self.pos = np.asarray(pos, dtype=np.int64).copy()

    def sl(self, lo, hi):
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        assert np.all(lo >= self.bb_lo) and np.all(hi <= self.bb_hi) and np.all(lo <= hi), (lo, hi, self.bb_lo, self.bb_hi)
        return tuple(slice(int(lo[k] - self.bb_lo[k]), int(hi[k] - self.bb_lo[k]) + 1) for k in range(3))

    def window(self):
        return window(self.size, self.pos)

    def offset(self):
        return model_offset(self.size, self.pos)

    def write(self, lo, hi, data):
        wlo, whi = self.window()
        assert np.all(np.asarray(lo) >= wlo) and np.all(np.asarray(hi) <= whi)  # tests write through the window only
        s = self.sl(lo, hi)
        self.world[s] = np.asarray(data, dtype=np.uint32).reshape(self.world[s].shape)
        self.written[s] = True

    def box(self, lo, hi):
        return self.world[self.sl(lo, hi)]

    def entering_is_revisit(self, new_pos):
        """does the window at new_pos take in voxels that were written before they left?"""
        nlo, nhi = window(self.size, new_pos)
        seen = self.written[self.sl(nlo, nhi)].copy()
        it = box_inter(nlo, nhi, *self.window())
        if it is not None:
            seen[tuple(slice(int(it[0][k] - nlo[k]), int(it[1][k] - nlo[k]) + 1) for k in range(3))] = False
        return bool(seen.any())

    def move(self, new_pos):
        lo, hi = self.window()
        leaving = np.ones(tuple(int(v) for v in self.size), dtype=bool)
        it = box_inter(lo, hi, *window(self.size, new_pos))
        if it is not None:
            leaving[tuple(slice(int(it[0][k] - lo[k]), int(it[1][k] - lo[k]) + 1) for k in range(3))] = False
        s = self.sl(lo, hi)
        self.store[s][leaving] = self.world[s][leaving]  # (basic slices are views: this writes into self.store)
        self.pos = np.asarray(new_pos, dtype=np.int64).copy()

    def set_ring(self, data):
        """the whole window from a map in storage order (an oracle's result mirrored back into the model)"""
        lo, hi = self.window()
        ax = ring_axes(self.size, self.pos, self.offset(), lo, hi)
        self.write(lo, hi, np.asarray(data, dtype=np.uint32).reshape(tuple(int(v) for v in self.size))[np.ix_(*ax)])

    def ring(self):
        """the window in storage order, as a download of the device map (or LocalMap.data) must show it"""
        lo, hi = self.window()
        ax = ring_axes(self.size, self.pos, self.offset(), lo, hi)
        out = np.empty(tuple(int(v) for v in self.size), dtype=np.uint32)
        out[np.ix_(*ax)] = self.box(lo, hi)
        return out.reshape(-1)

    def check_chunks(self, chunks, cs=64):
        """every voxel of every chunk of a GlobalMap == store, and store is the default entry wherever there is no chunk"""
        covered = np.zeros(self.store.shape, dtype=bool)
        for key, data in chunks.items():
            base = np.asarray(key, dtype=np.int64) * cs
            c = np.asarray(data).reshape(cs, cs, cs)
            it = box_inter(base, base + cs - 1, self.bb_lo, self.bb_hi)
            outside = np.ones((cs, cs, cs), dtype=bool)
            if it is not None:
                s_c = tuple(slice(int(it[0][k] - base[k]), int(it[1][k] - base[k]) + 1) for k in range(3))
                s_w = self.sl(*it)
                assert np.array_equal(c[s_c], self.store[s_w]), key
                covered[s_w] = True
                outside[s_c] = False
            assert np.all(c[outside] == self.default_raw), key
        assert np.all(self.store[~covered] == self.default_raw)


# ---------------------------------------------------------------------------------------------------- walks
# (shape, seed) of the walks the host test proves and the GPU tests run.  (71, 61, 67) straddles the 64-voxel chunk edge;
# (3, 19, 5) has a size-3 axis, the smallest ws_map_create admits.  The seeds are chosen so that the counts of
# test_map_window_host.py::test_walks_contain_what_they_are_meant_to hold.
WALKS = [((21, 17, 13), 11), ((3, 19, 5), 12), ((71, 61, 67), 13)]


def step_sizes(n):
    """the |d| a walk must hold along an axis of size n: 1, n/2, n/2 + 1, n - 1, n (those that are a step at all)"""
    return sorted({d for d in (1, n // 2, n // 2 + 1, n - 1, n) if 1 <= d <= n})


def make_walk(size, seed, diagonals=4, base=(0, 0, 0)):
    """positions of a walk from `base` and back: the walk from the origin and back, moved by `base`.  Per axis and per required |d| a step out and the step back (the way back is
    a revisit), mixed with three-axis diagonal steps that pull towards the origin, in an order drawn from `seed`; every step has
    |d| <= size per axis (what ws_shift_begin and LocalMap.shift admit)."""
    size = np.asarray(size, dtype=np.int64)
    rng = np.random.default_rng(seed)
    moves = []
    for axis in range(3):
        for d in step_sizes(int(size[axis])):
            moves.append(("axis", axis, d))
    moves += [("diag", 0, 0)] * diagonals
    order = rng.permutation(len(moves))
    pos = np.zeros(3, dtype=np.int64)
    walk = []
    for i in order:
        kind, axis, d = moves[int(i)]
        if kind == "axis":
            sign = -1 if pos[axis] > 0 or (pos[axis] == 0 and rng.integers(0, 2)) else 1
            step = np.zeros(3, dtype=np.int64)
            step[axis] = sign * d
            walk.append(pos + step)
            walk.append(pos.copy())
        else:
            mag = np.array([rng.integers(1, int(s) + 1) for s in size], dtype=np.int64)
            sign = np.where(pos > 0, -1, np.where(pos < 0, 1, rng.choice([-1, 1], 3)))
            pos = pos + sign * mag
            walk.append(pos.copy())
    while np.any(pos != 0):  # home, in steps the window admits
        pos = pos - np.clip(pos, -size, size)
        walk.append(pos.copy())
    base = np.asarray(base, dtype=np.int64)
    return [tuple(int(v) for v in p + base) for p in walk]


def walk_bounds(size, walk, base=(0, 0, 0)):
    """a bounding box for every window of the walk from `base`, the windows between the axis steps of one shift included"""
    size = np.asarray(size, dtype=np.int64)
    p = np.asarray([tuple(int(v) for v in base)] + list(walk), dtype=np.int64)
    return p.min(axis=0) - size // 2, p.max(axis=0) - size // 2 + size - 1


def axis_range_diff(a_lo, a_hi, b_lo, b_hi):
    """the integers of a_lo .. a_hi that b_lo .. b_hi does not hold, as (lo, hi); None if there are none"""
    left = np.setdiff1d(np.arange(a_lo, a_hi + 1), np.arange(b_lo, b_hi + 1))
    if left.size == 0:
        return None
    assert left[-1] - left[0] + 1 == left.size  # one run: |d| <= size
    return int(left[0]), int(left[-1])


def expected_slabs(size, pos, new_pos):
    """from pos, new_pos and size alone: per axis that moves (x, y, z) the box that leaves -- the voxels of the window before
    that axis step which the window after it does not hold -- and the box that enters, the other way round"""
    p = np.asarray(pos, dtype=np.int64).copy()
    out = []
    for axis in range(3):
        if int(new_pos[axis]) == int(p[axis]):
            continue
        q = p.copy()
        q[axis] = new_pos[axis]
        (blo, bhi), (alo, ahi) = window(size, p), window(size, q)
        leave = axis_range_diff(blo[axis], bhi[axis], alo[axis], ahi[axis])
        enter = axis_range_diff(alo[axis], ahi[axis], blo[axis], bhi[axis])
        llo, lhi, elo, ehi = blo.copy(), bhi.copy(), alo.copy(), ahi.copy()
        llo[axis], lhi[axis] = leave
        elo[axis], ehi[axis] = enter
        out.append({"axis": axis, "leave": (llo, lhi), "enter": (elo, ehi)})
        p = q
    return out


def seam_voxel(size, lo):
    """per axis the world voxel of the window that lies in storage plane 0: the ring seam runs between it and the voxel before"""
    size, lo = np.asarray(size, dtype=np.int64), np.asarray(lo, dtype=np.int64)
    return lo + (-(lo + size // 2)) % size


def crosses_all_seams(size, pos, lo, hi):
    """the box holds, along every axis that has more than one cell, the voxels on both sides of the ring seam"""
    wlo, _ = window(size, pos)
    x0 = seam_voxel(size, wlo)
    return all(int(size[k]) == 1 or (lo[k] <= x0[k] - 1 and x0[k] <= hi[k]) for k in range(3)) and any(int(s) > 1 for s in size)


def draw_boxes(size, pos, rng, count=3):
    """boxes inside the window at pos: the first lies across the ring seam of every axis whose seam is inside the window (the
    offset is rotated), the others anywhere"""
    size = np.asarray(size, dtype=np.int64)
    wlo, whi = window(size, pos)
    x0 = seam_voxel(size, wlo)
    boxes = []
    for n in range(count):
        lo, hi = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
        for k in range(3):
            if n == 0 and x0[k] > wlo[k]:
                lo[k] = rng.integers(wlo[k], x0[k])        # <= x0 - 1
                hi[k] = rng.integers(x0[k], whi[k] + 1)    # >= x0
            else:
                a, b = rng.integers(wlo[k], whi[k] + 1, 2)
                lo[k], hi[k] = min(a, b), max(a, b)
        boxes.append((lo, hi))
    return boxes


def draw_words(rng, n):
    """arbitrary 32-bit words: any dropped or swapped bit shows"""
    return rng.integers(0, 2 ** 32, int(n), dtype=np.uint64).astype(np.uint32)


def walk_coverage(size, walk, seed, base=(0, 0, 0)):
    """what a walk from `base` holds, counted from the walk itself with the writes of run_walk between its steps (same seed, same
    boxes); "origin" counts the returns to `base`"""
    size = np.asarray(size, dtype=np.int64)
    base = np.asarray(base, dtype=np.int64)
    w = World(size, *walk_bounds(size, walk, base), 0, pos=base)
    rng = np.random.default_rng(seed)
    cov = {"steps": {(axis, d): 0 for axis in range(3) for d in step_sizes(int(size[axis]))}, "diagonal": 0, "corner": 0, "revisit": 0,
           "origin": 0, "seam_boxes": 0, "chunk_borders": 0, "negative_chunks": 0}
    for new_pos in walk:
        for lo, hi in draw_boxes(size, w.pos, rng):
            w.write(lo, hi, draw_words(rng, np.prod(hi - lo + 1)))
            cov["seam_boxes"] += crosses_all_seams(size, w.pos, lo, hi)
        d = np.asarray(new_pos, dtype=np.int64) - w.pos
        for axis in range(3):
            if d[axis] and (axis, abs(int(d[axis]))) in cov["steps"] and np.count_nonzero(d) == 1:
                cov["steps"][(axis, abs(int(d[axis])))] += 1
        cov["diagonal"] += bool(np.all(d != 0))
        slabs = expected_slabs(size, w.pos, new_pos)
        cov["corner"] += any(box_inter(*slabs[i]["leave"], *slabs[j]["enter"]) is not None for i in range(len(slabs)) for j in range(i))
        for s in slabs:
            lo, hi = s["leave"]
            cov["chunk_borders"] += bool(np.any(lo // 64 != hi // 64))
            cov["negative_chunks"] += bool(np.any(lo // 64 < 0))
        cov["revisit"] += w.entering_is_revisit(new_pos)
        w.move(new_pos)
        cov["origin"] += bool(np.all(w.pos == base))
    return cov


def run_walk(size, walk, seed, route, default_raw, check_every=True, world=None, base=(0, 0, 0)):
    """the walk from `base` (where the route's window already is) through `route`, random boxes written between the shifts (mirrored into the model), the invariant after every step.
    route: .insert(lo, hi, words), .shift(world, new_pos), .check(world) -- the last compares whatever the route can show
    (parameters, downloads) with the model"""
    size = np.asarray(size, dtype=np.int64)
    w = world if world is not None else World(size, *walk_bounds(size, walk, base), default_raw, pos=base)
    rng = np.random.default_rng(seed)
    route.check(w)
    for new_pos in walk:
        for lo, hi in draw_boxes(size, w.pos, rng):
            words = draw_words(rng, np.prod(hi - lo + 1))
            route.insert(lo, hi, words)
            w.write(lo, hi, words)
        route.shift(w, new_pos)  # (gets the model BEFORE the move: the raw route checks the slabs against it)
        w.move(new_pos)
        if check_every:
            route.check(w)
    route.check(w)
    return w


# ---------------------------------------------------------------------------------------------------- far bases
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def aligned_base(size, seed, signs):
    """per axis the multiple of 64 size[k] of largest magnitude, with the sign given, for which the bounding box of the walk
    (size, seed) from there still fits int32: ring offsets and chunk alignment are those of the walk from the origin"""
    size = np.asarray(size, dtype=np.int64)
    blo, bhi = walk_bounds(size, make_walk(size, seed))
    unit = 64 * size
    base = np.where(np.asarray(signs) > 0, (I32_MAX - bhi) // unit * unit, -((blo - I32_MIN) // unit * unit))
    return tuple(int(v) for v in base)


def touching_base(size, seed, hi_axis=0, lo_axis=1):
    """the bounding box of the walk (size, seed) from there has voxel INT32_MAX as its last along hi_axis and INT32_MIN as its first
    along lo_axis; the third axis is unaligned, at 2^30 + 37"""
    size = np.asarray(size, dtype=np.int64)
    blo, bhi = walk_bounds(size, make_walk(size, seed))
    base = np.full(3, 2 ** 30 + 37, dtype=np.int64)
    base[hi_axis] = I32_MAX - bhi[hi_axis]
    base[lo_axis] = I32_MIN - blo[lo_axis]
    return tuple(int(v) for v in base)


def far_bases(size, seed):
    """the bases the far-position tests run a walk from, by name"""
    return {"aligned+-+": aligned_base(size, seed, (1, -1, 1)), "aligned-+-": aligned_base(size, seed, (-1, 1, -1)),
            "touching": touching_base(size, seed)}


def fits_int32(lo, hi):
    return bool(np.all(np.asarray(lo) >= I32_MIN) and np.all(np.asarray(hi) <= I32_MAX))
