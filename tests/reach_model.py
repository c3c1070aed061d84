"""The model of ws_map_reach / ws_store_reach (rules stated in include/warpsense_hip.h), restated by rule: which record of a dense
distance result (distance_model.model_box) is traversable, what a step weighs, a heap Dijkstra for the minimum, a plain
repeat-until-stable relaxation as its second witness, the lookup, and the path walk with its tie-break.  Volumes are (nx, ny, nz)
arrays, column maps (nx, ny) arrays; a column map is a volume one record thick along z whose seeds, points and goals lose their z."""
import heapq
import itertools

import numpy as np

INF = 0xFFFFFFFF
HEADER = np.dtype([("cost", "<u4"), ("steps", "<u4"), ("written", "<u4"), ("status", "<u4")])
RECORD = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("cost", "<u4")])
# the neighbours in ascending (dx, dy, dz): the order that picks a predecessor
OFFSETS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]


def weight(d):
    return {1: 10, 2: 14, 3: 17}[sum(1 for v in d if v)]


def traversable(rec, clear_d2=0, unknown_free=False):
    rec = np.asarray(rec, dtype=np.uint32)
    cls, d2 = rec >> np.uint32(30), rec & np.uint32(0xFFFFFF)
    return ((cls == 1) | (bool(unknown_free) & (cls == 0))) & (d2 >= clear_d2)


def _volume(a):
    return a if a.ndim == 3 else a[:, :, None]


def _local(shape, lo, pts):
    """(inside, local coordinates) of world voxels in a box of `shape` (2-D: z is ignored) whose first voxel is lo"""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 3)[:, :len(shape)]
    loc = pts - np.asarray(lo, dtype=np.int64)[:len(shape)]
    inside = np.all((loc >= 0) & (loc < np.asarray(shape, dtype=np.int64)), axis=1)
    if len(shape) == 2:
        loc = np.concatenate([loc, np.zeros((len(loc), 1), np.int64)], axis=1)
    return inside, loc


def kept_seeds(rec, lo, seeds, clear_d2=0, unknown_free=False):
    """the local coordinates of the seeds that are kept: inside the box and on a traversable record (one row per seed given)"""
    trav = _volume(traversable(rec, clear_d2, unknown_free))
    inside, loc = _local(rec.shape, lo, seeds)
    return [tuple(int(v) for v in p) for ok, p in zip(inside, loc) if ok and trav[tuple(p)]]


def field(rec, lo, seeds, clear_d2=0, unknown_free=False):
    """(costs shaped like rec, seeds kept, records reached): Dijkstra over the traversable records"""
    trav = np.pad(_volume(traversable(rec, clear_d2, unknown_free)), 1, constant_values=False)
    cost = np.full(trav.shape, INF, dtype=np.int64)
    kept = kept_seeds(rec, lo, seeds, clear_d2, unknown_free)
    heap = []
    for p in kept:
        q = (p[0] + 1, p[1] + 1, p[2] + 1)
        if cost[q] != 0:
            cost[q] = 0
            heap.append((0, q))
    steps = [(d, weight(d)) for d in OFFSETS]
    while heap:
        c, p = heapq.heappop(heap)
        if c != cost[p]:
            continue
        for d, w in steps:
            q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
            if trav[q] and c + w < cost[q]:
                cost[q] = c + w
                heapq.heappush(heap, (c + w, q))
    out = cost[1:-1, 1:-1, 1:-1].astype(np.uint32).reshape(rec.shape)
    return out, len(kept), int(np.count_nonzero(out != INF))


def relax(rec, lo, seeds, clear_d2=0, unknown_free=False):
    """the same costs by repeating c(v) = min(c(v), c(p) + w(p, v)) over all records until nothing changes"""
    trav = _volume(traversable(rec, clear_d2, unknown_free))
    big = np.int64(1) << 40
    cost = np.full(trav.shape, big, dtype=np.int64)
    for p in kept_seeds(rec, lo, seeds, clear_d2, unknown_free):
        cost[p] = 0
    while True:
        pad = np.pad(cost, 1, constant_values=big)
        new = cost.copy()
        for d in OFFSETS:
            sl = tuple(slice(1 + d[k], 1 + d[k] + cost.shape[k]) for k in range(3))
            np.minimum(new, pad[sl] + weight(d), out=new)
        new = np.where(trav, new, big)
        if np.array_equal(new, cost):
            break
        cost = new
    return np.where(cost >= big, INF, cost).astype(np.uint32).reshape(rec.shape)


def lookup(cost, lo, pts):
    inside, loc = _local(cost.shape, lo, pts)
    vol = _volume(cost)
    out = np.full(len(loc), INF, dtype=np.uint32)
    out[inside] = vol[tuple(loc[inside].T)]
    return out


def paths(cost, lo, goals, cap_steps):
    """(headers [g], records [g, cap_steps]) of the walks from the goals back to a seed: the predecessor is the first neighbour in
    OFFSETS order whose cost plus the step's weight is the voxel's cost"""
    goals = np.asarray(goals, dtype=np.int64).reshape(-1, 3)
    inside, loc = _local(cost.shape, lo, goals)
    vol = np.pad(_volume(cost).astype(np.int64), 1, constant_values=INF)
    columns = cost.ndim == 2
    hdr, rec = np.zeros(len(goals), dtype=HEADER), np.zeros((len(goals), cap_steps), dtype=RECORD)
    for i in range(len(goals)):
        if not inside[i]:
            hdr[i] = (INF, 0, 0, 2)
            continue
        p = tuple(int(v) + 1 for v in loc[i])
        if vol[p] == INF:
            hdr[i] = (INF, 0, 0, 1)
            continue
        total, steps, written = int(vol[p]), 0, 0
        while True:
            if written < cap_steps:
                z = goals[i][2] if columns else lo[2] + p[2] - 1
                rec[i, written] = (lo[0] + p[0] - 1, lo[1] + p[1] - 1, z, vol[p])
                written += 1
            if vol[p] == 0:
                break
            for d in OFFSETS:
                q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if vol[q] != INF and vol[q] + weight(d) == vol[p]:
                    break
            else:
                raise AssertionError("not a fixed point: no predecessor")
            p, steps = q, steps + 1
            assert steps <= total // 10
        hdr[i] = (total, steps, written, 0)
    return hdr, rec


def legal_path(records, written, trav_cost):
    """every consecutive pair of a written path is a step of the 26-neighbourhood whose weight is the cost difference"""
    r = records[:written]
    for a, b in zip(r[:-1], r[1:]):
        d = (int(a["x"]) - int(b["x"]), int(a["y"]) - int(b["y"]), int(a["z"]) - int(b["z"]))
        if max(abs(v) for v in d) != 1 or int(a["cost"]) - int(b["cost"]) != weight(d):
            return False
    return True


# ------------------------------------------------------------------------------------------------ records by hand
def records_from(free, d2=None, cls=None):
    """distance records of a box given as a boolean array of free voxels (everything else occupied), d2 as given or 1 for free"""
    free = np.asarray(free, dtype=bool)
    c = np.where(free, 1, 2).astype(np.uint32) if cls is None else np.asarray(cls, dtype=np.uint32)
    d = np.where(free, 1, 0).astype(np.uint32) if d2 is None else np.asarray(d2, dtype=np.uint32)
    return (c << np.uint32(30)) | d
