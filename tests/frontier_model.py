"""The numpy model of the frontier query (ws_map_frontier, ws_store_frontier; the rules are stated in include/warpsense_hip.h): dense
classification of an assembled raw array, six shifted comparisons for the mask, np.argwhere order for the records, a plain union-find
for the 26-connected components, relabelling by first member, and the cluster table by direct sums.  Nothing here knows how the
device gets there; every comparison against it is on raw bytes."""
from __future__ import annotations

import numpy as np

RECORD = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("mask", "<u4")])
CLUSTER = np.dtype([("first", "<u4"), ("count", "<u4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("sum", "<i8", (3,)), ("pad", "<u8")])
assert RECORD.itemsize == 16 and CLUSTER.itemsize == 64 and CLUSTER.fields["sum"][1] == 32

# bit b of a record's mask: the UNKNOWN neighbour at (axis, step)
NEIGHBOURS = ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))


def pack(value, weight):
    """raw entries from int16 values and weights (value in the low half)"""
    return (np.asarray(value).astype(np.int64) & 0xFFFF).astype(np.uint32) | ((np.asarray(weight).astype(np.int64) & 0xFFFF) << 16).astype(np.uint32)


def classes(raw, min_value=0, any_weight=False, present=None):
    """(free, unknown) of raw entries; `present` (bool, same shape): False marks a voxel of an absent chunk, UNKNOWN whatever it holds"""
    raw = np.asarray(raw, dtype=np.uint32)
    value = (raw & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32)
    weight = (raw >> 16).astype(np.uint16).view(np.int16).astype(np.int32)
    valid = (weight != 0) if any_weight else (weight > 0)
    if present is not None:
        valid = valid & np.asarray(present, dtype=bool)
    return valid & (value >= int(min_value)), ~valid


def records(raw_box, lo, min_value=0, any_weight=False, present=None):
    """the records of the box whose entries are raw_box [nx, ny, nz] and whose first world voxel is lo"""
    free, unknown = classes(raw_box, min_value, any_weight, present)
    mask = np.zeros(free.shape, dtype=np.uint32)
    for bit, (axis, step) in enumerate(NEIGHBOURS):
        nb = np.zeros(free.shape, dtype=bool)  # a neighbour outside the box is neither known nor unknown
        src, dst = [slice(None)] * 3, [slice(None)] * 3
        if step < 0:
            dst[axis], src[axis] = slice(1, None), slice(0, -1)
        else:
            dst[axis], src[axis] = slice(0, -1), slice(1, None)
        nb[tuple(dst)] = unknown[tuple(src)]
        mask |= nb.astype(np.uint32) << np.uint32(bit)
    mask[~free] = 0
    idx = np.argwhere(mask != 0)  # ascending (x, y, z), z fastest
    rec = np.zeros(len(idx), dtype=RECORD)
    lo = np.asarray(lo, dtype=np.int64)
    rec["x"], rec["y"], rec["z"] = (idx[:, 0] + lo[0]), (idx[:, 1] + lo[1]), (idx[:, 2] + lo[2])
    rec["mask"] = mask[idx[:, 0], idx[:, 1], idx[:, 2]]
    return rec


def clusters(rec):
    """(labels uint32 [n], table CLUSTER [K]) of records in record order: 26-connected components, numbered by first member"""
    n = len(rec)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.int64)
    where = {tuple(p): i for i, p in enumerate(xyz.tolist())}
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    steps = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) < (0, 0, 0)]
    for i, (x, y, z) in enumerate(xyz.tolist()):
        for dx, dy, dz in steps:
            j = where.get((x + dx, y + dy, z + dz))
            if j is not None:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)  # the root of a component is its first member
    root = np.array([find(i) for i in range(n)], dtype=np.int64)
    heads = np.flatnonzero(root == np.arange(n))
    number = np.full(n, -1, dtype=np.int64)
    number[heads] = np.arange(len(heads))
    labels = number[root].astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    table = np.zeros(len(heads), dtype=CLUSTER)
    for k, h in enumerate(heads.tolist()):
        members = xyz[labels == k]
        table["first"][k], table["count"][k] = h, len(members)
        table["lo"][k], table["hi"][k], table["sum"][k] = members.min(axis=0), members.max(axis=0), members.sum(axis=0)
    return labels, table


def frontier(raw_box, lo, min_value=0, any_weight=False, present=None):
    """(records, labels, table) of a box"""
    rec = records(raw_box, lo, min_value, any_weight, present)
    labels, table = clusters(rec)
    return rec, labels, table


def goals(table, resolution, min_size=1):
    """what warpsense_amd.frontier_goals returns, restated: centroids in metres, sizes, boxes; largest first, ties by `first`"""
    keep = table[table["count"] >= min_size]
    order = np.lexsort((keep["first"], -keep["count"].astype(np.int64)))
    keep = keep[order]
    centroid = keep["sum"].astype(np.float64) / keep["count"][:, None].astype(np.float64) * float(resolution) / 1000.0
    return centroid.reshape(-1, 3), keep["count"].copy(), keep["lo"].copy(), keep["hi"].copy()
