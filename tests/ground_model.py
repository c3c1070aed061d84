"""The numpy model of ws_map_ground / ws_store_ground and of the bridge ws_*_ground_distance, written from the rules stated in
include/warpsense_hip.h alone: loops per column and per voxel, no bit tricks.  The hand-made columns of the host test and the scenes
of the GPU tests are here too."""
import numpy as np

import distance_model as D
from query_model import unpack

UNKNOWN, GROUND, BLOCKED, VOID = 0, 1, 2, 3
REC = np.dtype([("z", "<i4"), ("w", "<u4")])
TAU = 600


def frac_of(v0, v1):
    assert v0 < 0 <= v1
    return min(255, (256 * (-v0)) // (v1 - v0))


def column(cls, value, lo_z, H, unknown_headroom=False, top=False):
    """(column class, z, frac) of one column: cls, value are its voxels inside the box, the first one at world z = lo_z"""
    n = len(cls)
    levels = []
    for i in range(n):
        if i + H > n - 1:  # z + H lies in the box's z range
            continue
        if cls[i] != 2 or cls[i + 1] != 1:
            continue
        if all(cls[i + k] == 1 or (unknown_headroom and cls[i + k] == 0) for k in range(2, H + 1)):
            levels.append(i)
    if levels:
        i = levels[-1] if top else levels[0]
        return GROUND, lo_z + i, frac_of(int(value[i]), int(value[i + 1]))
    if any(c == 2 for c in cls):
        return BLOCKED, 0, 0
    if any(c == 1 for c in cls):
        return VOID, 0, 0
    return UNKNOWN, 0, 0


def model_box(box, lo, H, any_weight=False, unknown_headroom=False, top=False):
    """(records shaped (nx, ny) of dtype REC, counts[4]) of the dense box of raw entries whose first voxel is world voxel `lo`"""
    assert 1 <= H <= 64
    nx, ny, nz = box.shape
    cls = D.classes(box, any_weight)
    value, _ = unpack(box)
    kind = np.zeros((nx, ny), dtype=np.int64)
    z = np.zeros((nx, ny), dtype=np.int64)
    frac = np.zeros((nx, ny), dtype=np.int64)
    for x in range(nx):
        for y in range(ny):
            kind[x, y], z[x, y], frac[x, y] = column(cls[x, y], value[x, y], int(lo[2]), H, unknown_headroom, top)
    h = z * 256 + frac
    step = np.zeros((nx, ny), dtype=np.int64)
    for x in range(nx):
        for y in range(ny):
            if kind[x, y] != GROUND:
                continue
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    u, v = x + dx, y + dy
                    if (dx or dy) and 0 <= u < nx and 0 <= v < ny and kind[u, v] == GROUND:
                        step[x, y] = max(step[x, y], abs(int(h[x, y]) - int(h[u, v])))
            step[x, y] = min(65535, step[x, y])
    rec = np.zeros((nx, ny), dtype=REC)
    rec["z"] = z.astype(np.int32)
    rec["w"] = (frac | (step << 8) | (kind << 30)).astype(np.uint32)
    return rec, np.array([np.count_nonzero(kind == c) for c in range(4)], dtype=np.uint64)


def same(got, want):
    return got.dtype == want.dtype == REC and got.shape == want.shape and np.array_equal(got["z"], want["z"]) and np.array_equal(got["w"], want["w"])


def bridge_classes(rec, max_step_q8):
    """the class of every column in the distance field of ws_*_ground_distance: 1 FREE, 2 OCCUPIED, 0 UNKNOWN"""
    kind, step = rec["w"] >> np.uint32(30), (rec["w"] >> np.uint32(8)) & np.uint32(0xFFFF)
    return np.where(kind == UNKNOWN, 0, np.where((kind == GROUND) & (step <= max_step_q8), 1, 2)).astype(np.uint8)


def bridge_model(rec, max_step_q8, R, unknown_occupied=False):
    """(distance records shaped (nx, ny), sites): the model's classes fed through distance_model's column transform"""
    cls = bridge_classes(rec, max_step_q8)
    site = (cls == 2) | (unknown_occupied & (cls == 0))
    g = np.where(site, 0, R * R).astype(np.int32)
    for axis in range(2):
        g = D.line_pass(g, axis, R)
    return (cls.astype(np.uint32) << np.uint32(30)) | g.astype(np.uint32), int(np.count_nonzero(site))


# ------------------------------------------------------------------------------------------------ hand-made voxels
def entries(shape):
    """(value, weight) arrays of a box nobody has seen"""
    return np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)


def pack(value, weight):
    v = np.asarray(value).astype(np.int16).astype(np.uint16).astype(np.uint32)
    w = np.asarray(weight).astype(np.int16).astype(np.uint16).astype(np.uint32)
    return v | (w << np.uint32(16))


def put_floor(value, weight, x, y, z, v0=-300, v1=300, free=8, w=5):
    """a floor at (x, y): OCCUPIED at z with value v0, FREE at z + 1 with value v1, FREE with value TAU up to z + free"""
    value[x, y, z], weight[x, y, z] = v0, w
    value[x, y, z + 1], weight[x, y, z + 1] = v1, w
    for k in range(2, free + 1):
        value[x, y, z + k], weight[x, y, z + k] = TAU, w
