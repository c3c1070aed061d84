"""The numpy model of ws_map_sample and ws_store_sample (the rules stated in include/warpsense_hip.h): the record dtype and classes, the
model over a Ring or a Chunks field, and the points the tests sample."""
import itertools

import numpy as np

import query_model as QM
import raycast_model as R
import store_raycast_scenes as SH


TAU, RES = R.TAU, R.RES
SAMPLE = np.dtype([("d_mm", "<i4"), ("weight", "<i4"), ("cls", "<u4"), ("raw", "<u4")])
UNKNOWN, FREE, SURFACE, INSIDE = 0, 1, 2, 3
CLASS_NAMES = ("unknown", "free", "surface", "inside")


# ------------------------------------------------------------------------------------------------ the numpy model
def raws(fld, v):
    """(raw entry, the voxel lies in the field) of world voxels v (n, 3): inside the window of a Ring; in a present chunk and inside
    the box of a Chunks"""
    v = np.asarray(v, dtype=np.int64)
    if isinstance(fld, R.Ring):
        inside = np.all((v >= fld.lo) & (v <= fld.hi), axis=1)
        i = (np.clip(v, fld.lo, fld.hi) - fld.pos + fld.offset + fld.size) % fld.size
        return fld.data[i[:, 0], i[:, 1], i[:, 2]], inside
    code = SH._code(v >> 6, fld.base)
    i = np.minimum(np.searchsorted(fld.code, code), max(len(fld.code) - 1, 0))
    present = (fld.code[i] == code) if len(fld.code) else np.zeros(len(v), dtype=bool)
    if fld.lo is not None:
        present = present & np.all((v >= fld.lo) & (v <= fld.hi), axis=1)
    l = v & 63
    return fld.data[i, l[:, 0], l[:, 1], l[:, 2]], present


def model(fld, res, pts, band, any_weight=False, select=()):
    """(records, counts (4,) uint64, gradient (n, 3) int32, selection (k, 3) int32) of the rules; select: class numbers"""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 3)
    n = len(pts)
    dead = np.any(np.abs(pts) >= 2 ** 30, axis=1)
    p = np.where(dead[:, None], 0, pts)
    ok, T = R.field(fld, res, p, any_weight)
    ok &= ~dead
    b = (p - res // 2) // res
    wmin = np.full(n, 2 ** 31, dtype=np.int64)
    for c in itertools.product((0, 1), repeat=3):
        w = QM.unpack(raws(fld, b + np.array(c, dtype=np.int64))[0])[1].astype(np.int64)
        wmin = np.minimum(wmin, np.abs(w) if any_weight else w)
    d = np.where(ok, T // (res ** 3), 0)
    cls = np.where(ok, np.where(d >= band, FREE, np.where(d <= -band, INSIDE, SURFACE)), UNKNOWN)
    g = p // res
    raw_g, in_g = raws(fld, g)
    rec = np.zeros(n, dtype=SAMPLE)
    rec["d_mm"], rec["weight"], rec["cls"], rec["raw"] = d, np.where(ok, wmin, 0), cls, np.where(in_g & ~dead, raw_g, 0)
    grad = np.zeros((n, 3), dtype=np.int64)
    all_valid = ~dead
    for k in range(3):
        e = np.zeros(3, dtype=np.int64)
        e[k] = 1
        (va, oka), (vb, okb) = fld.entries(g + e, any_weight), fld.entries(g - e, any_weight)
        grad[:, k] = va - vb
        all_valid &= oka & okb
    grad[~all_valid] = 0
    counts = np.bincount(cls, minlength=4).astype(np.uint64)
    sel = pts[np.isin(cls, list(select))].astype(np.int32)
    return rec, counts, grad.astype(np.int32), sel


def same(got, want):
    """(records, counts, gradient | None, selection | None) against the model's four"""
    return (got[0].tobytes() == want[0].tobytes() and np.array_equal(np.asarray(got[1], dtype=np.uint64), want[1])
            and (got[2] is None or (got[2].dtype == np.int32 and got[2].tobytes() == want[2].tobytes()))
            and (got[3] is None or (got[3].dtype == np.int32 and got[3].shape == want[3].shape and got[3].tobytes() == want[3].tobytes())))


# ------------------------------------------------------------------------------------------------ inputs shared with the GPU tests
def draw_storage(size, seed, tau=TAU):
    """storage-order entries of a map: values uniform in [-tau, tau]; one weight in ten zero, one in ten negative"""
    import warpsense_amd as W
    rng = np.random.default_rng(seed)
    n = int(np.prod(size))
    value = rng.integers(-tau, tau + 1, n)
    u = rng.random(n)
    weight = np.where(u < 0.8, rng.integers(1, 641, n), np.where(u < 0.9, -rng.integers(1, 641, n), 0))
    return W.pack_entry(value, weight).astype(np.uint32)


def window_of(size, lo=R.RANDOM_LO):
    """(pos, offset) of a window whose first voxel is lo, with a ring rotated on every axis"""
    size = np.asarray(size, dtype=np.int64)
    return np.asarray(lo, dtype=np.int64) + size // 2, (size // 2 + np.array([3, 1, 2])) % size


def window_points(lo, hi, res, seed, n=2048):
    """n points drawn over the window [lo, hi] (world voxels) grown by two voxels per side; every corner of the window +-1 mm; points
    with f = 0 and f = res - 1 per axis; the dead-point components +-2^30"""
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    rng = np.random.default_rng(seed)
    h = res // 2
    pts = [rng.integers((lo - 2) * res, (hi + 3) * res, (n, 3))]
    # half of the random points on the sample lattice: d_mm is then the voxel's own value, which reaches beyond the band
    pts[0][::2] = (pts[0][::2] // res) * res + h
    corners = np.array([[(lo if c[k] == 0 else hi + 1)[k] * res for k in range(3)] for c in itertools.product((0, 1), repeat=3)], dtype=np.int64)
    pts += [corners + s for s in (-1, 0, 1)]
    mid = ((lo + hi) // 2) * res + h  # a lattice point: f = 0 on every axis
    for k in range(3):
        for f in (0, res - 1):
            q = mid.copy()
            q[k] += f
            pts.append(q[None, :])
    pts.append(np.array([[2 ** 30, 0, 0], [0, -2 ** 30, 0], [1, 2, 2 ** 30], [-2 ** 30, -2 ** 30, -2 ** 30], [2 ** 30 - 1, 0, 0], [0, -(2 ** 30 - 1), 0]], dtype=np.int64))
    return np.concatenate(pts).astype(np.int64)


RESOLUTIONS = (1, 2, 50, 64, 1024)  # 1: the store only (ws_map_create admits 2 .. 1024); the model is checked at all of them
WINDOW_RESOLUTIONS = RESOLUTIONS[1:]


def window_case(size, seed, res, which=0):
    """the fixture of a window test: (storage entries, pos, offset, Ring, points, band)"""
    pos, off = window_of(size)
    data = draw_storage(size, seed + 100 * which)
    ring = R.Ring(data, size, pos, off)
    return data, pos, off, ring, window_points(ring.lo, ring.hi, res, seed + res + 15000), TAU // 2


def store_points(seed, res=None, n=1536):
    """points of the seam-store tests: random over the eight chunk positions around the origin grown by two voxels; a slab of points
    across every chunk border (|coordinate| below two voxels on one axis); points in the absent chunk; points next to it"""
    import store_scenes as SM
    res = SM.RES if res is None else res
    rng = np.random.default_rng(seed)
    span = 66 * res
    pts = [rng.integers(-span, span, (n, 3))]
    for k in range(3):
        q = rng.integers(-span, span, (256, 3))
        q[:, k] = rng.integers(-2 * res, 2 * res, 256)
        pts.append(q)
    lo_abs = np.asarray(SM.ABSENT, dtype=np.int64) * 64 * res
    pts.append(lo_abs + rng.integers(0, 64 * res, (256, 3)))
    # within two voxels of the faces the absent chunk shares with its neighbours, from both sides
    for k in range(3):
        q = lo_abs + rng.integers(0, 64 * res, (256, 3))
        face = 0 if SM.ABSENT[k] == -1 else 0  # the face at coordinate 0 on every axis: the chunks meet at the origin
        q[:, k] = face + rng.integers(-2 * res, 2 * res, 256)
        pts.append(q)
    pts[0][::2] = (pts[0][::2] // res) * res + res // 2
    return np.concatenate(pts).astype(np.int64)
