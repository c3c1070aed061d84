"""The numpy model of ws_map_raycast (the rules stated in include/warpsense_hip.h): the record dtype, the field over a ring, the march,
and the random and sphere rays the tests cast."""
import math

import numpy as np

import mesh_model as M
import query_model as QM
import surface_model as G


RAY = np.dtype([("x_mm", "<i4"), ("y_mm", "<i4"), ("z_mm", "<i4"), ("range_mm", "<i4")])
TAU, RES = G.TAU, G.RES
SIZES = G.SIZES


# ------------------------------------------------------------------------------------------------ the numpy model
def tdiv(a, b):
    """C division (towards zero) of int64 arrays, b > 0"""
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


class Ring:
    """a map as ws_map_download gives it: entries in storage order, read through HDF5LocalMap::get_index"""

    def __init__(self, data, size, pos, offset):
        self.size, self.pos, self.offset = (np.asarray(v, dtype=np.int64).reshape(3) for v in (size, pos, offset))
        self.data = np.asarray(data, dtype=np.uint32).reshape(tuple(int(s) for s in self.size))
        self.lo = self.pos - self.size // 2
        self.hi = self.lo + self.size - 1

    @classmethod
    def of_box(cls, box, lo):
        """a dense box of raw entries, box[ix, iy, iz] = the voxel lo + (ix, iy, iz), as a window"""
        size = np.asarray(box.shape, dtype=np.int64)
        return cls(box, size, np.asarray(lo, dtype=np.int64) + size // 2, size // 2)

    def entries(self, v, any_weight):
        """(value, valid) of world voxels v (n, 3): valid iff inside the window and observed under the weight rule"""
        inside = np.all((v >= self.lo) & (v <= self.hi), axis=1)
        vc = np.clip(v, self.lo, self.hi)
        i = (vc - self.pos + self.offset + self.size) % self.size
        value, weight = QM.unpack(self.data[i[:, 0], i[:, 1], i[:, 2]])
        value, weight = value.astype(np.int64), weight.astype(np.int64)
        return value, inside & ((weight != 0) if any_weight else (weight > 0))


def field(ring, res, p, any_weight):
    """(cell valid, T) at points p (n, 3) int64 mm"""
    h = res // 2
    q = p - h
    b = q // res
    f = q - b * res
    ok = np.ones(len(p), dtype=bool)
    T = np.zeros(len(p), dtype=np.int64)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                value, valid = ring.entries(b + np.array([cx, cy, cz], dtype=np.int64), any_weight)
                w = (f[:, 0] if cx else res - f[:, 0]) * (f[:, 1] if cy else res - f[:, 1]) * (f[:, 2] if cz else res - f[:, 2])
                ok &= valid
                T += value * w
    return ok, T


def model(ring, res, origin, dirs, max_range, any_weight=False, targets=False):
    """(records, gradient (n, 3) int32) of the rules, for every ray the whole walk k = 0 .. K"""
    o = np.asarray(origin, dtype=np.int64).reshape(3)
    d = np.asarray(dirs, dtype=np.int64).reshape(-1, 3)
    if targets:
        d = d - o
    n = len(d)
    L = np.array([math.isqrt(int(x) * int(x) + int(y) * int(y) + int(z) * int(z)) for x, y, z in d], dtype=np.int64).reshape(n)
    live = (L > 0) & np.all(np.abs(d) < 2 ** 30, axis=1)
    d = np.where(live[:, None], d, 0)
    Ls = np.where(live, L, 1)[:, None]
    step = max(res // 2, 1)
    K = max_range // step
    rec = np.zeros((n, 4), dtype=np.int64)
    rec[:, 3] = -1
    done = ~live
    prev_ok, prev_T = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    for k in range(K + 1):
        ok, T = field(ring, res, o + tdiv(d * (k * step), Ls), any_weight)
        hit = ~done & prev_ok & (prev_T > 0) & ok & (T <= 0)
        if hit.any():
            t = (k - 1) * step + (step * prev_T[hit]) // (prev_T[hit] - T[hit])
            rec[hit, 3] = t
            rec[hit, :3] = o + tdiv(d[hit] * t[:, None], Ls[hit])
            done |= hit
        prev_ok, prev_T = ok, T
    got = rec[:, 3] >= 0
    g = rec[:, :3] // res
    grad = np.zeros((n, 3), dtype=np.int64)
    all_valid = got.copy()
    for k in range(3):
        e = np.zeros(3, dtype=np.int64)
        e[k] = 1
        (va, oka), (vb, okb) = ring.entries(g + e, any_weight), ring.entries(g - e, any_weight)
        grad[:, k] = va - vb
        all_valid &= oka & okb
    grad[~all_valid] = 0
    out = np.empty(n, dtype=RAY)
    for k, name in enumerate(RAY.names):
        out[name] = rec[:, k]
    return out, grad.astype(np.int32)


def model_of(host, *args, **kw):
    return model(Ring(host.data_, host.size_, host.pos_, host.offset_), *args, **kw)


def same(got, want):
    return QM.same(got[0], want[0]) and (want[1] is None or QM.same(got[1], want[1]))


# ------------------------------------------------------------------------------------------------ inputs shared with the host tests
RANDOM_MAPS = [((21, 17, 13), 5), ((33, 33, 33), 7)]
RANDOM_LO = (-7, 2, -3)


def random_rays(size, seed, lo=RANDOM_LO, n=2048, res=RES):
    """origin at the window's centre, directions uniform in [-32768, 32768]^3"""
    rng = np.random.default_rng(seed)
    o = ((np.asarray(lo) + np.asarray(size) / 2) * res).astype(np.int64)
    return o, rng.integers(-32768, 32769, (n, 3))


def sphere_rays(centre, radius, n=4096, res=RES):
    """origin at (SPHERE_LO + 1.5) res, rays towards centre + N(0, (0.9 R)^2) points"""
    lo = np.asarray(M.SPHERE_LO)
    c_mm = (lo + np.asarray(centre)) * res
    o = ((lo + 1.5) * res).astype(np.int64)
    tgt = c_mm + np.random.default_rng(1).normal(size=(n, 3)) * radius * res * 0.9
    return o, np.round(tgt - o).astype(np.int64), c_mm


def check_sphere(rec, o, d, c_mm, r_mm, bound=RES / 10):
    """the conditions of a ray cast of a sphere map; returns (rays within 0.8 R, largest distance to the sphere, largest range error).
    bound: of the two errors in mm, measured for the resolution of the map (res / 10 = 5 mm at res 50)"""
    hit = rec["range_mm"] >= 0
    u = d / np.linalg.norm(d.astype(np.float64), axis=1)[:, None]
    oc = (o - c_mm).astype(np.float64)
    bq = (u * oc).sum(axis=1)
    imp = np.sqrt(np.maximum((oc ** 2).sum() - bq ** 2, 0))  # distance of the ray's line from the centre
    core = imp <= 0.8 * r_mm
    analytic = -bq - np.sqrt(np.maximum(r_mm ** 2 - imp ** 2, 0))
    p = np.stack([rec["x_mm"], rec["y_mm"], rec["z_mm"]], axis=1).astype(np.float64)
    dist = np.abs(np.sqrt(((p[hit] - c_mm) ** 2).sum(axis=1)) - r_mm)
    err = np.abs(rec["range_mm"][core & hit] - analytic[core & hit])
    print("sphere", r_mm, "core", int(core.sum()), "hits", int(hit.sum()), "dist max", dist.max(), "range err max", err.max())
    assert core.sum() > 1000 and np.all(hit[core]), (core.sum(), np.count_nonzero(hit[core]))              # every ray that passes the centre within 0.8 R hits
    assert not np.any(hit & (imp > r_mm)), np.count_nonzero(hit & (imp > r_mm))                       # no ray whose line misses the sphere hits
    assert dist.max() <= bound and err.max() <= bound, (dist.max(), err.max(), bound)
    return int(core.sum()), float(dist.max()), float(err.max())


def upload(size, pos, off, raws, tau=TAU, mw=640, res=RES):
    """a TSDFCuda whose two maps hold the given storage-order entries"""
    import warpsense_amd as W
    views = [W.DeviceMap(size, off, np.ascontiguousarray(r, dtype=np.uint32).reshape(-1), pos) for r in raws]
    t = W.TSDFCuda(views[0], tau, mw, res)
    t.new_map().to_device(views[1])
    return t, views
