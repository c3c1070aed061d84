"""ws_map_raycast — the ray cast of a device map (the rules are stated in include/warpsense_hip.h) against a numpy model of exactly
those rules applied to ws_map_download of the same map.  Everything is integer: every comparison is on the raw bytes of the records
and of the gradient.

The model walks every sample of every ray (vectorised over the rays, a loop over the samples); it shortens nothing."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_mesh as M
import test_gpu_surface as G
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
        value, weight = M.unpack(self.data[i[:, 0], i[:, 1], i[:, 2]])
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
    return G.same(got[0], want[0]) and (want[1] is None or G.same(got[1], want[1]))


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
    assert core.sum() > 1000 and np.all(hit[core])              # every ray that passes the centre within 0.8 R hits
    assert not np.any(hit & (imp > r_mm))                       # no ray whose line misses the sphere hits
    assert dist.max() <= bound and err.max() <= bound
    return int(core.sum()), float(dist.max()), float(err.max())


def upload(size, pos, off, raws, tau=TAU, mw=640, res=RES):
    """a TSDFCuda whose two maps hold the given storage-order entries"""
    import warpsense_amd as W
    views = [W.DeviceMap(size, off, np.ascontiguousarray(r, dtype=np.uint32).reshape(-1), pos) for r in raws]
    t = W.TSDFCuda(views[0], tau, mw, res)
    t.new_map().to_device(views[1])
    return t, views


# ------------------------------------------------------------------------------------------------ 6: arbitrary entries
@pytest.mark.parametrize("size", SIZES)
def test_arbitrary_entries_match_the_model(size):
    import torch
    pos, off = (0, 0, 0), tuple(s // 2 for s in size)
    t, views = upload(size, pos, off, [M.draw_entries(size, seed=M.seeds_for(size, which)) for which in (0, 1)])
    o, d = random_rays(size, seed=sum(size), lo=G.window(size, pos)[0])
    d_dev = torch.from_numpy(d.astype(np.int32)).cuda()
    tgt_dev = torch.from_numpy((o + d).astype(np.int32)).cuda()
    for which in (0, 1):
        for any_weight in (False, True):
            want = model_of(views[which], RES, o, d, 3000, any_weight)
            w = G.wrapper(t, which)
            n_hit = int(np.count_nonzero(want[0]["range_mm"] >= 0))
            print(size, which, any_weight, n_hit, int(np.count_nonzero(np.any(want[1] != 0, axis=1))))
            assert n_hit > 100
            assert same(w.raycast(o, d.astype(np.int32), 3000, any_weight=any_weight, gradient=True), want), (which, any_weight, "host")
            assert w.last_hits == n_hit
            assert same(w.raycast(o, d_dev, 3000, any_weight=any_weight, gradient=True), want), (which, any_weight, "dev")
            assert same(w.raycast(o, tgt_dev, 3000, any_weight=any_weight, gradient=True, targets=True), want), (which, any_weight, "targets")
            assert same(w.raycast(o, (o + d).astype(np.int32), 3000, any_weight=any_weight, targets=True), (want[0], None))


# ------------------------------------------------------------------------------------------------ 7: rotated rings
def test_rotated_rings_after_the_shift_sequence():
    W, tm, lm = M.make_maps((21, 17, 13), seed=5)
    for new_pos in [(3, 0, 0), (3, -4, 2), (10, -4, 2), (10, 5, -3), (-2, 5, -3)]:
        tm.shift_map(new_pos)
    rng = np.random.default_rng(11)
    for which in (0, 1):
        host = G.download(W, tm, lm, which)
        assert all(int(o) != 0 for o in host.offset_) and list(host.pos_) == [-2, 5, -3]
        lo, hi = G.window(host.size_, host.pos_)
        centre = ((lo + hi + 1) * RES // 2).astype(np.int64)
        big = 2 ** 30 - 1
        special = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0], [big, big, -big], [-big, 3, big], [big, -big, 7], [2 ** 30, 1, 1],
                            [0, 0, 0], [-2 ** 31, 0, 0]], dtype=np.int64)
        d = np.concatenate([rng.integers(-32768, 32769, (1024, 3)), special])
        outside = np.array([lo[0] * RES - 400, centre[1] + 30, centre[2] - 20], dtype=np.int64)  # origin outside the window, rays run into it
        d_out = np.concatenate([np.abs(rng.integers(-32768, 32769, (512, 1))) + 20000, rng.integers(-12000, 12001, (512, 2))], axis=1)
        n_hits = 0
        for o, dd in ((centre, d), (outside, d_out)):
            for any_weight in (False, True):
                want = model_of(host, RES, o, dd, 3000, any_weight)
                n_hits += int(np.count_nonzero(want[0]["range_mm"] >= 0))
                got = G.wrapper(tm.tsdf(), which).raycast(o, dd.astype(np.int32), 3000, any_weight=any_weight, gradient=True)
                assert same(got, want), (which, any_weight, o)
            if o is centre:
                # the ring's seam lies inside the window on every axis, where rays in all directions cross it; hits whose cell
                # straddles a seam exist on at least one axis (the slabs the shifts brought in are unobserved)
                hit = want[0]["range_mm"] >= 0
                p = np.stack([want[0]["x_mm"], want[0]["y_mm"], want[0]["z_mm"]], axis=1)[hit] // RES
                seam = [int(lo[k] + (-(lo[k] - host.pos_[k] + host.offset_[k])) % host.size_[k]) for k in range(3)]
                assert all(lo[k] < seam[k] <= hi[k] for k in range(3)), seam
                at_seam = [int(np.count_nonzero((p[:, k] >= seam[k] - 1) & (p[:, k] <= seam[k]))) for k in range(3)]
                print("hits at the seam per axis", at_seam)
                assert max(at_seam) > 0
        print(which, n_hits)
        assert n_hits > 1000
        assert int(np.count_nonzero(model_of(host, RES, outside, d_out, 3000, True)[0]["range_mm"] >= 0)) > 50


# ------------------------------------------------------------------------------------------------ 8: the sphere
def test_sphere_on_the_device_through_the_mapping():
    import warpsense_amd as W
    for edge, centre, radius in M.SPHERES:
        box = M.sphere_box(edge, centre, radius).reshape((edge,) * 3)
        lm = W.LocalMap(edge + 1, edge + 1, edge + 1, TAU, 0)  # (odd sizes: the sphere's box and one plane of unobserved voxels)
        lm.pos[:] = np.asarray(M.SPHERE_LO) + lm.size // 2
        lm.offset[:] = (3, edge - 2, edge // 2)  # a rotated ring
        store = lm.data.reshape(tuple(int(s) for s in lm.size))
        ax = [(np.arange(M.SPHERE_LO[k], M.SPHERE_LO[k] + edge) - lm.pos[k] + lm.offset[k] + lm.size[k]) % lm.size[k] for k in range(3)]
        store[np.ix_(*ax)] = box
        tm = W.TSDFMapping(W.Params(W.MapParams(resolution=RES, max_distance=TAU / 1000.0, max_weight=10, size=tuple(int(s) * RES / 1000.0 for s in lm.size))), lm)
        o, d, c_mm = sphere_rays(centre, radius)
        pose = np.eye(4)
        pose[:3, 3] = o / 1000.0
        rec, grad = tm.raycast(pose, d.astype(np.float64), 4000, gradient=True)
        oi, di = W.TSDFMapping.raycast_rays(pose, d.astype(np.float64))
        assert np.array_equal(oi, o) and np.all(np.max(np.abs(di), axis=1) == 2 ** 20)
        want = model(Ring(lm.data, lm.size, lm.pos, lm.offset), RES, oi, di, 4000)
        assert same((rec, grad), want) and same((rec, grad), model(Ring.of_box(box, M.SPHERE_LO), RES, oi, di, 4000))
        check_sphere(rec, o, di.astype(np.int64), c_mm, radius * RES)
        # the gradient points away from the centre at every hit
        hit = rec["range_mm"] >= 0
        p = np.stack([rec["x_mm"], rec["y_mm"], rec["z_mm"]], axis=1)[hit].astype(np.float64) - c_mm
        g = grad[hit].astype(np.float64)
        cos = (p * g).sum(axis=1) / (np.linalg.norm(p, axis=1) * np.maximum(np.linalg.norm(g, axis=1), 1e-9))
        assert np.all(np.any(grad[hit] != 0, axis=1)) and cos.min() > 0.95, cos.min()


# ------------------------------------------------------------------------------------------------ 9: repeatability, buffers, errors
def test_repeatable_partial_downloads_and_error_codes():
    import warpsense_amd as W
    size = (15, 15, 15)
    W_, tm, lm = M.make_maps(size, seed=21)
    t = tm.tsdf()
    avg = t.avg_map()
    L = t._L
    o, d = random_rays(size, seed=3, lo=G.window(lm.size, lm.pos)[0], n=700)
    d = d.astype(np.int32)
    rec, grad = avg.raycast(o, d, 3000, gradient=True)
    assert same(avg.raycast(o, d, 3000, gradient=True), (rec, grad)) and avg.last_hits == np.count_nonzero(rec["range_mm"] >= 0) > 100
    n = C.c_size_t(0)
    assert L.ws_map_raycast_records_dev(t.handle, C.byref(n)) and n.value == 700
    assert L.ws_map_raycast_gradient_dev(t.handle, C.byref(n)) and n.value == 700
    # a surface-cloud call and a mesh call between the ray cast and its download do not disturb it, and the other way round
    surf = avg.surface()
    vert, face = avg.mesh()
    part_r, part_g = np.zeros(233, dtype=RAY), np.zeros((233, 3), dtype=np.int32)
    assert L.ws_map_raycast_download(t.handle, part_r.ctypes.data_as(C.c_void_p), part_g.ctypes.data_as(C.c_void_p), 233, C.byref(n)) == 0
    assert n.value == 700 and G.same(part_r, rec[:233]) and G.same(part_g, grad[:233])
    assert L.ws_map_raycast_download(t.handle, None, None, 0, C.byref(n)) == 0 and n.value == 700
    avg.raycast(o, d[:100], 3000)
    got = np.zeros(len(surf), dtype=G.REC)
    assert L.ws_map_surface_download(t.handle, got.ctypes.data_as(C.c_void_p), None, len(surf), C.byref(n)) == 0 and G.same(got, surf)
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    pv, pf = np.zeros(len(vert), dtype=M.VERT), np.zeros((len(face), 3), dtype=np.uint32)
    assert L.ws_map_mesh_download(t.handle, pv.ctypes.data_as(C.c_void_p), pf.ctypes.data_as(C.c_void_p), len(vert), len(face), C.byref(gv), C.byref(gf)) == 0
    assert M.same((pv, pf), (vert, face))
    # without WS_RAYCAST_GRADIENT there is no gradient to fetch
    assert L.ws_map_raycast_gradient_dev(t.handle, C.byref(n)) is None and n.value == 0
    assert L.ws_map_raycast_download(t.handle, part_r.ctypes.data_as(C.c_void_p), part_g.ctypes.data_as(C.c_void_p), 50, C.byref(n)) == -1
    # n == 0: WS_OK, nothing
    r0, g0 = avg.raycast(o, np.zeros((0, 3), dtype=np.int32), 3000, gradient=True)
    assert r0.shape == (0,) and g0.shape == (0, 3) and L.ws_map_raycast_records_dev(t.handle, C.byref(n)) is None and n.value == 0
    # the error codes of the rules
    o3 = np.asarray(o, dtype=np.int32)
    call = lambda origin, count, rng, flags=0: L.ws_map_raycast(t.handle, 0, origin.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), count, rng, flags, None)
    assert call(o3, 10, 0) == -1 and call(o3, 10, -5) == -1 and call(o3, 10, 100, 8) == -1     # WS_ERR_INVALID
    far = np.array([0, 2 ** 31 - 1 - 3000 - 2 * RES + 1, 0], dtype=np.int32)
    assert call(far, 10, 3000) == -5                                                            # WS_ERR_RANGE
    edge_o = np.array([0, -(2 ** 31 - 1 - 3000 - 2 * RES), 0], dtype=np.int32)
    assert call(edge_o, 10, 3000) == 0
    assert call(o3, 2 ** 27 + 1, 3000) == -5
    coarse = W.LocalMap(15, 15, 15, TAU, 0)
    t2 = W.TSDFCuda(coarse.device_map(), 3000, 640, 1025)
    with pytest.raises(W.WsError):
        t2.avg_map().raycast(o, d[:10], 3000)
    # an empty map: every ray a no-hit
    r1, g1 = W.TSDFCuda(coarse.device_map(), TAU, 640, RES).avg_map().raycast(o, d, 3000, any_weight=True, gradient=True)
    assert np.all(r1["range_mm"] == -1) and not np.any(g1) and not np.any(r1["x_mm"])


# ------------------------------------------------------------------------------------------------ 10: after real scans
def test_after_real_scans_at_benchmark_size():
    """The 513^3 map @ 50 mm after two OS1-128 scans of the box room (the set-up of test_gpu_mesh's test of this name).
    (a) every 16th ray of the first scan against the model on the downloaded map, byte for byte.
    (b) scan_residual of the first scan (all 131 072 points) at the pose it was taken from: at least half of the rays hit and the
    median absolute residual is at most one voxel (50 mm).  Computed beforehand without a GPU with the oracle's update
    (tests/oracle_lib.py) and this file's model:
      a 129^3 map @ 50 mm, one 128 x 256 scan of a (2 800, 2 600, 1 800) mm room: 7 290 of 32 768 rays hit (22 %: 256 azimuths are
        69 mm apart at the walls, wider than a voxel, so most cells there have an unobserved corner), median |residual| 33.8 mm;
        with 32 rings 178 of 8 192.  A small room is not the denser input: the scan must be dense, so the input stays the
        benchmark's 128 x 1024 scan;
      this test's own maps (513^3, the two scans) from the oracle, every 16th ray of the first scan: 5 142 of 8 192 hit (62.8 %),
        median |residual| 49.4 mm, signed median -32.6 mm, 95th percentile 253 mm.
    On the MI355X, all 131 072 rays: 63.3 % hit, median |residual| 48.9 mm -- inside the bound by one millimetre."""
    import torch
    import warpsense_amd as W
    tau, res, mw, size = 1000, 50, 640, (512, 512, 512)
    lm = W.LocalMap(*size, tau, 0)
    lm.offset[:] = (lm.size // 2 + np.array([-226, -20, 11])) % lm.size
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(s * res / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    t = tm.tsdf()
    scans = []
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        scans.append(pts)
        pos = [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor]
        t.update_tsdf(torch.from_numpy(pts).cuda(), pos, (0, 0, 32768))
    reg = W.RegistrationCuda(None)
    reg.prepare_registration(torch.from_numpy(S.transform_points_mm(S.os1_128_scan(), S.perturbation())).cuda())
    T0, it0 = reg.register_cloud(t.device_map(), np.eye(4, dtype=np.float32), 200, 0.1, 0.03, res)
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    t.avg_map().to_host(host)
    # (a)
    o = np.zeros(3, dtype=np.int64)
    sub = scans[0][::16].astype(np.int64)
    assert len(sub) == 8192
    want = model_of(host, res, o, sub, 12000)
    n_hit = int(np.count_nonzero(want[0]["range_mm"] >= 0))
    print("model hits", n_hit, "of", len(sub))
    assert n_hit > 4096
    assert same(t.avg_map().raycast(o, sub.astype(np.int32), 12000, gradient=True), want)
    assert same(t.avg_map().raycast(o, torch.from_numpy(sub.astype(np.int32)).cuda(), 12000, gradient=True, targets=True), want)
    # (b)
    pts_dev = torch.from_numpy(scans[0]).cuda()
    resid = tm.scan_residual(pts_dev, np.eye(4))
    assert resid.shape == (131072,) and np.array_equal(np.isnan(resid), np.isnan(tm.scan_residual(scans[0], np.eye(4))))
    hit = ~np.isnan(resid)
    med = float(np.median(np.abs(resid[hit])))
    print("scan_residual: hit share", hit.mean(), "median |residual| mm", med, "p95", float(np.percentile(np.abs(resid[hit]), 95)))
    assert hit.mean() >= 0.5
    assert med <= res
    # the whole pattern from the pose, the default range: the same bytes twice, and the maps are left alone
    rec, grad = tm.raycast(np.eye(4), gradient=True)
    assert len(rec) == 131072 and same(tm.raycast(np.eye(4), gradient=True), (rec, grad)) and np.count_nonzero(rec["range_mm"] >= 0) > 65536
    T1, it1 = reg.register_cloud(t.device_map(), np.eye(4, dtype=np.float32), 200, 0.1, 0.03, res)
    assert it1 == it0 and it0 > 50 and np.array_equal(T0, T1)


# ------------------------------------------------------------------------------------------------ 11: C++ twin
def test_cpp_twin_matches_the_python_route(tmp_path):
    import warpsense_amd as W
    cxx = shutil.which("g++")
    assert cxx is not None, "the C++ drop-in needs g++"
    exe = tmp_path / "raycast_dropin"
    lib = os.path.join(ROOT, "warpsense_amd")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}",
                           os.path.join(ROOT, "tests", "cpp", "raycast_dropin.cpp"), "-o", str(exe), f"-L{lib}", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-lwarpsense_hip", "-lpthread"])
    tau, res, mw, edge = 1000, 50, 640, 65
    pts = S.os1_128_scan(rings=32, azimuths=256, half_extents_mm=(1400.0, 1300.0, 900.0), seed=2)
    pts.tofile(tmp_path / "scan.bin")
    out = subprocess.run([str(exe), str(tmp_path / "scan.bin"), str(len(pts)), str(edge), str(res), str(tau), str(mw)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    lm = W.LocalMap(edge, edge, edge, tau, 0)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    t.update_tsdf(pts, (0, 0, 0), (0, 0, 32768))
    rec, grad = t.avg_map().raycast((0, 0, 0), pts, 3000, gradient=True)  # the scan's points as directions
    hits = int(np.count_nonzero(rec["range_mm"] >= 0))
    assert hits > 4096
    assert lines["dirs"] == [str(len(rec)), str(hits), f"{G.fnv1a(rec.tobytes()):016x}", f"{G.fnv1a(grad.tobytes()):016x}"]
    rec2, _ = t.avg_map().raycast((10, -20, 5), pts, 3000, any_weight=True, targets=True)
    hits2 = int(np.count_nonzero(rec2["range_mm"] >= 0))
    assert hits2 > 4096 and not G.same(rec2, rec)
    assert lines["targets"] == [str(len(rec2)), str(hits2), f"{G.fnv1a(rec2.tobytes()):016x}", "-"]
