"""ws_map_distance — the exact Euclidean distance field of a device map against a numpy model of the rules stated in
include/warpsense_hip.h, applied to ws_map_download / ws_map_extract_box of the same map.  Every comparison is bit for bit:
np.array_equal on the raw uint32 records.

The model is separable like the kernels, but it is a witness only because tests/test_distance_host.py holds it against a
brute-force minimum over all (voxel, site) pairs on every box shape, range and flag combination used here."""
import ctypes as C
import subprocess
import time

import numpy as np
import pytest

from distance_model import FLAGS, RANGES, RES, SIZES, TAU, check_inputs, draw_entries, model, model_box, same, seeds_for, sites_and_classes
from dropin_build import build_dropin
import query_model as QM
import surface_model as G
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


def boxes_of(lo, hi):
    """the whole window, an inner box, and a box one voxel thick per axis"""
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    out = {"window": (None, None), "inner": ((lo[0] + 2, lo[1] + 3, lo[2] + 1), (hi[0] - 4, hi[1] - 1, hi[2] - 2))}
    for k in range(3):
        a, b = list(lo), list(hi)
        a[k] = b[k] = lo[k] + (hi[k] - lo[k]) // 3
        out[f"thin {'xyz'[k]}"] = (tuple(a), tuple(b))
    return out


@pytest.mark.parametrize("size", SIZES)
def test_arbitrary_entries_match_the_model(size):
    """(through TSDFCuda directly: LocalMap forces odd sizes, the C ABI does not); rotated rings, both maps, every flag
    combination, every range, the window, an inner box and three thin ones"""
    import warpsense_amd as W
    n = int(np.prod(size))
    pos, off = (3, -2, 5), tuple((s // 2 + 1 + 2 * k) % s for k, s in enumerate(size))
    assert all(o != 0 for o in off)
    views = [W.DeviceMap(size, off, draw_entries(size, seeds_for(size, which)), pos) for which in (0, 1)]
    for v in views:
        check_inputs(v.data_, size)
    t = W.TSDFCuda(views[0], TAU, 640, RES)
    t.new_map().to_device(views[1])
    lo, hi = QM.window(size, pos)
    compared = 0
    for which in (0, 1):
        host = W.DeviceMap(size, off, np.empty(n, dtype=np.uint32), pos)
        QM.wrapper(t, which).to_host(host)
        assert np.array_equal(host.data_, views[which].data_)
        for name, (a, b) in boxes_of(lo, hi).items():
            for kw in FLAGS:
                for R in RANGES:
                    want, n_sites = model(host, R, a, b, **kw)
                    got = QM.wrapper(t, which).distance(lo=a, hi=b, max_dist_vox=R, **kw)
                    assert same(got, want) and QM.wrapper(t, which).last_sites == n_sites, (size, which, name, kw, R)
                    compared += 1
    assert compared == 2 * 5 * 8 * 5
    for which in (0, 1):  # read-only on the maps
        host = W.DeviceMap(size, off, np.empty(n, dtype=np.uint32), pos)
        QM.wrapper(t, which).to_host(host)
        assert np.array_equal(host.data_, views[which].data_)


def make_maps(size, seed):
    """as make_maps of test_gpu_surface.py, with this file's draw"""
    import warpsense_amd as W
    lm = W.LocalMap(*size, TAU, 0)
    shape = tuple(int(s) for s in lm.size)
    lm.data[:] = draw_entries(shape, seed)
    params = W.Params(W.MapParams(resolution=RES, max_distance=TAU / 1000.0, max_weight=10, size=tuple(s * RES / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    other = W.LocalMap(*size, TAU, 0)
    other.data[:] = draw_entries(shape, seed + 1000)
    tm.tsdf().new_map().to_device(other.device_map())
    return W, tm, lm


def test_rotated_rings_after_the_shift_sequence():
    """after the shift sequence of test_gpu_surface.py all three offsets are non-zero; both maps, the window and a box that
    crosses the ring's seam on every axis"""
    W, tm, lm = make_maps((21, 17, 13), seed=5)
    for new_pos in [(3, 0, 0), (3, -4, 2), (10, -4, 2), (10, 5, -3), (-2, 5, -3)]:
        tm.shift_map(new_pos)
        assert tm.tsdf().avg_map().distance(max_dist_vox=3).shape == (21, 17, 13)  # (a call between two shifts)
    for which in (0, 1):
        host = QM.download(W, tm, lm, which)
        assert all(int(o) != 0 for o in host.offset_) and list(host.pos_) == [-2, 5, -3]
        lo, hi = QM.window(host.size_, host.pos_)
        seam = [int(lo[k] + (-(lo[k] - host.pos_[k] + host.offset_[k])) % host.size_[k]) for k in range(3)]
        assert all(lo[k] < seam[k] <= hi[k] for k in range(3)), seam
        for a, b in ((None, None), (tuple(s - 2 for s in seam), tuple(s + 1 for s in seam))):
            for kw in FLAGS:
                for R in (3, 40):
                    want, n_sites = model(host, R, a, b, **kw)
                    assert same(QM.wrapper(tm.tsdf(), which).distance(lo=a, hi=b, max_dist_vox=R, **kw), want), (which, a, kw, R)
        assert model(host, 7)[1] >= 3


# ------------------------------------------------------------------------------------------------ fresh maps, columns
def test_fresh_map_zero_sites_and_unknown_occupied():
    import warpsense_amd as W
    lm = W.LocalMap(15, 17, 13, TAU, 0)  # every voxel (tau, 0): unknown
    t = W.TSDFCuda(lm.device_map(), TAU, 640, RES)
    avg = t.avg_map()
    n = C.c_size_t(99)
    assert t._L.ws_map_distance_dev(t.handle, C.byref(n)) is None and n.value == 0  # nothing before the first call
    for R in RANGES:
        rec = avg.distance(max_dist_vox=R)
        assert rec.shape == (15, 17, 13) and np.all(rec == R * R) and avg.last_sites == 0  # class 0, d2 = R^2
        col = avg.distance(max_dist_vox=R, columns=True)
        assert col.shape == (15, 17) and np.all(col == R * R) and avg.last_sites == 0
        assert not np.any(avg.distance(max_dist_vox=R, unknown_occupied=True)) and avg.last_sites == 15 * 17 * 13
        assert not np.any(avg.distance(max_dist_vox=R, unknown_occupied=True, columns=True)) and avg.last_sites == 15 * 17


def test_columns_with_a_column_whose_only_site_is_an_unknown_voxel():
    """15 x 15 x 15, every voxel free (value 20, weight 64) but: (4, 5, 6) occupied, (10, 3, 2) unknown, (12, 12, :) all of
    negative weight.  Height band z in [1, 8]."""
    import warpsense_amd as W
    size, pos, off = (15, 15, 15), (0, 0, 0), (7, 7, 7)
    value, weight = np.full(size, 20), np.full(size, 64)
    value[4, 5, 6] = -20
    weight[10, 3, 2] = 0
    weight[12, 12, :] = -3
    view = W.DeviceMap(size, off, W.pack_entry(value.reshape(-1), weight.reshape(-1)).astype(np.uint32), pos)
    # the arrays above are in storage order: world voxel = storage index - 7 with these offsets
    t = W.TSDFCuda(view, TAU, 640, RES)
    avg = t.avg_map()
    a, b = (-7, -7, -6), (7, 7, 1)
    for R in (3, 40):
        for kw in FLAGS:
            want, n_sites = model(view, R, a, b, **kw)
            got = avg.distance(lo=a, hi=b, max_dist_vox=R, **kw)
            assert same(got, want) and avg.last_sites == n_sites, (R, kw)
    col = avg.distance(lo=a, hi=b, max_dist_vox=40, columns=True, unknown_occupied=True)
    assert avg.last_sites == 3  # the occupied column, the column of the unknown voxel and the negative-weight column
    assert W.distance_class(col)[4, 5] == 2 and W.distance_class(col)[10, 3] == 0 and W.distance_class(col)[12, 12] == 0
    assert W.distance_d2(col)[4, 5] == 0 and W.distance_d2(col)[10, 3] == 0 and W.distance_d2(col)[10, 4] == 1 and W.distance_class(col)[10, 4] == 1
    col = avg.distance(lo=a, hi=b, max_dist_vox=40, columns=True)
    assert avg.last_sites == 1 and W.distance_d2(col)[10, 3] == 36 + 4 and W.distance_class(col)[10, 3] == 1 and W.distance_class(col)[12, 12] == 0
    col = avg.distance(lo=a, hi=b, max_dist_vox=40, columns=True, unknown_occupied=True, any_weight=True)
    assert avg.last_sites == 2 and W.distance_class(col)[12, 12] == 1


# ------------------------------------------------------------------------------------------------ buffers, errors
def test_repeatable_apart_from_the_other_results_downloads_and_error_codes():
    import mesh_model as M
    import raycast_model as RC
    W, tm, lm = make_maps((15, 15, 15), seed=22)
    t = tm.tsdf()
    avg, L = t.avg_map(), t._L
    before = [QM.download(W, tm, lm, which).data_.copy() for which in (0, 1)]
    rec = avg.distance(max_dist_vox=7)
    assert same(avg.distance(max_dist_vox=7), rec) and same(tm.distance_field(max_dist_m=0.35), rec)  # 350 mm / 50 mm = 7 voxels
    assert same(tm.distance_field(max_dist_m=0.301), rec) and not same(tm.distance_field(max_dist_m=0.3), rec)  # ceil
    dev = avg.distance(max_dist_vox=7, device=True)
    assert dev.is_cuda and tuple(dev.shape) == (15, 15, 15) and np.array_equal(dev.cpu().numpy().view(np.uint32), rec)
    # the results of the surface cloud, the mesh and the ray cast survive a distance call, and the other way round
    surf = avg.surface()
    vert, face = avg.mesh(any_weight=True)  # (half the weights are not positive: the default rule leaves hardly a valid cell)
    o, d = RC.random_rays((15, 15, 15), seed=3, lo=QM.window(lm.size, lm.pos)[0], n=300)
    rays, _ = avg.raycast(o, d.astype(np.int32), 3000)
    rec40 = avg.distance(max_dist_vox=40, unknown_occupied=True)
    n = C.c_size_t(0)
    got = np.zeros(len(surf), dtype=G.REC)
    assert L.ws_map_surface_download(t.handle, got.ctypes.data_as(C.c_void_p), None, len(surf), C.byref(n)) == 0 and QM.same(got, surf)
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    pv, pf = np.zeros(len(vert), dtype=M.VERT), np.zeros((len(face), 3), dtype=np.uint32)
    assert L.ws_map_mesh_download(t.handle, pv.ctypes.data_as(C.c_void_p), pf.ctypes.data_as(C.c_void_p), len(vert), len(face), C.byref(gv), C.byref(gf)) == 0
    assert M.same((pv, pf), (vert, face)) and len(vert) > 0
    pr = np.zeros(300, dtype=RC.RAY)
    assert L.ws_map_raycast_download(t.handle, pr.ctypes.data_as(C.c_void_p), None, 300, C.byref(n)) == 0 and QM.same(pr, rays)
    avg.surface(band=1)
    avg.mesh()
    avg.raycast(o, d[:10].astype(np.int32), 3000)
    # the download's prefix rule
    part = np.zeros(1000, dtype=np.uint32)
    assert L.ws_map_distance_download(t.handle, part.ctypes.data_as(C.c_void_p), 1000, C.byref(n)) == 0
    assert n.value == 15 ** 3 and np.array_equal(part, rec40.reshape(-1)[:1000])
    assert L.ws_map_distance_download(t.handle, None, 0, C.byref(n)) == 0 and n.value == 15 ** 3
    assert L.ws_map_distance_dev(t.handle, C.byref(n)) and n.value == 15 ** 3
    # both maps are bit-identical before and after
    for which in (0, 1):
        assert np.array_equal(QM.download(W, tm, lm, which).data_, before[which])
    # the error codes of the rules
    lo, hi = (np.asarray(v, dtype=np.int32) for v in QM.window(lm.size, lm.pos))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.ws_map_distance(t.handle, 0, None, None, 0, 0, None) == -5 and L.ws_map_distance(t.handle, 0, None, None, 256, 0, None) == -5  # WS_ERR_RANGE
    assert L.ws_map_distance(t.handle, 0, None, None, 1, 0, None) == 0 and L.ws_map_distance(t.handle, 0, None, None, 255, 0, None) == 0
    assert L.ws_map_distance(t.handle, 0, None, None, 7, 8, None) == -1 and L.ws_map_distance(t.handle, 2, None, None, 7, 0, None) == -1  # WS_ERR_INVALID
    out_lo = lo.copy()
    out_lo[0] -= 1
    assert L.ws_map_distance(t.handle, 0, p(out_lo), p(hi), 7, 0, None) == -1
    bad_hi = hi.copy()
    bad_hi[1] = lo[1] - 1
    assert L.ws_map_distance(t.handle, 0, p(lo), p(bad_hi), 7, 0, None) == -1 and L.ws_map_distance(t.handle, 0, p(lo), None, 7, 0, None) == -1
    assert L.ws_map_distance(t.handle, 0, p(lo), p(hi), 7, 0, None) == 0
    with pytest.raises(W.WsError):
        avg.distance(max_dist_vox=0)
    # the timing entry: four figures, the last one zero for columns
    ms = (C.c_float * 4)()
    assert L.ws_debug_distance_timing(t.handle, 1, None) == 0
    avg.distance(max_dist_vox=7)
    assert L.ws_debug_distance_timing(t.handle, -1, ms) == 0 and all(v > 0 for v in ms)
    assert L.ws_debug_distance_timing(t.handle, 0, ms) == 0


# ------------------------------------------------------------------------------------------------ maps made by the update
def test_after_two_scans_into_a_129_window():
    import torch
    import warpsense_amd as W
    tau, res, mw, size = 1000, 50, 640, (128, 128, 128)
    lm = W.LocalMap(*size, tau, 0)
    lm.offset[:] = (lm.size // 2 + np.array([-31, 17, 5])) % lm.size
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        pts = S.os1_128_scan(rings=64, azimuths=512, half_extents_mm=(2800.0, 2600.0, 1800.0), sensor_mm=sensor, seed=40 + k)
        pos = [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor]
        t.update_tsdf(torch.from_numpy(pts).cuda(), pos, (0, 0, 32768))
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    t.avg_map().to_host(host)
    assert model(host, 7)[1] > 10_000
    cases = [(8, kw) for kw in FLAGS] + [(R, kw) for R in RANGES for kw in (FLAGS[0], dict(any_weight=False, unknown_occupied=True, columns=True), dict(any_weight=True, unknown_occupied=False, columns=True))]
    for R, kw in cases:
        want, n_sites = model(host, R, **kw)
        got = t.avg_map().distance(max_dist_vox=R, **kw)
        assert same(got, want) and t.avg_map().last_sites == n_sites, (R, kw)
    after = np.empty_like(lm.data)
    t.avg_map().to_host(W.DeviceMap(lm.size.copy(), lm.offset.copy(), after, lm.pos.copy()))
    assert np.array_equal(after, host.data_)


def exact_at(site_xyz, samples):
    """min over ALL sites of |v - s|^2 for every sample, by pairs (not clamped)"""
    out = np.empty(len(samples), dtype=np.int64)
    s = site_xyz.astype(np.int32)
    for i, v in enumerate(samples.astype(np.int32)):
        d = s - v
        out[i] = int(np.min(np.einsum("ij,ij->i", d, d)))  # |d| <= 512: the sum fits int32
    return out


def test_after_real_scans_at_benchmark_size():
    """the benchmark's 513^3 map @ 50 mm after two OS1-128 scans: the whole window for R = 8 against the model; R = 40 and 255
    against the exact minimum over all sites at 4 096 sampled voxels"""
    import torch
    import warpsense_amd as W
    tau, res, mw, size = 1000, 50, 640, (512, 512, 512)
    lm = W.LocalMap(*size, tau, 0)
    lm.offset[:] = (lm.size // 2 + np.array([-226, -20, 11])) % lm.size
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        pos = [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor]
        t.update_tsdf(torch.from_numpy(pts).cuda(), pos, (0, 0, 32768))
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    t.avg_map().to_host(host)
    avg = t.avg_map()
    t0 = time.perf_counter()
    got = avg.distance(max_dist_vox=8)
    t1 = time.perf_counter()
    want, n_sites = model(host, 8)
    print(f"513^3 R = 8: distance() incl. download {t1 - t0:.3f} s, model {time.perf_counter() - t1:.1f} s, {n_sites} sites")
    assert n_sites > 100_000 and avg.last_sites == n_sites and same(got, want)
    assert same(avg.distance(max_dist_vox=8), got)  # the same bytes twice
    del want
    lo, hi = QM.window(host.size_, host.pos_)
    box = QM.ring_box(host.data_, host.size_, host.pos_, host.offset_, lo, hi)
    site, cls = sites_and_classes(box)
    site_xyz = np.argwhere(site)
    rng = np.random.default_rng(513)
    # half of them anywhere in the window, half within 20 voxels per axis of a site (d2 <= 1200 < 40^2)
    near = site_xyz[rng.integers(0, len(site_xyz), 2048)] + rng.integers(-20, 21, (2048, 3))
    samples = np.concatenate([rng.integers(0, 513, (2048, 3)), np.clip(near, 0, 512)])
    unclamped = exact_at(site_xyz, samples)
    for R in (40, 255):
        exact = np.minimum(unclamped, R * R)
        assert np.count_nonzero(exact < R * R) >= 1024, R  # at least a quarter within R of a site
        got = avg.distance(max_dist_vox=R)
        at = got[samples[:, 0], samples[:, 1], samples[:, 2]]
        print(f"R = {R}: {np.count_nonzero(exact < R * R)} of 4096 samples within R, {np.count_nonzero(exact == 0)} on a site")
        assert np.array_equal((at & np.uint32(0xFFFFFF)).astype(np.int64), exact)
        assert np.array_equal(at >> np.uint32(30), cls[samples[:, 0], samples[:, 1], samples[:, 2]])
        assert avg.last_sites == n_sites
    col = avg.distance(max_dist_vox=40, columns=True)
    want_col, n_cols = model_box(box, 40, columns=True)
    assert same(col, want_col) and avg.last_sites == n_cols
    after = np.empty_like(lm.data)
    avg.to_host(W.DeviceMap(lm.size.copy(), lm.offset.copy(), after, lm.pos.copy()))
    assert np.array_equal(after, host.data_)


# ------------------------------------------------------------------------------------------------ C++ twin
def test_cpp_twin_matches_the_python_route(tmp_path):
    import warpsense_amd as W
    exe = build_dropin("distance_dropin", tmp_path)
    tau, res, mw, edge = 1000, 50, 640, 65
    pts = S.os1_128_scan(rings=32, azimuths=256, half_extents_mm=(1400.0, 1300.0, 900.0), seed=2)
    pts.tofile(tmp_path / "scan.bin")
    out = subprocess.run([str(exe), str(tmp_path / "scan.bin"), str(len(pts)), str(edge), str(res), str(tau), str(mw)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    lm = W.LocalMap(edge, edge, edge, tau, 0)
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=(edge * res / 1000.0,) * 3))
    tm = W.TSDFMapping(params, lm)
    t = tm.tsdf()
    t.update_tsdf(pts, (0, 0, 0), (0, 0, 32768))
    avg = t.avg_map()

    def line(rec, sites):
        ext = rec.shape if rec.ndim == 3 else rec.shape + (1,)
        return [str(v) for v in ext] + [str(sites), f"{QM.fnv1a(rec.tobytes()):016x}"]
    rec = tm.distance_field(max_dist_m=1.0)  # 20 voxels
    assert avg.last_sites > 1000 and np.count_nonzero((W.distance_d2(rec) > 0) & (W.distance_d2(rec) < 400)) > 10_000
    assert lines["window"] == line(rec, avg.last_sites)
    a, b = (-(edge // 4), -3, -6), (edge // 4, edge // 3, 5)
    rec = avg.distance(lo=a, hi=b, max_dist_vox=7, unknown_occupied=True, any_weight=True)
    assert lines["box"] == line(rec, avg.last_sites)
    rec = tm.distance_field(lo=a, hi=b, max_dist_m=2.0, columns=True)
    assert rec.shape == (2 * (edge // 4) + 1, edge // 3 + 4) and lines["columns"] == line(rec, avg.last_sites)
    mm = W.distance_mm(rec, res)
    assert mm.dtype == np.float32 and np.array_equal(mm, np.float32(res) * np.sqrt(W.distance_d2(rec).astype(np.float32)))
