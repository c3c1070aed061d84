"""ws_map_raycast — the ray cast of a device map (the rules are stated in include/warpsense_hip.h) against a numpy model of exactly
those rules applied to ws_map_download of the same map.  Everything is integer: every comparison is on the raw bytes of the records
and of the gradient.

The model walks every sample of every ray (vectorised over the rays, a loop over the samples); it shortens nothing."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import mesh_model as M
import query_model as QM
from raycast_model import RAY, RES, Ring, SIZES, TAU, check_sphere, model, model_of, random_rays, same, sphere_rays, upload
import surface_model as G
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 6: arbitrary entries
@pytest.mark.parametrize("size", SIZES)
def test_arbitrary_entries_match_the_model(size):
    import torch
    pos, off = (0, 0, 0), tuple(s // 2 for s in size)
    t, views = upload(size, pos, off, [M.draw_entries(size, seed=M.seeds_for(size, which)) for which in (0, 1)])
    o, d = random_rays(size, seed=sum(size), lo=QM.window(size, pos)[0])
    d_dev = torch.from_numpy(d.astype(np.int32)).cuda()
    tgt_dev = torch.from_numpy((o + d).astype(np.int32)).cuda()
    for which in (0, 1):
        for any_weight in (False, True):
            want = model_of(views[which], RES, o, d, 3000, any_weight)
            w = QM.wrapper(t, which)
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
        host = QM.download(W, tm, lm, which)
        assert all(int(o) != 0 for o in host.offset_) and list(host.pos_) == [-2, 5, -3]
        lo, hi = QM.window(host.size_, host.pos_)
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
                got = QM.wrapper(tm.tsdf(), which).raycast(o, dd.astype(np.int32), 3000, any_weight=any_weight, gradient=True)
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
    o, d = random_rays(size, seed=3, lo=QM.window(lm.size, lm.pos)[0], n=700)
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
    assert n.value == 700 and QM.same(part_r, rec[:233]) and QM.same(part_g, grad[:233])
    assert L.ws_map_raycast_download(t.handle, None, None, 0, C.byref(n)) == 0 and n.value == 700
    avg.raycast(o, d[:100], 3000)
    got = np.zeros(len(surf), dtype=G.REC)
    assert L.ws_map_surface_download(t.handle, got.ctypes.data_as(C.c_void_p), None, len(surf), C.byref(n)) == 0 and QM.same(got, surf)
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
    exe = build_dropin("raycast_dropin", tmp_path)
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
    assert lines["dirs"] == [str(len(rec)), str(hits), f"{QM.fnv1a(rec.tobytes()):016x}", f"{QM.fnv1a(grad.tobytes()):016x}"]
    rec2, _ = t.avg_map().raycast((10, -20, 5), pts, 3000, any_weight=True, targets=True)
    hits2 = int(np.count_nonzero(rec2["range_mm"] >= 0))
    assert hits2 > 4096 and not QM.same(rec2, rec)
    assert lines["targets"] == [str(len(rec2)), str(hits2), f"{QM.fnv1a(rec2.tobytes()):016x}", "-"]
