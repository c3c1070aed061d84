"""ws_map_mesh — a triangle mesh of a device map by naive surface nets (the rules are stated in include/warpsense_hip.h) against a
numpy model of exactly those rules applied to ws_map_download / ws_map_extract_box of the same map.  Everything is integer:
every comparison is on the raw bytes of the vertex records and of the face indices."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

from dropin_build import build_dropin
from mesh_model import RES, SIZES, SPHERES, SPHERE_LO, TAU, VERT, cell_masks, check_inputs, draw_entries, make_maps, mesh_report, model, model_box, quad_masks, same, seeds_for, sphere_box
import query_model as QM
import surface_model as G
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size", SIZES)
def test_arbitrary_entries_match_the_model(size):
    import warpsense_amd as W
    n = int(np.prod(size))
    pos, off = (0, 0, 0), tuple(s // 2 for s in size)
    views = [W.DeviceMap(size, off, draw_entries(size, seed=seeds_for(size, which)), pos) for which in (0, 1)]
    for v in views:
        check_inputs(v.data_, size)
    t = W.TSDFCuda(views[0], TAU, 640, RES)
    t.new_map().to_device(views[1])
    for which in (0, 1):
        host = W.DeviceMap(size, off, np.empty(n, dtype=np.uint32), pos)
        QM.wrapper(t, which).to_host(host)
        assert np.array_equal(host.data_, views[which].data_)
        for any_weight in (False, True):
            got = QM.wrapper(t, which).mesh(any_weight=any_weight)
            want = model(host, RES, any_weight=any_weight)
            print(size, which, any_weight, len(want[0]), len(want[1]))
            assert len(want[0]) > 100 and len(want[1]) > 100 and same(got, want), (size, which, any_weight)


def test_rotated_rings_after_the_shift_sequence():
    W, tm, lm = make_maps((21, 17, 13), seed=5)
    for new_pos in [(3, 0, 0), (3, -4, 2), (10, -4, 2), (10, 5, -3), (-2, 5, -3)]:
        tm.shift_map(new_pos)
        assert tm.tsdf().avg_map().mesh()[0].dtype == VERT  # (a call between two shifts: the buffers follow the window)
    for which in (0, 1):
        host = QM.download(W, tm, lm, which)
        assert all(int(o) != 0 for o in host.offset_) and list(host.pos_) == [-2, 5, -3]
        for any_weight in (False, True):
            got = QM.wrapper(tm.tsdf(), which).mesh(any_weight=any_weight)
            want = model(host, RES, any_weight=any_weight)
            assert len(want[0]) > 100 and len(want[1]) > 100 and same(got, want), (which, any_weight)


def test_boxes():
    """a ring rotated on every axis around a window that is not at the origin, every voxel drawn (through TSDFCuda directly)"""
    import warpsense_amd as W
    size, pos, off = (21, 17, 13), (10, 5, -3), (5, 11, 9)
    data = draw_entries(size, seed=9)
    check_inputs(data, size)
    host = W.DeviceMap(size, off, data, pos)
    t = W.TSDFCuda(host, TAU, 640, RES)
    avg = t.avg_map()
    lo, hi = QM.window(host.size_, host.pos_)
    whole = avg.mesh()
    assert same(whole, avg.mesh(lo=lo, hi=hi)) and same(whole, model(host, RES))
    seam = [int(lo[k] + (-(lo[k] - host.pos_[k] + host.offset_[k])) % host.size_[k]) for k in range(3)]
    assert all(lo[k] < seam[k] <= hi[k] for k in range(3)), seam
    boxes = {
        "one voxel thick": ((lo[0], lo[1], 0), (hi[0], hi[1], 0)),
        "one voxel": ((5, 3, -2), (5, 3, -2)),
        "two voxels thick": ((lo[0], seam[1] - 1, lo[2]), (hi[0], seam[1], hi[2])),
        "starts and ends mid-column": ((lo[0] + 2, lo[1] + 3, lo[2] + 1), (hi[0] - 4, hi[1] - 1, hi[2] - 2)),
        "crosses the wrap on every axis": (tuple(s - 2 for s in seam), tuple(s + 1 for s in seam)),
        "one cell column": ((lo[0], hi[1] - 1, lo[2]), (lo[0] + 1, hi[1], hi[2])),
    }
    nonempty = with_vertices = 0
    for name, (a, b) in boxes.items():
        for any_weight in (False, True):
            got = avg.mesh(lo=a, hi=b, any_weight=any_weight)
            want = model(host, RES, a, b, any_weight)
            assert same(got, want), (name, any_weight)
            assert len(got[1]) == 0 or int(got[1].max()) < len(got[0])  # faces of a box refer to vertices of that box
            nonempty += len(want[1]) > 0
            with_vertices += len(want[0]) > 0
            if "one voxel" in name:
                assert len(got[0]) == 0 and len(got[1]) == 0
    # (thin boxes have few cells and a face needs 18 valid voxels: the mid-column box alone has faces under both rules)
    print(nonempty, with_vertices)
    assert nonempty >= 2 and with_vertices >= 6
    nv, nf = C.c_size_t(9), C.c_size_t(9)
    one = (np.array([lo[0], lo[1], 0], dtype=np.int32), np.array([hi[0], hi[1], 0], dtype=np.int32))
    assert t._L.ws_map_mesh(t.handle, 0, one[0].ctypes.data_as(C.c_void_p), one[1].ctypes.data_as(C.c_void_p), 0, C.byref(nv), C.byref(nf)) == 0
    assert (nv.value, nf.value) == (0, 0)  # WS_OK, empty
    # the mesh of a box is not a subset of the whole mesh at its rim: the model decides, and the whole mesh has more
    a, b = boxes["starts and ends mid-column"]
    assert len(avg.mesh(lo=a, hi=b)[1]) < len(whole[1])
    with pytest.raises(W.WsError):
        avg.mesh(lo=(int(lo[0]) - 1, 0, 0), hi=(int(lo[0]), 0, 0))  # outside the window
    with pytest.raises(W.WsError):
        avg.mesh(lo=(0, 0, 0), hi=(0, -1, 0))


def test_sphere_on_the_device_is_closed():
    import warpsense_amd as W
    for edge, centre, radius in SPHERES:
        box = sphere_box(edge, centre, radius)
        size = (edge,) * 3
        pos = tuple(SPHERE_LO[k] + edge // 2 for k in range(3))
        off = (3, edge - 2, edge // 2)  # a rotated ring: storage holds the box in ring order
        data = np.empty(edge ** 3, dtype=np.uint32).reshape(size)
        ax = [(np.arange(SPHERE_LO[k], SPHERE_LO[k] + edge) - pos[k] + off[k] + edge) % edge for k in range(3)]
        data[np.ix_(*ax)] = box
        view = W.DeviceMap(size, off, data.reshape(-1), pos)
        t = W.TSDFCuda(view, TAU, 640, RES)
        got = t.avg_map().mesh()
        want = model_box(box, SPHERE_LO, RES)
        assert same(got, want) and same(got, model(view, RES))
        rep = mesh_report(*got)
        assert rep["closed"] and rep["chi"] == 2 and rep["unreferenced"] == 0, rep


def test_repeatable_aliased_and_partial_downloads():
    W, tm, lm = make_maps((15, 15, 15), seed=21)
    t = tm.tsdf()
    avg = t.avg_map()
    vert, face = avg.mesh()
    assert same(avg.mesh(), (vert, face))  # two calls: identical bytes
    dv, df = avg.mesh(device=True)
    assert dv.is_cuda and df.is_cuda and tuple(dv.shape) == (len(vert), 4) and tuple(df.shape) == (len(face), 3)
    nv = C.c_size_t(0)
    assert dv.data_ptr() == t._L.ws_map_mesh_vertices_dev(t.handle, C.byref(nv)) and nv.value == len(vert)
    assert df.data_ptr() == t._L.ws_map_mesh_faces_dev(t.handle, C.byref(nv)) and nv.value == len(face)
    assert np.array_equal(dv.cpu().numpy().view(np.uint8).reshape(-1), vert.view(np.uint8).reshape(-1))
    assert np.array_equal(df.cpu().numpy().view(np.uint8).reshape(-1), face.view(np.uint8).reshape(-1))
    assert same(tm.surface_mesh(), (vert, face))
    # a surface-cloud call between the mesh call and its download does not disturb it, and the other way round
    avg.mesh()
    rec = avg.surface()
    cv, cf = len(vert) // 3, len(face) // 2
    assert cv > 10 and cf > 10
    pv, pf = np.zeros(cv, dtype=VERT), np.zeros((cf, 3), dtype=np.uint32)
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    assert t._L.ws_map_mesh_download(t.handle, pv.ctypes.data_as(C.c_void_p), pf.ctypes.data_as(C.c_void_p), cv, cf, C.byref(gv), C.byref(gf)) == 0
    assert (gv.value, gf.value) == (len(vert), len(face)) and QM.same(pv, vert[:cv]) and QM.same(pf, face[:cf])
    assert t._L.ws_map_mesh_download(t.handle, None, None, 0, 0, C.byref(gv), C.byref(gf)) == 0 and (gv.value, gf.value) == (len(vert), len(face))
    n = C.c_size_t(0)
    got = np.zeros(len(rec), dtype=G.REC)
    assert t._L.ws_map_surface_download(t.handle, got.ctypes.data_as(C.c_void_p), None, len(rec), C.byref(n)) == 0 and QM.same(got, rec)
    # an empty map: WS_OK, nothing
    lm0 = W.LocalMap(15, 15, 15, TAU, 0)
    v0, f0 = W.TSDFCuda(lm0.device_map(), TAU, 640, RES).avg_map().mesh(any_weight=True)
    assert v0.shape == (0,) and f0.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ after real scans
def test_after_real_scans_at_benchmark_size():
    """the benchmark's 131 072-point scan into the 513^3 map @ 50 mm, two updates, on a ring whose seams lie inside the window"""
    import torch
    import warpsense_amd as W
    tau, res, mw, size = 1000, 50, 640, (512, 512, 512)
    lm = W.LocalMap(*size, tau, 0)
    lm.offset[:] = (lm.size // 2 + np.array([-226, -20, 11])) % lm.size  # (every voxel is the default entry: any rotation is a valid ring)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        pos = [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor]
        t.update_tsdf(torch.from_numpy(pts).cuda(), pos, (0, 0, 32768))
    pert = S.transform_points_mm(S.os1_128_scan(), S.perturbation())
    reg = W.RegistrationCuda(None)
    reg.prepare_registration(torch.from_numpy(pert).cuda())
    T0, it0 = reg.register_cloud(t.device_map(), np.eye(4, dtype=np.float32), 200, 0.1, 0.03, res)
    t0 = time.perf_counter()
    vert, face = t.avg_map().mesh()
    print(f"513^3 mesh() incl. download: {time.perf_counter() - t0:.4f} s, {len(vert)} vertices, {len(face)} faces")
    assert same(t.avg_map().mesh(), (vert, face))
    T1, it1 = reg.register_cloud(t.device_map(), np.eye(4, dtype=np.float32), 200, 0.1, 0.03, res)
    assert it1 == it0 and it0 > 50 and np.array_equal(T0, T1)  # the call left the maps and the pending-scan state alone
    assert int(face.max()) < len(vert)
    assert np.all((face[:, 0] != face[:, 1]) & (face[:, 1] != face[:, 2]) & (face[:, 0] != face[:, 2]))  # no degenerate triangle
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    t.avg_map().to_host(host)
    lo, hi = QM.window(host.size_, host.pos_)
    # whole-window counts against the model's, over x-slabs that overlap by one voxel (cells) and own their faces' owner planes
    n_v = n_f = 0
    step = 32
    for x0 in range(int(lo[0]), int(hi[0]), step):
        x1 = min(x0 + step, int(hi[0]))
        cv, active, inside = cell_masks(QM.ring_box(host.data_, host.size_, host.pos_, host.offset_, (max(x0 - 1, int(lo[0])), lo[1], lo[2]), (x1, hi[1], hi[2])))
        first = 1 if x0 > int(lo[0]) else 0  # the slab's first cell plane belongs to the slab before
        n_v += int(np.count_nonzero(active[first:]))
        n_f += 2 * sum(int(np.count_nonzero(m[first:])) for m in quad_masks(cv, inside))
    assert (len(vert), len(face)) == (n_v, n_f) and n_v > 100_000, (len(vert), len(face), n_v, n_f)
    seam_x = int(lo[0] + (-(lo[0] - host.pos_[0] + host.offset_[0])) % host.size_[0])
    assert lo[0] + 40 < seam_x < hi[0] - 40
    boxes = {"around the sensor": ((-100, -100, -55), (100, 100, 55)),
             "across the x seam": ((seam_x - 30, -165, -55), (seam_x + 29, 165, 55)),
             "at a wall": ((180, -150, -45), (215, 150, 45))}
    for name, (a, b) in boxes.items():
        assert int(np.prod([b[k] - a[k] + 1 for k in range(3)])) <= 64 << 20
        got = t.avg_map().mesh(lo=a, hi=b)
        want = model(host, res, a, b)
        print(name, len(want[0]), len(want[1]))
        assert len(want[1]) > 10_000 and same(got, want), name
    fresh_v, fresh_f = t.new_map().mesh(any_weight=True)
    assert len(fresh_v) == 0 and len(fresh_f) == 0


def test_byte_offsets_beyond_4_gib():
    """the 1025^3 window of configs[2] (4.3 GB per map, device-only voxels): after a shift and one scan, a box at the far end of
    memory order against the model on ws_map_extract_box"""
    import torch
    import warpsense_amd as W
    free, _ = torch.cuda.mem_get_info()
    if free / 2 ** 30 < 24:
        if os.environ.get("WS_ALLOW_BIG_SKIP") == "1":
            pytest.skip("needs ~24 GB on the GPU")
        pytest.fail("needs ~24 GB on the GPU (set WS_ALLOW_BIG_SKIP=1 to skip on this box)")
    tau, res, mw, size = 1000, 50, 640, (1024, 1024, 1024)
    mp = W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(s * res / 1000.0 for s in size))
    lm = W.LocalMap(*size, tau, 0, host_voxels=False)
    shift = (500, -5, 3)  # (as test_gpu_surface.py: the LAST storage plane is world x = 512, inside the sensor's room)
    lm.pos[:] = shift
    lm.offset[:] = (lm.size // 2 + np.asarray(shift)) % lm.size
    tm = W.TSDFMapping(W.Params(mp), lm)
    tm.shift_map((shift[0] + 2, shift[1], shift[2] - 1))
    shift = tuple(int(v) for v in lm.pos)
    pts = S.os1_128_scan(sensor_mm=(4.0, 9.0, 2.0), seed=300) + (np.asarray(shift, dtype=np.int32) * res)[None, :]
    tm.update_tsdf(torch.from_numpy(pts).cuda(), pos_rm=list(shift), up_rm=(0, 0, 32768))
    assert tm.tsdf().stats()["error_flags"] == 0
    avg = tm.tsdf().avg_map()
    lo, hi = QM.window(lm.size, lm.pos)
    n_side = int(lm.size[0])
    x_far = int(lo[0] + (n_side - 1 - (lo[0] - lm.pos[0] + lm.offset[0])) % n_side)
    assert x_far == 512 and lo[0] + 60 < x_far and x_far + 4 <= hi[0]
    for a, b in [((x_far - 59, lo[1], lo[2]), (x_far, hi[1], hi[2])),                    # the far end of memory order
                 ((x_far - 3, lo[1] + 1, lo[2] + 2), (x_far + 4, hi[1] - 3, hi[2] - 1))]:  # across the x seam
        ext = tuple(int(b[k] - a[k] + 1) for k in range(3))
        assert int(np.prod(ext)) <= 64 << 20
        box = avg.extract_box(a, b).reshape(ext)
        want = model_box(box, np.asarray(a, dtype=np.int64), res)
        got = avg.mesh(lo=a, hi=b)
        assert len(want[1]) > 1000 and same(got, want), (a, b)


# ------------------------------------------------------------------------------------------------ C++ twin
def test_cpp_twin_matches_the_python_route(tmp_path):
    import warpsense_amd as W
    exe = build_dropin("mesh_dropin", tmp_path)
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
    vert, face = t.avg_map().mesh()
    assert len(vert) > 1000 and len(face) > 1000
    assert lines["mesh"] == [str(len(vert)), str(len(face)), f"{QM.fnv1a(vert.tobytes()):016x}", f"{QM.fnv1a(face.tobytes()):016x}"]
    bv, bf = t.avg_map().mesh(lo=(5, -30, -25), hi=(32, 30, 25), any_weight=True)  # the room's +x wall
    assert 0 < len(bf) and len(bv) < len(vert)
    assert lines["box"] == [str(len(bv)), str(len(bf)), f"{QM.fnv1a(bv.tobytes()):016x}", f"{QM.fnv1a(bf.tobytes()):016x}"]
