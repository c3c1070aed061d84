"""ws_map_surface — the surface cloud of a device map (publish_local_map, include/warpsense/visualization/map.h:14-121, on the
device) against a numpy model applied to ws_map_download / ws_map_extract_box of the same map.  Every comparison is bit for bit:
np.array_equal on the raw bytes of the records and of the marker floats.

The model is a line-for-line port of map.h:19-75 (the reference lines are cited in it); it is not part of the oracle."""
import os
import subprocess
import time

import numpy as np
import pytest

from dropin_build import build_dropin
from query_model import download, fnv1a, same, window, wrapper
from surface_model import F, REC, RES, SIZES, TAU, check_inputs, draw_entries, model, model_box, skeleton_model
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


def make_maps(size, seed):
    """as _maps of test_gpu_map_shift.py, with draw_entries; new_map gets entries of its own (another seed)"""
    import warpsense_amd as W
    lm = W.LocalMap(*size, TAU, 0)
    lm.data[:] = draw_entries(lm.data.size, seed)
    check_inputs(lm.data)
    params = W.Params(W.MapParams(resolution=RES, max_distance=TAU / 1000.0, max_weight=10, size=tuple(s * RES / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    other = W.LocalMap(*size, TAU, 0)
    other.data[:] = draw_entries(other.data.size, seed + 1000)
    check_inputs(other.data)
    tm.tsdf().new_map().to_device(other.device_map())
    return W, tm, lm


@pytest.mark.parametrize("size", SIZES)
def test_arbitrary_entries_match_the_model(size):
    """(through TSDFCuda directly: LocalMap forces odd sizes, the C ABI does not)"""
    import warpsense_amd as W
    n = int(np.prod(size))
    pos, off = (0, 0, 0), tuple(s // 2 for s in size)
    views = [W.DeviceMap(size, off, draw_entries(n, seed=sum(size) + 1000 * which), pos) for which in (0, 1)]
    for v in views:
        check_inputs(v.data_)
    t = W.TSDFCuda(views[0], TAU, 640, RES)
    t.new_map().to_device(views[1])
    for which in (0, 1):
        host = W.DeviceMap(size, off, np.empty(n, dtype=np.uint32), pos)
        wrapper(t, which).to_host(host)
        assert np.array_equal(host.data_, views[which].data_)
        rec, mk = wrapper(t, which).surface(marker=True)
        want_rec, want_mk = model(host, TAU, RES)
        assert len(want_rec) > 0 and same(rec, want_rec) and same(mk, want_mk), (size, which)
        assert same(wrapper(t, which).surface(), want_rec)


def test_even_sizes_visit_each_ring_cell_once():
    """LocalMap forces odd sizes, the C ABI does not: an even-sized device map through TSDFCuda directly, rotated offsets"""
    import warpsense_amd as W
    size, pos, off = (16, 18, 20), (3, -2, 5), (5, 0, 19)
    data = draw_entries(16 * 18 * 20, seed=77)
    check_inputs(data)
    view = W.DeviceMap(size, off, data, pos)
    t = W.TSDFCuda(view, TAU, 640, RES)
    rec, mk = t.avg_map().surface(marker=True)
    want_rec, want_mk = model(view, TAU, RES)
    assert same(rec, want_rec) and same(mk, want_mk)
    lo, hi = window(size, pos)
    assert same(t.avg_map().surface(lo=lo, hi=hi), want_rec)
    # pos - size/2 .. pos + size/2 passes the window rule but holds one ring cell twice along every axis: refused
    with pytest.raises(W.WsError):
        t.avg_map().surface(lo=lo, hi=hi + 1)


def test_rotated_rings_after_the_shift_sequence():
    """after the shift sequence of test_shift_sequence_matches_host_mirror (without its return to the origin) all three offsets are
    non-zero and the z and y runs wrap; both maps"""
    W, tm, lm = make_maps((21, 17, 13), seed=5)
    for new_pos in [(3, 0, 0), (3, -4, 2), (10, -4, 2), (10, 5, -3), (-2, 5, -3)]:
        tm.shift_map(new_pos)
        assert tm.tsdf().avg_map().surface().dtype == REC  # (a call between two shifts: the buffers follow the window)
    for which in (0, 1):
        host = download(W, tm, lm, which)
        assert all(int(o) != 0 for o in host.offset_) and list(host.pos_) == [-2, 5, -3]
        rec, mk = wrapper(tm.tsdf(), which).surface(marker=True)
        want_rec, want_mk = model(host, TAU, RES)
        assert len(want_rec) > 100 and same(rec, want_rec) and same(mk, want_mk), which


def test_boxes_and_bands():
    W, tm, lm = make_maps((21, 17, 13), seed=9)
    for new_pos in [(3, -4, 2), (10, 5, -3)]:
        tm.shift_map(new_pos)
    host = download(W, tm, lm)
    avg = tm.tsdf().avg_map()
    lo, hi = window(host.size_, host.pos_)
    whole = avg.surface()
    assert same(whole, avg.surface(lo=lo, hi=hi)) and same(whole, model(host, TAU, RES)[0])
    # where the ring wraps in world coordinates: storage index 0 of axis k is world pos - offset (mod size)
    seam = [int(lo[k] + (-(lo[k] - host.pos_[k] + host.offset_[k])) % host.size_[k]) for k in range(3)]
    assert all(lo[k] < seam[k] <= hi[k] for k in range(3)), seam
    boxes = {
        "one voxel": ((5, 3, -2), (5, 3, -2)),
        "starts and ends mid-column": ((lo[0] + 2, lo[1] + 3, lo[2] + 1), (hi[0] - 4, hi[1] - 1, hi[2] - 2)),
        "crosses the wrap on every axis": (tuple(s - 2 for s in seam), tuple(s + 1 for s in seam)),
        "one column": ((lo[0], hi[1], lo[2]), (lo[0], hi[1], hi[2])),
    }
    for name, (a, b) in boxes.items():
        for band in (1, TAU // 2, TAU, 0):
            rec, mk = avg.surface(lo=a, hi=b, band=band, marker=True)
            want_rec, want_mk = model(host, TAU, RES, a, b, band)
            assert same(rec, want_rec) and same(mk, want_mk), (name, band)
    assert same(avg.surface(band=0), avg.surface(band=TAU)) and len(avg.surface(band=1)) < len(avg.surface(band=TAU // 2)) < len(whole)
    with pytest.raises(W.WsError):
        avg.surface(lo=(int(lo[0]) - 1, 0, 0), hi=(int(lo[0]), 0, 0))  # outside the window
    with pytest.raises(W.WsError):
        avg.surface(lo=(0, 0, 0), hi=(0, -1, 0))


def test_device_tensors_alias_the_result():
    W, tm, lm = make_maps((15, 15, 15), seed=21)
    avg = tm.tsdf().avg_map()
    rec, mk = avg.surface(marker=True)
    drec, dmk = avg.surface(marker=True, device=True)
    assert drec.is_cuda and dmk.is_cuda and tuple(drec.shape) == (len(rec), 4) and tuple(dmk.shape) == (len(rec), 7)
    assert np.array_equal(drec.cpu().numpy().view(np.uint8).reshape(-1), rec.view(np.uint8).reshape(-1))
    assert np.array_equal(dmk.cpu().numpy().view(np.uint8), mk.view(np.uint8))
    assert same(tm.surface_cloud(), rec)


def test_empty_map_and_download_capacity():
    import ctypes as C
    import warpsense_amd as W
    lm = W.LocalMap(15, 15, 15, TAU, 0)  # every voxel (tau, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, 640, RES)
    rec, mk = t.avg_map().surface(marker=True)
    assert rec.shape == (0,) and mk.shape == (0, 7)
    n = C.c_size_t(99)
    assert t._L.ws_map_surface(t.handle, 0, None, None, 0, 0, C.byref(n)) == 0 and n.value == 0  # WS_OK (the reference only logs)
    W2, tm, lm2 = make_maps((15, 15, 15), seed=31)
    t2 = tm.tsdf()
    full_rec, full_mk = t2.avg_map().surface(marker=True)
    cap = len(full_rec) // 3
    assert cap > 10
    part_rec, part_mk = np.zeros(cap, dtype=REC), np.zeros((cap, 7), dtype=F)
    assert t2._L.ws_map_surface_download(t2.handle, part_rec.ctypes.data_as(C.c_void_p), part_mk.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
    assert n.value == len(full_rec) and same(part_rec, full_rec[:cap]) and same(part_mk, full_mk[:cap])
    assert t2._L.ws_map_surface_download(t2.handle, None, None, 0, C.byref(n)) == 0 and n.value == len(full_rec)  # either pointer may be NULL


# ------------------------------------------------------------------------------------------------ after real scans
def test_after_real_scans_at_benchmark_size():
    """the benchmark's 131 072-point scan into the 513^3 map @ 50 mm, two updates (as test_full_size_scan_matches_oracle)"""
    import torch
    import warpsense_amd as W
    tau, res, mw, size = 1000, 50, 640, (512, 512, 512)
    lm = W.LocalMap(*size, tau, 0)
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
    rec, mk = t.avg_map().surface(marker=True)
    print(f"513^3 surface(marker=True) incl. download: {time.perf_counter() - t0:.4f} s, {len(rec)} points")
    rec2, mk2 = t.avg_map().surface(marker=True)
    assert same(rec, rec2) and same(mk, mk2)  # deterministic: identical bytes
    T1, it1 = reg.register_cloud(t.device_map(), np.eye(4, dtype=np.float32), 200, 0.1, 0.03, res)
    assert it1 == it0 and it0 > 50 and np.array_equal(T0, T1)  # the call left the maps and the pending-scan state alone
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    t.avg_map().to_host(host)
    v, w = W.unpack_entry(host.data_)
    count = int(np.count_nonzero((w > 0) & (np.abs(v.astype(np.int32)) < tau)))
    del v, w
    assert len(rec) == count > 1_000_000
    want_rec, want_mk = model(host, tau, res)
    assert same(rec, want_rec) and same(mk, want_mk)
    fresh = np.empty_like(lm.data)
    t.new_map().to_host(W.DeviceMap(lm.size.copy(), lm.offset.copy(), fresh, lm.pos.copy()))
    assert np.all(fresh == W.pack_entry(tau, 0)) and len(t.new_map().surface()) == 0


def test_byte_offsets_beyond_4_gib():
    """the 1025^3 window of configs[2] (4.3 GB per map, set up as test_gpu_configs.py does: device-only voxels): after a shift and
    one scan, three boxes of at most 64 M voxels against the model on ws_map_extract_box -- one at the far end of memory order --
    and the whole-window count against a count made slab by slab."""
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
    # A window that has moved: world x lives in storage plane (x + 512) % 1025 wherever the window is, so the LAST storage plane
    # is world x = 512; the window is placed around it (pos / offset as HDF5LocalMap::shift leaves them, hdf5_local_map.cpp:53-118)
    # so that the sensor's room covers the end of the allocation.
    shift = (500, -5, 3)
    lm.pos[:] = shift
    lm.offset[:] = (lm.size // 2 + np.asarray(shift)) % lm.size
    tm = W.TSDFMapping(W.Params(mp), lm)
    tm.shift_map((shift[0] + 2, shift[1], shift[2] - 1))  # and one real shift on top (the slabs are still default entries)
    shift = tuple(int(v) for v in lm.pos)
    # (the synthetic room is centred on the origin: the scan is taken there and moved to the window by whole voxels)
    pts = S.os1_128_scan(sensor_mm=(4.0, 9.0, 2.0), seed=300) + (np.asarray(shift, dtype=np.int32) * res)[None, :]
    tm.update_tsdf(torch.from_numpy(pts).cuda(), pos_rm=list(shift), up_rm=(0, 0, 32768))
    assert tm.tsdf().stats()["error_flags"] == 0
    avg = tm.tsdf().avg_map()
    lo, hi = window(lm.size, lm.pos)
    n_side = int(lm.size[0])
    # world x of the LAST storage plane (storage x = size - 1): voxel indices up to 1025^3 - 1, byte offsets up to 4.3e9
    x_far = int(lo[0] + (n_side - 1 - (lo[0] - lm.pos[0] + lm.offset[0])) % n_side)
    assert x_far == 512 and lo[0] + 60 < x_far and x_far + 4 <= hi[0]
    boxes = [((x_far - 59, lo[1], lo[2]), (x_far, hi[1], hi[2])),                               # the far end of memory order
             ((shift[0] - 200, shift[1] - 150, shift[2] - 40), (shift[0] + 199, shift[1] + 149, shift[2] + 40)),  # the room around the sensor
             ((x_far - 3, lo[1] + 1, lo[2] + 2), (x_far + 4, hi[1] - 3, hi[2] - 1))]            # across the x seam
    t0 = time.perf_counter()
    total_in_boxes = 0
    for a, b in boxes:
        ext = tuple(int(b[k] - a[k] + 1) for k in range(3))
        assert int(np.prod(ext)) <= 64 << 20
        box = avg.extract_box(a, b).reshape(ext)
        want_rec, want_mk = model_box(box, np.asarray(a, dtype=np.int64), tau, res)
        rec, mk = avg.surface(lo=a, hi=b, marker=True)
        assert same(rec, want_rec) and same(mk, want_mk), (a, b)
        assert len(rec) > 10_000, (a, b)  # the scan's surface is in every one of them
        total_in_boxes += len(rec)
    assert total_in_boxes > 100_000
    t1 = time.perf_counter()
    whole = len(avg.surface())
    counted = 0
    for x0 in range(int(lo[0]), int(hi[0]) + 1, 60):
        x1 = min(x0 + 59, int(hi[0]))
        slab = avg.extract_box((x0, lo[1], lo[2]), (x1, hi[1], hi[2]))
        v = (slab & 0xFFFF).astype(np.uint16).view(np.int16)
        w = (slab >> 16).astype(np.uint16).view(np.int16)
        counted += int(np.count_nonzero((w > 0) & (np.abs(v.astype(np.int32)) < tau)))
    print(f"1025^3: three boxes {t1 - t0:.2f} s, whole-window count against slabs {time.perf_counter() - t1:.2f} s, {whole} points")
    assert whole == counted > 1_000_000


def test_cpp_twin_matches_the_python_route(tmp_path):
    import warpsense_amd as W
    exe = build_dropin("surface_dropin", tmp_path)
    tau, res, mw, edge = 1000, 50, 640, 65
    pts = S.os1_128_scan(rings=32, azimuths=256, half_extents_mm=(1400.0, 1300.0, 900.0), seed=2)
    pts.tofile(tmp_path / "scan.bin")
    pos = (-37, 12, 5)
    out = subprocess.run([str(exe), str(tmp_path / "scan.bin"), str(len(pts)), str(edge), str(res), str(tau), str(mw), *(str(p) for p in pos)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    lm = W.LocalMap(edge, edge, edge, tau, 0)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    t.update_tsdf(pts, (0, 0, 0), (0, 0, 32768))
    rec, mk = t.avg_map().surface(marker=True)
    assert len(rec) > 1000
    assert lines["cloud"] == [str(len(rec)), f"{fnv1a(rec.tobytes()):016x}", f"{fnv1a(mk.tobytes()):016x}"]
    box = t.avg_map().surface(lo=(-(edge // 4), -3, -(edge // 2)), hi=(edge // 4, edge // 3, 5), band=tau // 2)
    assert 0 < len(box) < len(rec)
    assert lines["box"] == [str(len(box)), f"{fnv1a(box.tobytes()):016x}", "0"]
    sk = np.array([float(v) for v in lines["skeleton"][1:]]).reshape(-1, 3)
    assert lines["skeleton"][0] == "24" and np.array_equal(sk, skeleton_model((edge,) * 3, pos, res))
