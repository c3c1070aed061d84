"""ws_map_sample — the point sample of a device map (the rules are stated in include/warpsense_hip.h) against the numpy model of
tests/test_sample_host.py applied to the same entries.  Everything is integer: every comparison is on the raw bytes of the records,
the gradient and the selection, and on the exact counts.  The inputs are those of test_sample_host, which checks without a GPU that
every class and the non-zero gradients occur at least 16 times in each case."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mesh_model as M
import query_model as QM
import raycast_model as R
import sample_model as H
from scan_clouds import CLUSTER_AT, app_stream, room_scan

pytestmark = pytest.mark.gpu
TAU, RES = H.TAU, H.RES
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
ALL = (H.UNKNOWN, H.FREE, H.SURFACE, H.INSIDE)


def names(classes):
    return [H.CLASS_NAMES[c] for c in classes]


def upload(size, seed, res):
    """a TSDFCuda at resolution res whose two maps hold draw_storage(seed), draw_storage(seed + 100); the Rings of the model"""
    cases = [H.window_case(size, seed, res, which) for which in (0, 1)]
    t, _ = R.upload(size, cases[0][1], cases[0][2], [c[0] for c in cases], tau=TAU, res=res)
    return t, cases


# ------------------------------------------------------------------------------------------------ 1: arbitrary entries, four resolutions
@pytest.mark.parametrize("res", H.WINDOW_RESOLUTIONS)
@pytest.mark.parametrize("size,seed", R.RANDOM_MAPS)
def test_random_maps_match_the_model(size, seed, res):
    import torch
    t, cases = upload(size, seed, res)
    for which in (0, 1):
        _, _, _, ring, pts, band = cases[which]
        p32 = pts.astype(np.int32)
        p_dev = torch.from_numpy(p32).cuda()
        w = QM.wrapper(t, which)
        for any_weight in (False, True):
            want = H.model(ring, res, pts, band, any_weight, select=(H.FREE, H.INSIDE))
            kw = dict(band_mm=band, any_weight=any_weight, gradient=True, select=("free", "inside"))
            got = w.sample(p32, **kw)
            print(size, res, which, any_weight, got[1].tolist())
            assert H.same(got, want), (which, any_weight, "host")
            assert H.same(w.sample(p_dev, **kw), want), (which, any_weight, "dev")       # the _dev form, and a second call: the same bytes
            plain = w.sample(p32, band_mm=band, any_weight=any_weight)
            assert plain[2] is None and plain[3] is None and H.same(plain, want)
    t.close()


# ------------------------------------------------------------------------------------------------ 2: the edges of a wave and of a workgroup
def test_sizes_and_every_select_mask():
    size, seed = R.RANDOM_MAPS[1]
    t, cases = upload(size, seed, RES)
    _, _, _, ring, pts, band = cases[0]
    w = t.avg_map()
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 65, 255, 257, 2048):
        sub = pts[rng.permutation(len(pts))[:n]]
        want = H.model(ring, RES, sub, band, True, select=(H.UNKNOWN, H.SURFACE))
        assert H.same(w.sample(sub.astype(np.int32), band_mm=band, any_weight=True, gradient=True, select=("unknown", "surface")), want), n
    sub = pts[rng.permutation(len(pts))[:257]]
    cls = H.model(ring, RES, sub, band, True)[0]["cls"]
    assert all(np.count_nonzero(cls == c) > 0 for c in ALL)
    for k in range(1, 5):
        for classes in itertools.combinations(ALL, k):  # the 15 non-empty masks: order and content
            want = H.model(ring, RES, sub, band, True, select=classes)
            got = w.sample(sub.astype(np.int32), band_mm=band, any_weight=True, select=names(classes))
            assert H.same(got, want) and len(got[3]) == int(sum(want[1][c] for c in classes)), classes
    t.close()


def test_selection_over_more_than_1024_workgroups():
    """262 144 + 77 points are 1025 workgroup totals: the smallest count at which the scan of the selection gives a thread more than
    one total (scan_block_totals, ws_device.h: seg > 1), with a ragged last workgroup."""
    size, seed = R.RANDOM_MAPS[0]
    t, cases = upload(size, seed, RES)
    _, _, _, ring, _, band = cases[0]
    n = 262144 + 77
    reps = []
    while sum(len(p) for p in reps) < n:
        reps.append(H.window_points(ring.lo, ring.hi, RES, seed=4000 + len(reps)))
    pts = np.concatenate(reps)[:n]
    assert len(pts) == n and (n + 255) // 256 == 1025
    want = H.model(ring, RES, pts, band, True, select=(H.UNKNOWN, H.SURFACE))
    cls = want[0]["cls"]
    for part in (cls[:256], cls[262144:]):  # every class in the first and in the last (77-point) workgroup
        assert len(part) in (256, 77) and all(np.count_nonzero(part == c) > 0 for c in ALL), np.bincount(part, minlength=4)
    got = t.avg_map().sample(pts.astype(np.int32), band_mm=band, any_weight=True, select=("unknown", "surface"))
    print(got[1].tolist(), len(got[3]))
    assert len(want[3]) == int(want[1][H.UNKNOWN] + want[1][H.SURFACE]) > 1024
    assert H.same(got, want)
    t.close()


# ------------------------------------------------------------------------------------------------ 3: rotated rings, even sizes
def test_rotated_rings_after_the_shift_sequence():
    W, tm, lm = M.make_maps((21, 17, 13), seed=5)
    for new_pos in [(3, 0, 0), (3, -4, 2), (10, -4, 2), (10, 5, -3), (-2, 5, -3)]:
        tm.shift_map(new_pos)
    for which in (0, 1):
        host = QM.download(W, tm, lm, which)
        assert all(int(o) != 0 for o in host.offset_) and list(host.pos_) == [-2, 5, -3]
        ring = R.Ring(host.data_, host.size_, host.pos_, host.offset_)
        pts = H.window_points(ring.lo, ring.hi, RES, seed=17 + which, n=4096)
        for any_weight in (False, True):
            # (M.draw_entries: values in [-2 tau, 2 tau], so band tau has all four classes)
            want = H.model(ring, RES, pts, TAU, any_weight, select=(H.SURFACE, H.INSIDE))
            n_grad = int(np.count_nonzero(np.any(want[2] != 0, axis=1)))
            print(which, any_weight, want[1].tolist(), n_grad)
            assert want[1].min() >= 16 and n_grad >= 16
            got = QM.wrapper(tm.tsdf(), which).sample(pts.astype(np.int32), any_weight=any_weight, gradient=True, select=("surface", "inside"))  # band: the map's tau
            assert H.same(got, want), (which, any_weight)


@pytest.mark.parametrize("size", [(16, 18, 20), (15, 17, 24)])
def test_even_window_sizes(size):
    t, cases = upload(size, 31, RES)
    for which in (0, 1):
        _, _, _, ring, pts, band = cases[which]
        want = H.model(ring, RES, pts, band, True, select=(H.FREE,))
        assert want[1].min() >= 16 and np.count_nonzero(np.any(want[2] != 0, axis=1)) >= 16
        assert H.same(QM.wrapper(t, which).sample(pts.astype(np.int32), band_mm=band, any_weight=True, gradient=True, select=("free",)), want), which
    t.close()


# ------------------------------------------------------------------------------------------------ 4: buffers, prefixes, refusals
def test_prefix_downloads_refusals_and_no_points():
    import warpsense_amd as W
    size, seed = R.RANDOM_MAPS[0]
    t, cases = upload(size, seed, RES)
    _, _, _, ring, pts, band = cases[0]
    L, avg = t._L, t.avg_map()
    p32 = np.ascontiguousarray(pts[:700].astype(np.int32))
    rec, counts, grad, sel = avg.sample(p32, band_mm=band, any_weight=True, gradient=True, select=("unknown", "inside"))
    n, ns = C.c_size_t(0), C.c_size_t(0)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    assert L.ws_map_sample_records_dev(t.handle, C.byref(n)) and n.value == 700
    assert L.ws_map_sample_gradient_dev(t.handle, C.byref(n)) and n.value == 700
    assert L.ws_map_sample_selected_dev(t.handle, C.byref(n)) and n.value == len(sel) > 16
    # the other queries between the call and its download do not disturb it
    avg.surface(), avg.mesh(), avg.raycast((0, 0, 0), p32[:50], 3000)
    pr, pg, ps = np.zeros(233, dtype=H.SAMPLE), np.zeros((233, 3), dtype=np.int32), np.zeros((5, 3), dtype=np.int32)
    assert L.ws_map_sample_download(t.handle, vp(pr), vp(pg), vp(ps), 233, 5, C.byref(n), C.byref(ns)) == 0
    assert (n.value, ns.value) == (700, len(sel)) and QM.same(pr, rec[:233]) and QM.same(pg, grad[:233]) and QM.same(ps, sel[:5])
    assert L.ws_map_sample_download(t.handle, None, None, None, 0, 0, C.byref(n), C.byref(ns)) == 0 and (n.value, ns.value) == (700, len(sel))

    def last_is_intact():
        a, b, c = np.zeros(700, dtype=H.SAMPLE), np.zeros((700, 3), dtype=np.int32), np.zeros((len(sel), 3), dtype=np.int32)
        assert L.ws_map_sample_download(t.handle, vp(a), vp(b), vp(c), 700, len(sel), C.byref(n), C.byref(ns)) == 0
        return (n.value, ns.value) == (700, len(sel)) and QM.same(a, rec) and QM.same(b, grad) and QM.same(c, sel)

    # every refusal returns its code, launches nothing and leaves the last result readable
    cnt = np.full(4, 77, dtype=np.uint64)
    call = lambda which=0, count=10, flags=0, p=p32: L.ws_map_sample(t.handle, which, vp(p), count, band, flags, vp(cnt))
    assert call(flags=64) == WS_ERR_INVALID and call(flags=1 << 31) == WS_ERR_INVALID and call(which=2) == WS_ERR_INVALID and call(which=-1) == WS_ERR_INVALID
    assert call(p=None) == WS_ERR_INVALID and L.ws_map_sample(None, 0, vp(p32), 10, band, 0, None) == WS_ERR_INVALID
    assert call(count=2 ** 27 + 1) == WS_ERR_RANGE
    assert cnt.tolist() == [77] * 4 and last_is_intact()
    coarse = W.LocalMap(15, 15, 15, TAU, 0)
    t2 = W.TSDFCuda(coarse.device_map(), 3000, 640, 1025)
    with pytest.raises(W.WsError):
        t2.avg_map().sample(p32[:10])
    assert L.ws_map_sample_records_dev(t2.handle, C.byref(n)) is None and n.value == 0  # nothing was ever allocated there
    t2.close()
    assert last_is_intact()
    # without the flags there is no gradient and no selection to fetch
    avg.sample(p32[:100], band_mm=band)
    assert L.ws_map_sample_gradient_dev(t.handle, C.byref(n)) is None and n.value == 0
    assert L.ws_map_sample_selected_dev(t.handle, C.byref(n)) is None and n.value == 0
    assert L.ws_map_sample_download(t.handle, vp(pr), vp(pg), None, 50, 0, C.byref(n), None) == WS_ERR_INVALID
    assert L.ws_map_sample_download(t.handle, vp(pr), None, vp(ps), 50, 5, C.byref(n), None) == WS_ERR_INVALID
    # a selection that selects nothing
    r0 = avg.sample(np.array([[2 ** 30, 0, 0]], dtype=np.int32), select=("free",))
    assert r0[1].tolist() == [1, 0, 0, 0] and r0[3].shape == (0, 3) and not r0[0].tobytes().strip(b"\0")
    assert L.ws_map_sample_selected_dev(t.handle, C.byref(n)) is None and n.value == 0
    # n == 0: WS_OK, counts zero, nothing written
    cnt[:] = 77
    assert L.ws_map_sample(t.handle, 0, None, 0, band, 2 | 8, vp(cnt)) == 0 and cnt.tolist() == [0] * 4
    assert L.ws_map_sample_records_dev(t.handle, C.byref(n)) is None and n.value == 0
    e = avg.sample(np.zeros((0, 3), dtype=np.int32), gradient=True, select=("free",))
    assert e[0].shape == (0,) and e[2].shape == (0, 3) and e[3].shape == (0, 3)
    # the timing entry answers, switched on and off
    assert L.ws_debug_sample_timing(t.handle, 1, None) == 0
    avg.sample(p32, band_mm=band, select=("free",))
    ms = (C.c_float * 3)()
    assert L.ws_debug_sample_timing(t.handle, 0, ms) == 0 and ms[1] > 0 and ms[2] > 0
    t.close()


def test_after_real_scans_a_cluster_in_mid_room_is_free():
    """A 65^3 map @ 50 mm, tau 1000, after two 32 x 256 scans of a (2 800, 2 600, 1 800) mm room.  Computed beforehand without a GPU
    with the oracle's update (tests/oracle_lib.py) and the model: the first scan sampled where it lies is 7 678 SURFACE, 514 UNKNOWN and
    no FREE point at band tau; 200 points within 100 mm of (600, 0, 0) are FREE at band tau / 2, all of them (smallest d_mm 710)."""
    import torch
    import warpsense_amd as W
    tau, res, mw, edge = 1000, 50, 640, 65
    lm = W.LocalMap(edge, edge, edge, tau, 0)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    scans = []
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (120.0, -80.0, 30.0)]):
        scans.append(room_scan(k, sensor))
        t.update_tsdf(scans[k], [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor], (0, 0, 32768))
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    t.avg_map().to_host(host)
    ring = R.Ring(host.data_, host.size_, host.pos_, host.offset_)
    rec, counts, _, _ = t.avg_map().sample(scans[0])
    print("scan at its own pose", counts.tolist())
    assert H.same((rec, counts, None, None), H.model(ring, res, scans[0], tau))
    assert counts[H.SURFACE] > counts[H.FREE] and counts[H.SURFACE] > len(scans[0]) // 2
    cluster = (np.asarray(CLUSTER_AT) + np.random.default_rng(5).integers(-100, 101, (200, 3))).astype(np.int32)
    mixed = np.concatenate([scans[0][:3000], cluster, scans[0][3000:]]).astype(np.int32)
    want = H.model(ring, res, mixed, tau // 2, select=(H.FREE,))
    got = t.avg_map().sample(mixed, band_mm=tau // 2, select=("free",))
    assert H.same(got, want) and np.array_equal(got[3], cluster)  # the whole cluster, in order, and no wall point
    # the selection on the device feeds the update and the registration like the same points from the host
    fresh = lambda: W.TSDFCuda(W.DeviceMap(host.size_.copy(), host.offset_.copy(), host.data_.copy(), host.pos_.copy()), tau, mw, res)
    ta, tb = fresh(), fresh()
    keep_dev = ta.avg_map().sample(torch.from_numpy(mixed).cuda(), band_mm=tau // 2, select=("unknown", "surface", "inside"), device=True)[3]
    keep = np.delete(mixed, np.arange(3000, 3200), axis=0)
    assert isinstance(keep_dev, W.DevicePoints) and len(keep_dev) == len(keep) and np.array_equal(keep_dev.to_host(), keep)
    maps, poses = [], []
    for tx, src in ((ta, keep_dev), (tb, keep)):
        tx.update_tsdf(src, (1, 0, 0), (0, 0, 32768))
        out = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
        tx.avg_map().to_host(out)
        maps.append(out.data_.copy())
        reg = W.RegistrationCuda(None)
        reg.prepare_registration(src)  # (the selection stays valid until the next sample on ta)
        poses.append(reg.register_cloud(tx.device_map(), np.eye(4, dtype=np.float32), 50, 0.1, 0.03, res))
    assert np.array_equal(maps[0], maps[1]) and not np.array_equal(maps[0], host.data_)
    assert np.array_equal(poses[0][0], poses[1][0]) and poses[0][1] == poses[1][1] > 0
    t.close(), ta.close(), tb.close()


def test_app_rejects_dynamic_points_only_when_asked():
    import warpsense_amd as W
    tau, res, mw, size = 1000, 50, 640, (128, 128, 64)
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(s * res / 1000.0 for s in size), shift=0.6),
                      W.RegistrationParams(200, 0.1, 0.03))
    clouds = app_stream(4)
    runs = {}
    for name, kw in (("plain", {}), ("off", {"reject_dynamic": False}), ("on", {"reject_dynamic": True})):
        app = W.App(params, None, **kw)
        for c in clouds:
            app.cloud_callback(c)
        runs[name] = app
    # off is the default: the same poses bit for bit, and no new key in the timings
    assert all(np.array_equal(a, b) for a, b in zip(runs["plain"].poses, runs["off"].poses))
    assert all("rejected" not in t for t in runs["off"].timings) and [t["points"] for t in runs["plain"].timings] == [t["points"] for t in runs["off"].timings]
    on = runs["on"]
    rejected = [t["rejected"] for t in on.timings]
    print("rejected per scan", rejected, "updates", on.n_updates)
    at_updates = [t["rejected"] for t in on.timings if "tsdf" in t]  # the scans that were integrated
    # an empty map is UNKNOWN everywhere: nothing is dropped from the first update; from the second on the thing in free space is
    assert on.n_updates == len(at_updates) >= 2 and at_updates[0] == 0 and all(r > 0 for r in at_updates[1:]) and rejected[1] > 0
    assert on.timings[0]["points"] == runs["plain"].timings[0]["points"] and on.timings[1]["points"] + rejected[1] == runs["plain"].timings[1]["points"]
