"""ws_scan_preprocess_sweep on the GPU: every result is compared with the host model preprocess_sweep_host (tests/test_sweep_host.py pins
that to the oracle) bit for bit including the order, for host and for device input."""
import numpy as np
import pytest

from scan_clouds import POSES, make_cloud
from scan_clouds import rigid
from scan_clouds import both_routes
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pre():
    import warpsense_amd as W
    p = W.ScanPreprocessor(4096)
    yield p
    p.close()


@pytest.mark.parametrize("n", [1, 257, 3000])
@pytest.mark.parametrize("stride", [3, 5])
def test_one_bin_is_the_plain_call(pre, n, stride):
    import warpsense_amd as W
    cloud = make_cloud(n, seed=n + stride, stride=stride) if n > 1 else np.array([[3.0, -2.0, 1.0] + [0.0] * (stride - 3)], dtype=np.float32)
    for pose in POSES:
        want = pre.preprocess(cloud, pose, 50).to_host()
        got = both_routes(pre, cloud, np.asarray(pose, dtype=np.float32)[None], 50)
        assert np.array_equal(got, want)
        assert np.array_equal(got, W.preprocess_sweep_host(cloud, np.asarray(pose, dtype=np.float32)[None], 50))
        if stride == 5:
            assert np.array_equal(both_routes(pre, cloud, np.asarray(pose, dtype=np.float32)[None], 50, time_field=3, t_begin=0.0, t_end=255.0), want)


@pytest.mark.parametrize("k", [2, 7, 64, 1024])
@pytest.mark.parametrize("ring_major", [True, False])
@pytest.mark.parametrize("columns,rows", [(64, 5), (1024, 4), (3, 1)])
def test_bins_by_index(pre, k, ring_major, columns, rows):
    """n = 320 crosses the 256-point workgroup edge with both orders; 1024 x 4 gives a wave 64 rows (ring-major) or one (column-major)"""
    import warpsense_amd as W
    n = columns * rows
    cloud = make_cloud(n, seed=1000 * k + columns) if n > 20 else np.array([[3.0, -2.0, 1.0], [3.01, -2.0, 1.0], [-4.0, 2.5, 0.5]], dtype=np.float32)
    poses = W.sweep_poses(POSES[1], rigid(300.0 * np.cos(0.4), 300.0 * np.sin(0.4), 0.0, 8.0), k)
    want = W.preprocess_sweep_host(cloud, poses, 50, columns=columns, ring_major=ring_major)
    got = both_routes(pre, cloud, poses, 50, columns=columns, ring_major=ring_major)
    assert np.array_equal(got, want)
    if n > 20:  # the bins matter: one pose for all gives other points
        assert not np.array_equal(got, pre.preprocess(cloud, poses[-1], 50).to_host())


def test_bins_by_time(pre):
    import warpsense_amd as W
    n, k = 300, 16
    cloud = make_cloud(n, seed=77, stride=5)
    rng = np.random.default_rng(5)
    t = rng.uniform(-0.1, 1.1, size=n).astype(np.float32)
    t[:12] = [0.0, 1.0, -0.5, 2.5, np.nan, 1.0 / 16, 0.25, 15.0 / 16, np.nextafter(np.float32(0.25), np.float32(0)), np.inf, -np.inf, 0.5]
    t[100:100 + k] = np.arange(k, dtype=np.float32) / np.float32(k)  # every bin edge
    cloud[:, 4] = t
    cloud[:20, :3] = np.abs(cloud[:20, :3]) + 1.0  # (the special times sit on points that are not dropped for being near)
    poses = W.sweep_poses(POSES[1], rigid(300.0, 20.0, 0.0, 8.0), k)
    want = W.preprocess_sweep_host(cloud, poses, 50, time_field=4)
    assert np.array_equal(both_routes(pre, cloud, poses, 50, time_field=4), want)
    cloud[:, 4] = np.float32(100.0) + np.float32(0.1) * t  # an Ouster-like stamp: seconds within a 100 ms sweep
    want = W.preprocess_sweep_host(cloud, poses, 50, time_field=4, t_begin=100.0, t_end=100.1)
    assert np.array_equal(both_routes(pre, cloud, poses, 50, time_field=4, t_begin=100.0, t_end=100.1), want)
    assert len(want) < n  # the NaN time and the near points are gone


def test_duplicates_across_bins_are_kept_once_at_the_first_index(pre):
    poses = np.broadcast_to(np.eye(4, dtype=np.float32), (2, 4, 4)).copy()
    poses[1, 0, 3] = 100.0
    cloud = np.array([[1.10, 2.0, 2.0], [1.00, 2.0, 2.0], [1.30, 2.0, 2.0], [1.30, 2.0, 2.0]], dtype=np.float32)
    got = both_routes(pre, cloud, poses, 50, columns=2, ring_major=True)
    assert got.tolist() == [[1125, 2025, 2025], [1325, 2025, 2025], [1425, 2025, 2025]]
    # the other way round: the bin-1 point comes first and keeps the place
    got = both_routes(pre, cloud[[1, 0, 2, 3]], poses, 50, columns=4, ring_major=False)  # rows = 1: bins 0 0 1 1
    assert got.tolist() == [[1025, 2025, 2025], [1125, 2025, 2025], [1425, 2025, 2025]]


def test_edge_cases(pre):
    import warpsense_amd as W
    poses = W.sweep_poses(np.eye(4), rigid(100.0, 0.0, 0.0, 3.0), 4)
    empty = pre.preprocess_sweep(np.zeros((0, 3), dtype=np.float32), poses, 50, columns=4)
    assert len(empty) == 0 and empty.to_host().shape == (0, 3)
    near = np.full((128, 3), 0.1, dtype=np.float32)
    assert len(pre.preprocess_sweep(near, poses, 50, columns=4)) == 0
    bad = np.array([[np.nan, 1, 1], [np.inf, 1, 1], [5, 5, 5], [5, 5, 5]], dtype=np.float32)
    assert np.array_equal(both_routes(pre, bad, poses, 50), W.preprocess_sweep_host(bad, poses, 50))


def test_the_range_check_cannot_be_reached(pre):
    """The issue asks for a bin whose translation pushes a point past 2^20 mm and WS_ERR_RANGE.  No such table exists: the
    arithmetic the issue prescribes (wrapping int32 sum, division by 32768) keeps every coordinate within +-65 536 mm (see
    test_sweep_host.test_the_range_check_cannot_be_reached_through_the_fixed_point_matrix).  What can be checked is that the largest
    poses the fixed-point matrix holds go through, wrapped like the host model's."""
    import warpsense_amd as W
    poses = np.broadcast_to(np.eye(4, dtype=np.float32), (2, 4, 4)).copy()
    poses[1, :3, 3] = (65535.0, -65535.0, 65000.0)
    poses[1, :3, :3] *= 900.0
    cloud = np.array([[60.0, -60.0, 2.0], [65.0, 65.0, -65.0], [1.3, 2.0, 2.0], [-3.0, 2.0, 9.0]], dtype=np.float32)
    assert np.array_equal(both_routes(pre, cloud, poses, 50, columns=2), W.preprocess_sweep_host(cloud, poses, 50, columns=2))


def test_refusals_and_a_valid_call_afterwards(pre):
    import ctypes as C
    import warpsense_amd as W
    from warpsense_amd import _lib
    cloud = make_cloud(320, seed=3, stride=5)
    poses = W.sweep_poses(POSES[1], rigid(300.0, 0.0, 0.0, 8.0), 8)
    want = W.preprocess_sweep_host(cloud, poses, 50, columns=64)
    refused = [
        dict(poses=np.zeros((0, 4, 4), dtype=np.float32)),                                   # k = 0
        dict(poses=np.broadcast_to(np.eye(4, dtype=np.float32), (4097, 4, 4))),              # k > 4096
        dict(columns=63),                                                                    # n % columns != 0
        dict(columns=0),
        dict(time_field=0), dict(time_field=2), dict(time_field=5), dict(time_field=9),      # x y z, or beyond the record
        dict(time_field=4, t_begin=1.0, t_end=1.0), dict(time_field=4, t_end=np.inf), dict(time_field=4, t_begin=np.nan),
    ]
    for kw in refused:
        kw = dict(kw)
        P = kw.pop("poses", poses)
        with pytest.raises(W.WsError):
            pre.preprocess_sweep(cloud, P, 50, **({"columns": 64} if not kw else kw))
        assert np.array_equal(pre.preprocess_sweep(cloud, poses, 50, columns=64).to_host(), want)
    with pytest.raises(W.WsError):  # more points than ws_scan_create reserved (4096)
        pre.preprocess_sweep(np.ones((8192, 3), dtype=np.float32), poses, 50, columns=64)
    # NULL arguments, straight at the C ABI
    L, n_out = _lib.load(), C.c_size_t(0)
    rule = _lib.Sweep(64, 1, -1, 0.0, 1.0)
    flat = np.ascontiguousarray(poses.transpose(0, 2, 1)).reshape(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for fn in (L.ws_scan_preprocess_sweep, L.ws_scan_preprocess_sweep_dev):
        assert fn(None, ptr(cloud), 320, 5, ptr(flat), 8, C.byref(rule), 50, C.byref(n_out)) == -1
        assert fn(pre.handle, None, 320, 5, ptr(flat), 8, C.byref(rule), 50, C.byref(n_out)) == -1
        assert fn(pre.handle, ptr(cloud), 320, 5, None, 8, C.byref(rule), 50, C.byref(n_out)) == -1
        assert fn(pre.handle, ptr(cloud), 320, 5, ptr(flat), 8, None, 50, C.byref(n_out)) == -1
    assert np.array_equal(both_routes(pre, cloud, poses, 50, columns=64), want)
    assert np.array_equal(pre.preprocess(cloud, POSES[1], 50).to_host(), W.preprocess_sweep_host(cloud, POSES[1][None], 50))


def test_sweep_output_feeds_update_and_registration():
    """the device-resident output of a sweep goes straight into update_tsdf / register_cloud: same map and pose as the host model's
    points fed from the host"""
    import warpsense_amd as W
    tau, res, size = 1000, 50, (96, 96, 48)
    begin, end = rigid(-100.0, 40.0, 0.0, -3.0), rigid(200.0, 100.0, 0.0, 5.0)
    cloud = S.os1_128_sweep(begin, end, rings=32, azimuths=256, half_extents_mm=(2000.0, 1800.0, 900.0), seed=3)
    poses = W.sweep_poses(end, np.linalg.inv(begin) @ end, 256)
    sensor = end.astype(np.float32)
    params = W.Params(W.MapParams(resolution=res, max_distance=1.0, max_weight=10, size=tuple(s * res / 1000.0 for s in size)))
    out = []
    for mode in ("device", "host"):
        lm = W.LocalMap(*size, tau, 0)
        reg = W.TSDFRegistration(params, lm)
        if mode == "device":
            scan = W.ScanPreprocessor().preprocess_sweep(cloud, poses, res)
        else:
            scan = W.preprocess_sweep_host(cloud, poses, res)
        assert len(scan) > 4000
        reg.update_tsdf(scan, pose=sensor)
        T = reg.register_cloud(scan, S.perturbation(20, -15, 5, 1.0))
        host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
        reg.tsdf().avg_map().to_host(host)
        out.append((host.data_.copy(), T, reg.last_iterations))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_app_with_identity_motion_is_todays_app_and_constant_velocity_follows_the_sensor():
    import warpsense_amd as W
    from scan_clouds import sensor_clouds
    tau, res, mw, size, shift_m = 1000, 50, 640, (128, 128, 64), 0.6
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(s * res / 1000.0 for s in size), shift=shift_m),
                      W.RegistrationParams(200, 0.1, 0.03))
    clouds = sensor_clouds(6, 180.0)
    # the same path with the sensor moving while it turns: sweep k ends at position k and began at position k - 1 (the first stands)
    at = lambda k: rigid(180.0 * max(k, 0), 90.0 * max(k, 0), 0.0, 0.0)  # noqa: E731
    moving = [S.os1_128_sweep(at(k - 1), at(k), rings=32, azimuths=256, half_extents_mm=(2600.0, 2200.0, 1100.0), seed=100 + k) for k in range(6)]
    runs = {}
    for name, kw, call, stream in (("plain", {}, {}, clouds), ("identity", {"sweep_bins": 256}, {"sweep_motion": np.eye(4, dtype=np.float32)}, clouds),
                                   ("deskew", {"deskew": "constant-velocity", "sweep_bins": 256}, {}, moving)):
        app = W.App(params, None, **kw)
        for c in stream:
            app.cloud_callback(c, **call)
        runs[name] = (np.stack(app.poses), app.n_updates, app.n_shifts, [t["points"] for t in app.timings])
        app.terminate()
    assert np.array_equal(runs["plain"][0].view(np.uint32), runs["identity"][0].view(np.uint32))
    assert runs["plain"][1:] == runs["identity"][1:] and runs["plain"][2] >= 1
    # constant velocity on the moving sweeps runs, follows the sensor and shifts the window as before.  (How closely it follows is
    # not asserted: on this small map the registration itself lags -- 792 mm of 900 on the snapshots -- and the motion taken from
    # two lagging poses under-compensates the next sweep: 682 mm of 900 when this was written.  tools/replay_stream.py
    # --moving-sweeps [--deskew] measures the effect on the full-size stream)
    assert runs["deskew"][2] == runs["plain"][2] and runs["deskew"][1] >= 2
    assert np.all(np.isfinite(runs["deskew"][0])) and min(runs["deskew"][3]) > 4000
    print("final positions (plain, deskew):", runs["plain"][0][-1][:3, 3], runs["deskew"][0][-1][:3, 3])
    assert runs["deskew"][0][-1][0, 3] > 0.6 * shift_m * 1000.0  # (it did move: the shift was earned)
    with pytest.raises(ValueError):
        W.App(params, None, deskew="imu")
