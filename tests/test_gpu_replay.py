"""ROS-free replay node: warpsense_amd.App reproduces the sequencing of App::cloud_callback
(src/warpsense/app.cpp:65-117) — checked against the same sequence driven through the CPU oracle."""
import numpy as np
import pytest
from scan_clouds import _angle, oracle_replay, sensor_clouds


pytestmark = pytest.mark.gpu


def test_replay_matches_oracle_sequence(tmp_path):
    import warpsense_amd as W
    from warpsense_amd import build
    tau, res, mw, size = 1000, 50, 640, (128, 128, 64)
    reg = (200, 0.1, 0.03)
    shift_m = 0.6
    h5 = str(tmp_path / "replay.h5") if build.find_hdf5() is not None and build.build_h5() else None
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(s * res / 1000.0 for s in size),
                                  shift=shift_m), W.RegistrationParams(*reg))
    clouds = sensor_clouds(6, 180.0)
    app = W.App(params, h5)
    for c in clouds:
        app.cloud_callback(c)
    want_poses, want_its, want_updates, want_shifts, om = oracle_replay(clouds, app.hdf5_local_map_.size, tau, mw, res, reg, shift_m)
    assert app.n_updates == want_updates >= 2 and app.n_shifts == want_shifts >= 1
    assert [t["iterations"] for t in app.timings] == want_its
    for got, want in zip(app.poses, want_poses):
        assert np.linalg.norm(got[:3, 3] - want[:3, 3]) / 1000.0 < 1e-4
        assert _angle(got[:3, :3], want[:3, :3]) < 1e-4
    # the sensor really moved and the estimate follows it (180 mm per scan along x, 90 mm along y; scan-to-map
    # registration against a map that is only refreshed every 0.3 m lags behind a little)
    assert abs(app.poses[-1][0, 3] - 5 * 180.0) < 200.0 and abs(app.poses[-1][1, 3] - 5 * 90.0) < 100.0
    # bit-identical poses (hard: a one-ulp difference must not skip the map comparison) -> identical final window
    for k, (got, want) in enumerate(zip(app.poses, want_poses)):
        assert np.array_equal(got, want), (k, np.abs(got - want).max())
    lm = app.hdf5_local_map_
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    app.gpu_.tsdf().avg_map().to_host(host)
    assert np.array_equal(host.data_, om.data)
    app.terminate()
    if h5:
        g = W.GlobalMap(tau, 0, filename=h5, open_existing=True)
        import ctypes as C
        n = C.c_int64(0)
        g._H.ws_h5_num_poses(g._file, C.byref(n))
        assert n.value == len(clouds)
        vals = np.zeros(7, dtype=np.float32)
        g._H.ws_h5_read_pose(g._file, len(clouds) - 1, vals.ctypes.data_as(C.c_void_p))
        assert np.allclose(vals[:3], app.poses[-1][:3, 3] / 1000.0, atol=6e-4)
        g.close()
