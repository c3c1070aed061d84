"""Motion-compensated scan pre-processing, the parts that need no GPU: the ABI symbols, ws_sweep_poses against a numpy restatement,
the host model preprocess_sweep_host against the C oracle (k = 1) and against the geometry of a room seen from a moving sensor,
and the bin rule at its edges."""
import numpy as np
import pytest

import oracle_lib as O
from scan_clouds import POSES, make_cloud
from scan_clouds import rigid
from warpsense_amd import synthetic as S

ROOM = (2000.0, 1800.0, 900.0)


def numpy_sweep_poses(pose_end, motion, k):
    """restatement of ws_sweep_poses in numpy double on the float32 inputs: pose_end @ rel((b + 0.5) / k), rotation of rel(s) =
    exp((1 - s) log(R^T)) by axis and angle (Rodrigues), translation (1 - s) (-R^T t); rounded to float32 at the end"""
    E = np.asarray(pose_end, dtype=np.float32).astype(np.float64)
    Mo = np.asarray(motion, dtype=np.float32).astype(np.float64)
    Q = Mo[:3, :3].T
    u = -(Q @ Mo[:3, 3])
    v = 0.5 * np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    sn = np.sqrt(v @ v)
    angle = np.arctan2(sn, 0.5 * (Q[0, 0] + Q[1, 1] + Q[2, 2] - 1.0))
    a = v / sn if sn > 0 else np.zeros(3)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    out = np.zeros((k, 4, 4), dtype=np.float32)
    for b in range(k):
        w = 1.0 - (b + 0.5) / k
        rel = np.eye(4)
        rel[:3, :3] = np.eye(3) + np.sin(w * angle) * K + (1.0 - np.cos(w * angle)) * (K @ K)
        rel[:3, 3] = w * u
        out[b] = (E @ rel).astype(np.float32)
    return out


def ulps(a, b):
    """distance of two float32 arrays in units of the larger one's ulp"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def test_new_symbols_are_present_and_sweep_poses_runs_without_a_device():
    import warpsense_amd as W
    from warpsense_amd import _lib
    L = _lib.load()
    for name in ("ws_sweep_poses", "ws_scan_preprocess_sweep", "ws_scan_preprocess_sweep_dev"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("sweep_poses", "preprocess_sweep_host"):
        assert hasattr(W, name), name
    assert hasattr(W.ScanPreprocessor, "preprocess_sweep") and hasattr(S, "os1_128_sweep")
    assert W.sweep_poses(np.eye(4), rigid(100, 0, 0, 2.0), 4).shape == (4, 4, 4)


@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_sweep_poses_matches_the_numpy_restatement_within_one_ulp(k):
    """both sides evaluate the same formula in double, far below a float32 ulp, and differ only where the final rounding falls"""
    import warpsense_amd as W
    for pose_end, motion in [(POSES[1], rigid(300, -40, 10, 8.0)), (POSES[2], rigid(-250, 120, -30, -15.0, 6.0)), (np.eye(4), rigid(0, 0, 0, 89.0)),
                             (POSES[1], rigid(400, 0, 0, 0.0))]:
        got = W.sweep_poses(pose_end, motion, k)
        want = numpy_sweep_poses(pose_end, motion, k)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.all(ulps(got, want) <= 1.0), ulps(got, want).max()


def test_bin_zero_of_one_is_the_pose_at_half_the_sweep():
    import warpsense_amd as W
    begin, end = rigid(1000, 500, 0, 20.0), rigid(1400, 560, 20, 30.0)
    motion = np.linalg.inv(begin) @ end
    got = W.sweep_poses(end, motion, 1)[0].astype(np.float64)
    half = S.sweep_pose_at(begin, end, 0.5)
    assert np.abs(got[:3, :3] - half[:3, :3]).max() < 1e-6 and np.abs(got[:3, 3] - half[:3, 3]).max() < 1e-3
    # half way: half the yaw (25 degrees)
    assert abs(np.rad2deg(np.arctan2(got[1, 0], got[0, 0])) - 25.0) < 1e-4


@pytest.mark.parametrize("k", [1, 7, 1024])
def test_identity_motion_returns_the_end_pose_bit_for_bit(k):
    import warpsense_amd as W
    for pose in POSES:
        got = W.sweep_poses(pose, np.eye(4), k)
        assert got.shape == (k, 4, 4)
        assert np.array_equal(got.view(np.uint32), np.broadcast_to(np.asarray(pose, dtype=np.float32), (k, 4, 4)).view(np.uint32))


def test_first_and_last_pose_approach_the_ends_of_the_sweep_as_one_over_k():
    import warpsense_amd as W
    end, motion = POSES[1].astype(np.float64), rigid(400, 50, -20, 10.0)
    begin = end @ np.linalg.inv(motion)
    gaps = []
    for k in (16, 64, 256, 1024):
        P = W.sweep_poses(end, motion, k).astype(np.float64)
        gaps.append((np.linalg.norm(P[0][:3, 3] - begin[:3, 3]), np.linalg.norm(P[-1][:3, 3] - end[:3, 3]), np.abs(P[0][:3, :3] - begin[:3, :3]).max()))
    gaps = np.array(gaps)
    # the centre of the first / last bin is half a bin from the end of the sweep: ~|motion| / (2 k)
    assert np.all(gaps[:, 0] < 1.05 * 404.0 / (2 * np.array([16, 64, 256, 1024])) + 1e-3)
    for col in (0, 1):
        ratio = gaps[:-1, col] / gaps[1:, col]
        assert np.all(np.abs(ratio[:2] - 4.0) < 0.2), ratio  # k x 4 -> gap / 4
    assert gaps[-1, 2] < 2e-4


def test_sweep_poses_refusals():
    import warpsense_amd as W
    bad = np.eye(4)
    bad[0, 3] = np.nan
    with pytest.raises(W.WsError):
        W.sweep_poses(np.eye(4), rigid(0, 0, 0, 91.0), 4)
    with pytest.raises(W.WsError):
        W.sweep_poses(np.eye(4), bad, 4)
    with pytest.raises(W.WsError):
        W.sweep_poses(bad, np.eye(4), 4)
    with pytest.raises(W.WsError):
        W.sweep_poses(np.eye(4), np.eye(4), 0)
    with pytest.raises(W.WsError):
        W.sweep_poses(np.eye(4), np.eye(4), 4097)
    assert W.sweep_poses(np.eye(4), rigid(0, 0, 0, 89.0), 4).shape == (4, 4, 4)  # the next valid call works


@pytest.mark.parametrize("res,stride", [(50, 3), (64, 5), (20, 3)])
def test_host_model_with_one_bin_is_the_oracle_bit_for_bit(res, stride):
    import warpsense_amd as W
    cloud = make_cloud(3000, seed=res, stride=stride)
    for pose in POSES:
        want = O.preprocess(cloud, pose, res)
        got = W.preprocess_sweep_host(cloud, np.asarray(pose, dtype=np.float32)[None], res)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        got = W.preprocess_sweep_host(cloud, np.asarray(pose, dtype=np.float32)[None], res, columns=3000, ring_major=False)
        assert np.array_equal(got, want)
    one = np.array([[3.0, -2.0, 1.0] + [0.0] * (stride - 3)], dtype=np.float32)
    assert np.array_equal(W.preprocess_sweep_host(one, POSES[1][None], res), O.preprocess(one, POSES[1], res))


def wall_distance(pts_mm):
    p = np.asarray(pts_mm, dtype=np.float64)
    return np.abs(np.abs(p) - np.asarray(ROOM)[None, :]).min(axis=1)


def moving_sweep():
    """rings 16 x azimuths 64 in the 2000 x 1800 x 900 mm room; the sensor moves 400 mm and yaws 10 degrees during the sweep"""
    begin, end = rigid(-200.0, 100.0, 0.0, 5.0), rigid(-200.0 + 400.0 * np.cos(0.3), 100.0 + 400.0 * np.sin(0.3), 0.0, 15.0)
    cloud = S.os1_128_sweep(begin, end, rings=16, azimuths=64, half_extents_mm=ROOM, seed=5, noise=False)
    return begin, end, cloud


def test_deskewed_points_lie_on_the_walls_and_the_plain_route_does_not_put_them_there():
    """Every ray of the sweep ends ON a wall (no range noise).  What moves a pre-processed point away from its wall plane:
      - the snap to the voxel centre in the sensor frame: at most res / 2 per axis, res * sqrt(3) / 2 in length (a rotation
        keeps lengths);
      - the fixed-point matrix: each of the 9 rotation entries is truncated to a multiple of 1 / 32768, the snapped coordinates are
        below 3000 mm (the room's half diagonal is 2839 mm, the sensor stays within 450 mm of the centre: ranges < 3300 mm, but a
        single coordinate < 2450 mm), so three products lose at most 3 * 3000 / 32768 = 0.28 mm per axis, the translation 1 / 32768;
      - the truncating division by 32768: below 1 mm per axis;
      - the float32 forms of the cloud in metres (3 m: 2.4e-4 mm) and of the pose (ws_sweep_poses rounds a translation of at most
        500 mm to 3e-5 mm and rotation entries to 6e-8, times 3000 mm: 2e-4 mm per product): below 0.002 mm per axis.
    Per axis 0.28 + 1 + 0.002 < 1.3 mm, in length < 1.3 * sqrt(3) = 2.25 mm < 3 mm.  The bin of a column is the column (k =
    azimuths), and its pose is the pose the column was cast from.  So: distance to the nearest wall plane <= res * sqrt(3) / 2 + 3."""
    import warpsense_amd as W
    res = 50
    begin, end, cloud = moving_sweep()
    assert cloud.shape == (16 * 64, 3) and cloud.dtype == np.float32
    motion = np.linalg.inv(begin) @ end
    assert abs(np.linalg.norm(motion[:3, 3]) - 400.0) < 1e-6
    pts = W.preprocess_sweep_host(cloud, W.sweep_poses(end, motion, 64), res)
    bound = res * np.sqrt(3.0) / 2.0 + 3.0
    assert len(pts) > 500
    d = wall_distance(pts)
    print(f"de-skewed: max wall distance {d.max():.3f} mm (bound {bound:.3f})")
    assert d.max() <= bound, d.max()
    plain = O.preprocess(cloud, end.astype(np.float32), res)
    dp = wall_distance(plain)
    print(f"one pose: max wall distance {dp.max():.3f} mm")
    assert dp.max() > bound  # otherwise the input shows nothing
    # the time field says the same as the index
    timed = S.os1_128_sweep(begin, end, rings=16, azimuths=64, half_extents_mm=ROOM, seed=5, noise=False, with_time=True)
    assert timed.shape == (1024, 4) and np.array_equal(timed[:, :3], cloud)
    assert np.array_equal(W.preprocess_sweep_host(timed, W.sweep_poses(end, motion, 64), res, time_field=3), pts)


def test_a_still_sweep_is_the_snapshot():
    """pose_begin == pose_end: every column is cast from the one pose, so the sweep is os1_128_scan seen from the sensor"""
    T = rigid(300.0, -200.0, 50.0, 0.0)
    cloud = S.os1_128_sweep(T, T, rings=8, azimuths=32, half_extents_mm=ROOM, seed=9)
    snap = S.os1_128_scan(sensor_mm=(300.0, -200.0, 50.0), rings=8, azimuths=32, half_extents_mm=ROOM, seed=9)
    assert np.abs(cloud.astype(np.float64) * 1000.0 + T[:3, 3] - snap).max() < 1.0 + 1e-3  # (the snapshot truncates to mm)


def test_bin_rule_at_its_edges():
    import warpsense_amd as W
    k = 8
    t = np.array([0.0, 1.0, -0.5, 2.5, np.nan, 0.125, 0.25, 0.875, np.nextafter(np.float32(0.25), np.float32(0)), np.inf, -np.inf], dtype=np.float32)
    cloud = np.zeros((len(t), 5), dtype=np.float32)
    cloud[:, 0] = 1.0
    cloud[:, 1] = 1.0 + np.arange(len(t))  # distinct points
    cloud[:, 4] = t
    b = W.sweep_bins(len(t), k, cloud, time_field=4)
    #                 t_begin t_end below above NaN  s*k = 1 -> upper  s*k = 2   7   just below 2   +inf  -inf
    assert b.tolist() == [0, k - 1, 0, k - 1, -1, 1, 2, 7, 1, k - 1, 0]
    # other bounds: s = (t - 10) / (12 - 10)
    t[8] = 0.375  # (one ulp below 0.25 does not survive 10 + 2 t in float32)
    b[8] = 3
    cloud[:, 4] = np.float32(10.0) + np.float32(2.0) * t
    assert W.sweep_bins(len(t), k, cloud, time_field=4, t_begin=10.0, t_end=12.0).tolist() == b.tolist()
    # a NaN time drops the point, whatever its coordinates
    poses = np.broadcast_to(np.eye(4, dtype=np.float32), (k, 4, 4)).copy()
    poses[:, 0, 3] = 1000.0 * np.arange(k)  # the bin shows in x
    out = W.preprocess_sweep_host(cloud, poses, 50, time_field=4, t_begin=10.0, t_end=12.0)
    assert len(out) == len(t) - 1
    assert out[:, 0].tolist() == [1025 + 1000 * bb for bb in b.tolist() if bb >= 0]
    assert out[:, 1].tolist() == [1025 + 1000 * i for i, bb in enumerate(b.tolist()) if bb >= 0]
    # by index: ring-major and column-major, k that does not divide the columns
    assert W.sweep_bins(12, 2, columns=3, ring_major=True).tolist() == [0, 0, 1] * 4          # col * 2 // 3
    assert W.sweep_bins(12, 2, columns=3, ring_major=False).tolist() == [0] * 8 + [1] * 4
    assert W.sweep_bins(6, 7, columns=3).tolist() == [0, 2, 4, 0, 2, 4]                          # more bins than columns
    for bad in (dict(columns=5), dict(columns=0)):
        with pytest.raises(ValueError):
            W.sweep_bins(12, 2, **bad)
    for bad in (dict(time_field=2), dict(time_field=5), dict(time_field=4, t_begin=1.0, t_end=1.0), dict(time_field=4, t_end=np.inf)):
        with pytest.raises(ValueError):
            W.sweep_bins(len(t), k, cloud, **bad)
    with pytest.raises(ValueError):
        W.sweep_bins(12, 0, columns=3)
    with pytest.raises(ValueError):
        W.sweep_bins(12, 4097, columns=3)


def test_duplicates_across_bins_are_kept_once_at_the_first_position():
    import warpsense_amd as W
    poses = np.broadcast_to(np.eye(4, dtype=np.float32), (2, 4, 4)).copy()
    poses[1, 0, 3] = 100.0  # bin 1 is 100 mm further along x
    # columns 0, 1 -> bins 0, 1.  (1.10 m in bin 0) and (1.00 m in bin 1) both land on x = 1125
    cloud = np.array([[1.10, 2.0, 2.0], [1.00, 2.0, 2.0], [1.30, 2.0, 2.0], [1.30, 2.0, 2.0]], dtype=np.float32)
    out = W.preprocess_sweep_host(cloud, poses, 50, columns=2, ring_major=True)
    assert out.tolist() == [[1125, 2025, 2025], [1325, 2025, 2025], [1425, 2025, 2025]]


def test_the_range_check_cannot_be_reached_through_the_fixed_point_matrix():
    """WS_ERR_RANGE guards the 21-bit fields of the hash key.  With the arithmetic the sweep shares with the plain call -- a wrapping
    int32 sum divided by 32768 -- every coordinate lies within +-2^31 / 32768 = +-65 536 mm < 2^20 mm, whatever the pose: the
    largest translation to_int_mat can hold is 65 535 mm, and beyond it the products wrap (as in the reference).  So no pose
    table makes the call fail with WS_ERR_RANGE; the check stays in the kernel for the day the arithmetic widens."""
    import warpsense_amd as W
    poses = np.broadcast_to(np.eye(4, dtype=np.float32), (2, 4, 4)).copy()
    poses[1, :3, 3] = (65535.0, -65535.0, 65000.0)
    poses[1, :3, :3] *= 900.0  # (and a "rotation" that wraps every product)
    cloud = np.array([[60.0, -60.0, 2.0], [65.0, 65.0, -65.0], [1.3, 2.0, 2.0], [-3.0, 2.0, 9.0]], dtype=np.float32)
    out = W.preprocess_sweep_host(cloud, poses, 50, columns=2)
    assert len(out) == 4 and np.abs(out).max() <= 65536
