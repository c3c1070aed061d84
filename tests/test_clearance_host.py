"""The rules of ws_map_clearance without a GPU: clearance_model.py against answers written down by hand, then ws_clearance_centres and
ws_clearance_margin of the built library (host only, from ws_clearance.h) against the model, and the refusals of the device calls that
need no device."""
import ctypes as C

import numpy as np
import pytest

import clearance_model as CM

Q30 = CM.Q30
IDENT = [Q30, 0, 0, 0, Q30, 0, 0, 0, Q30]
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
RESOLUTIONS = (1, 20, 64, 1000, 1024)


def pose(x=0, y=0, z=0, rot=IDENT):
    return list(rot) + [x, y, z]


# ------------------------------------------------------------------------------------------------ 1. the model against hand-written answers
def test_rotated_offset_rounds_half_up_at_exactly_half_a_millimetre():
    half = 1 << 29
    for rot00, want in [(half, 1), (half - 1, 0), (-half, 0), (-half - 1, -1), (3 * half, 2), (-3 * half, -1)]:
        p = pose(x=7, rot=[rot00, 0, 0, 0, Q30, 0, 0, 0, Q30])
        assert CM.centre(p, (1, 0, 0), 0) == 7 + want, (rot00, want)
    # three terms: 2^29 comes together from 2^28 + 2^28 + 0
    assert CM.centre(pose(rot=[1 << 28, 1 << 28, 5, 0, 0, 0, 0, 0, 0]), (1, 1, 0), 0) == 1
    assert CM.centre(pose(rot=[-(1 << 28), -(1 << 28), 5, 0, 0, 0, 0, 0, 0]), (1, 1, 0), 0) == 0


def test_voxel_is_the_floor_at_negative_coordinates():
    for x, res, want in [(-1, 50, -1), (-50, 50, -1), (-51, 50, -2), (0, 50, 0), (49, 50, 0), (50, 50, 1), (-1, 1, -1), (-1024, 1024, -1), (-1025, 1024, -2)]:
        assert CM.voxel(pose(x=x, y=x, z=x), (0, 0, 0), res) == (want, want, want), (x, res)


# a row of four records along x at res 10: free d2 4, free d2 1, occupied d2 0, unknown d2 4; the body: radius 5 at 0 and at +10 mm in x
ROW = np.array([(1 << 30) | 4, (1 << 30) | 1, (2 << 30) | 0, (0 << 30) | 4], dtype=np.uint32).reshape(4, 1, 1)
BODY = np.array([[0, 0, 0, 5], [10, 0, 0, 5]], dtype=np.int32)
A = [pose(0), pose(10)]    # margins 15, 5 | 5, -5
B = [pose(0), pose(5)]     # margins 15, 5 | 15, 5: the minimum twice
D = [pose(30), pose(30)]   # margins 15 on the unknown record, the second sphere outside


def test_records_by_hand_argmin_tie_first_hit_and_cost_sum():
    rec, per_pose, best = CM.score(ROW, (0, 0, 0), False, 10, np.array([A, B, D]), BODY, soft=10)
    assert rec[0].tolist() == (-5, 1, 65, 1, 0, 0, 0 + 25 + 25 + 225)
    assert rec[1].tolist() == (5, -1, 1, 0, 0, 0, 25 + 25)  # the first of the two samples at 5
    assert rec[2].tolist() == (15, -1, 0, 0, 2, 2, 0)
    assert per_pose[0].tolist() == [(5, 0, 0), (-5, 1, 0)] and per_pose[2].tolist() == [(15, 0, 1), (15, 0, 1)]
    assert best == 1
    # columns: z is ignored and the index has two axes
    rec_c, _, _ = CM.score(ROW.reshape(4, 1), (0, 0, 0), True, 10, np.array([[pose(0, 0, 12345), pose(10, 0, -999)]]), BODY, soft=10)
    assert rec_c[0].tolist() == rec[0].tolist()
    # a trajectory wholly outside
    rec_o, pp_o, best_o = CM.score(ROW, (0, 0, 0), False, 10, np.array([[pose(-25), pose(45)]]), BODY, soft=10)
    assert rec_o[0].tolist() == (CM.NONE, -1, 0xFFFFFFFF, 0, 4, 0, 0) and pp_o[0, 0].tolist() == (CM.NONE, 0, 2) and best_o == -1


def test_best_with_a_tie_and_with_every_trajectory_disqualified():
    assert CM.score(ROW, (0, 0, 0), False, 10, np.array([A, B, B, D]), BODY, soft=10)[2] == 1          # B twice: the lower index
    assert CM.score(ROW, (0, 0, 0), False, 10, np.array([A, B, B, D]), BODY, soft=10, outside_ok=True)[2] == 3  # D costs 0
    assert CM.score(ROW, (0, 0, 0), False, 10, np.array([A, D]), BODY, soft=10)[2] == -1
    assert CM.score(ROW, (0, 0, 0), False, 10, np.array([A, D]), BODY, soft=10, outside_ok=True)[2] == 1
    assert CM.score(ROW, (0, 0, 0), False, 10, np.array([A, A]), BODY, soft=10, outside_ok=True)[2] == -1


# ------------------------------------------------------------------------------------------------ 2. the built library against the model
@pytest.fixture(scope="module")
def L():
    from warpsense_amd import _lib
    return _lib.load()


def lib_centres(L, poses, body, res):
    poses, body = np.ascontiguousarray(poses, dtype=np.int32).reshape(-1, 12), np.ascontiguousarray(body, dtype=np.int32).reshape(-1, 4)
    out = np.full((len(poses), len(body), 3), 77, dtype=np.int32)
    rc = L.ws_clearance_centres(poses.ctypes.data_as(C.c_void_p), len(poses), body.ctypes.data_as(C.c_void_p), len(body), res, out.ctypes.data_as(C.c_void_p))
    return rc, out


def test_centres_of_the_library_on_random_poses_and_at_the_ends_of_every_domain(L):
    rng = np.random.default_rng(5)
    ends_rot, ends_off, ends_pos = [-Q30, -Q30 + 1, -1, 0, 1, Q30 - 1, Q30], [-(1 << 20), -(1 << 20) + 1, -1, 0, 1, 1 << 20], [-Q30 + 1, -1, 0, 1, Q30 - 1]
    poses = np.zeros((300, 12), dtype=np.int64)
    poses[:, :9] = rng.integers(-Q30, Q30 + 1, size=(300, 9))
    poses[:, 9:] = rng.integers(-Q30 + 1, Q30, size=(300, 3))
    poses[:100, :9] = rng.choice(ends_rot, size=(100, 9))   # all nine at an end: the sum reaches +-3 * 2^50
    poses[50:150, 9:] = rng.choice(ends_pos, size=(100, 3))
    for t in range(150, 200):
        poses[t, :9] = CM.rotation_q30(rng, "generic" if t % 2 else "quarter")
    body = np.zeros((64, 4), dtype=np.int64)
    body[:, :3] = rng.integers(-(1 << 20), (1 << 20) + 1, size=(64, 3))
    body[:32, :3] = rng.choice(ends_off, size=(32, 3))
    body[:, 3] = rng.integers(0, 65536, size=64)
    for res in RESOLUTIONS:
        rc, got = lib_centres(L, poses, body, res)
        assert rc == 0 and np.array_equal(got, CM.centres(poses, body, res)), res
    # the half-millimetre cases of the model, through the library
    half = 1 << 29
    for rot00, want in [(half, 1), (half - 1, 0), (-half, 0), (-half - 1, -1)]:
        rc, got = lib_centres(L, [pose(x=7, rot=[rot00, 0, 0, 0, Q30, 0, 0, 0, Q30])], [[1, 0, 0, 0]], 1)
        assert rc == 0 and got[0, 0, 0] == 7 + want


def test_centres_refusals(L):
    ok_pose, ok_body = [pose(1, 2, 3)], [[0, 0, 0, 1]]
    assert lib_centres(L, ok_pose, ok_body, 50)[0] == 0
    for res, rc in [(0, WS_ERR_INVALID), (-3, WS_ERR_INVALID), (1025, WS_ERR_RANGE)]:
        assert lib_centres(L, ok_pose, ok_body, res)[0] == rc
    assert lib_centres(L, ok_pose, np.zeros((65, 4)), 50)[0] == WS_ERR_RANGE
    for bad in ([[(1 << 20) + 1, 0, 0, 1]], [[0, -(1 << 20) - 1, 0, 1]], [[0, 0, 0, -1]], [[0, 0, 0, 65536]]):
        assert lib_centres(L, ok_pose, bad, 50)[0] == WS_ERR_RANGE, bad
    for bad in (pose(Q30), pose(0, -Q30), pose(rot=[Q30 + 1] + IDENT[1:]), pose(rot=IDENT[:8] + [-Q30 - 1])):
        assert lib_centres(L, [bad], ok_body, 50)[0] == WS_ERR_RANGE
    out = np.zeros(3, dtype=np.int32)
    assert L.ws_clearance_centres(None, 1, np.zeros(4, np.int32).ctypes.data_as(C.c_void_p), 1, 50, out.ctypes.data_as(C.c_void_p)) == WS_ERR_INVALID
    assert L.ws_clearance_centres(np.zeros(12, np.int32).ctypes.data_as(C.c_void_p), 1, None, 1, 50, out.ctypes.data_as(C.c_void_p)) == WS_ERR_INVALID
    assert L.ws_clearance_centres(None, 0, np.zeros(4, np.int32).ctypes.data_as(C.c_void_p), 1, 50, None) == 0


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_margin_of_the_library_for_every_d2(L, res):
    import math
    f = L.ws_clearance_margin
    root = [math.isqrt(d2 * res * res) for d2 in range(65026)]
    assert all(r * r <= d2 * res * res < (r + 1) * (r + 1) for d2, r in enumerate(root))
    assert [f(d2, res, 0) for d2 in range(65026)] == root
    assert [f(d2, res, 65535) for d2 in range(0, 65026, 7)] == [root[d2] - 65535 for d2 in range(0, 65026, 7)]
    assert CM.margin(65025, res, 3) == 255 * res - 3 == f(65025, res, 3)


def test_device_calls_refuse_null_handles(L):
    poses, body, best = np.zeros(12, np.int32), np.array([0, 0, 0, 1], np.int32), C.c_int64(5)
    pp, bp = poses.ctypes.data_as(C.c_void_p), body.ctypes.data_as(C.c_void_p)
    n = C.c_size_t(9)
    for owner, tail in (("map", ()), ("store", (50,))):
        for form in ("", "_dev"):
            assert getattr(L, f"ws_{owner}_clearance{form}")(None, pp, 1, 1, bp, 1, 0, *tail, 0, C.byref(best)) == WS_ERR_INVALID
        assert best.value == 5
        for part in ("records", "poses"):
            n.value = 9
            assert getattr(L, f"ws_{owner}_clearance_{part}_dev")(None, C.byref(n)) is None and n.value == 0
        assert getattr(L, f"ws_{owner}_clearance_download")(None, None, None, 0, 0, C.byref(n), None) == WS_ERR_INVALID
    assert L.ws_debug_clearance_timing(None, -1, None) == WS_ERR_INVALID
    assert L.ws_debug_store_clearance_timing(None, -1, None) == WS_ERR_INVALID


def test_python_helpers_make_the_records_of_the_call():
    import warpsense_amd as W
    body = W.body_spheres([[0, 0, 0], [0.3, 0, -0.1]], [0.2, 0.25])
    assert body.dtype == np.int32 and body.tolist() == [[0, 0, 0, 200], [300, 0, -100, 250]]
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [1.0, -2.0, 0.5]
    rows = W.trajectory_poses([[1.0, -2.0, 0.5, np.pi / 2]])
    mats = W.trajectory_poses(T[None])
    assert rows.shape == mats.shape == (1, 12) and mats[0].tolist() == [0, -Q30, 0, Q30, 0, 0, 0, 0, Q30, 1000, -2000, 500]
    assert np.array_equal(rows[0, 9:], mats[0, 9:]) and np.max(np.abs(rows[0, :9].astype(np.int64) - mats[0, :9])) <= 1
    fan = W.arc_rollouts((1.0, 2.0, 0.0, 0.0), [0.5, 1.0], [-0.4, 0.0, 0.4], steps=4, dt=0.5)
    assert fan.shape == (6, 4, 12) and fan.dtype == np.int32
    assert fan[4, :, 9].tolist() == [1500, 2000, 2500, 3000] and fan[4, :, 10].tolist() == [2000] * 4  # speed 1, straight
    assert fan[5, 3, 10] > 2000 > fan[3, 3, 10]  # a positive yaw rate turns to +y
    assert np.array_equal(W.clearance_centres(fan, body, 50), CM.centres(fan.reshape(-1, 12), body, 50).reshape(6, 4, 2, 3))
    assert W.clearance_margin(16, 50, 100) == 100
