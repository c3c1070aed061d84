"""ws_register_cloud_batch on the GPU: K registrations of one cloud, one workgroup per start pose, against the single call
(bit for bit), against perform_registration (the scores) and against the CPU oracle; relocalize on the committed kidnap case.

The scene, the cloud, the pose list and the kidnap case are constants of this file; tests/test_reg_batch_host.py proves on the
oracle alone that they exercise what they are meant to (every way a loop ends, a lattice that contains the right basin)."""
import numpy as np
import pytest

import oracle_lib as O
from reg_scenes import EPSILON, FAR_AWAY, IT_WEIGHT_GRADIENT, KIDNAP_BEST, KIDNAP_LATTICE, KIDNAP_MAX_ITERATIONS, KIDNAP_MIN_FRACTION, MAX_ITERATIONS, ORACLE_ITERATIONS, POSES, SCENE, batch, batch_cloud, check_batch_equals_single, kidnap_case, pose_list
import reg_scenes as R
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    reg, oa, pts, res = R.build_scene(**SCENE)
    q = batch_cloud(pts)
    reg.reg_.prepare_registration(q)
    return reg, oa, q, res


@pytest.mark.parametrize("k", [1, 2, 7, 64, 300])
def test_batch_equals_single(scene, k):
    """T_out[k], iterations[k] == ws_register_cloud alone, in both loop modes; 300 workgroups exceed the 256 compute units"""
    reg, oa, q, res = scene
    reg.reg_.flags = 0
    reg.reg_.prepare_registration(q)
    T, it, e, c = check_batch_equals_single(reg, pose_list(k), MAX_ITERATIONS, res)
    if k >= len(POSES):
        assert it[FAR_AWAY] == 1 and c[FAR_AWAY] == 0 and e[FAR_AWAY] == 0
        assert np.array_equal(T[FAR_AWAY], S.perturbation(*POSES[FAR_AWAY]))
        assert len(set(it[:len(POSES)].tolist())) >= 4 and (it == MAX_ITERATIONS).any() and (it[c > 0] < MAX_ITERATIONS).any()


@pytest.mark.parametrize("max_it", [0, 1, 2, 7, 200])
def test_batch_equals_single_for_every_iteration_limit(scene, max_it):
    reg, oa, q, res = scene
    reg.reg_.flags = 0
    reg.reg_.prepare_registration(q)
    poses = pose_list(len(POSES))
    T, it, e, c = check_batch_equals_single(reg, poses, max_it, res)
    assert (it <= max_it).all()
    if max_it == 0:
        # nothing moves, and the score is that of the start pose
        assert np.array_equal(T, poses) and not it.any()
        assert c[0] > 1000 and e[0] > 0


@pytest.mark.parametrize("flags", [0, 1])
def test_batch_equals_single_for_both_flags(scene, flags):
    reg, oa, q, res = scene
    reg.reg_.flags = flags
    try:
        reg.reg_.prepare_registration(q[:8192 - 13])  # (N % 32 != 0: the compat launch drops the tail)
        T, it, e, c = check_batch_equals_single(reg, pose_list(7), 25, res)
        for k in range(7):
            assert (int(e[k]), int(c[k])) == O.reg_iterate(oa, T[k], q[:8192 - 13], res, flags)[2:]
    finally:
        reg.reg_.flags = 0


@pytest.mark.parametrize("n", [0, 5, 1000, 65536 + 77, 200_000])
def test_batch_equals_single_for_ragged_point_counts(scene, n):
    """no point, fewer points than lanes, a ragged tail, more than one point per lane, beyond the compat launch's 65 536"""
    reg, oa, q, res = scene
    rng = np.random.default_rng(n)
    qn = q[rng.integers(0, q.shape[0], n)] if n else np.zeros((0, 3), dtype=np.int32)
    for flags in (0, 1):
        reg.reg_.flags = flags
        try:
            reg.reg_.prepare_registration(qn)
            T, it, e, c = check_batch_equals_single(reg, pose_list(7), 12, res)
            if n == 0:
                assert not c.any() and (it == 1).all() and np.array_equal(T, pose_list(7))
            for k in (0, 4):
                assert (int(e[k]), int(c[k])) == O.reg_iterate(oa, T[k], qn, res, flags)[2:]
        finally:
            reg.reg_.flags = 0


def test_batch_matches_the_oracle(scene):
    """per hypothesis: the oracle's iteration count, its pose within 1e-4 m / 1e-4 rad (the bound of
    test_register_cloud_matches_oracle_pose), and the oracle's e, c at the device's final pose"""
    reg, oa, q, res = scene
    reg.reg_.flags = 0
    reg.reg_.prepare_registration(q)
    poses = pose_list(len(POSES))
    T, it, e, c = batch(reg, poses, MAX_ITERATIONS, res)
    assert it.tolist() == ORACLE_ITERATIONS
    for k in range(len(POSES)):
        To, ito, _ = O.register_cloud(oa, q, poses[k], MAX_ITERATIONS, IT_WEIGHT_GRADIENT, EPSILON, res)
        dt, ang = R.pose_error(T[k], To)
        print(k, it[k], ito, dt, ang)
        assert it[k] == ito and dt < 1e-4 and ang < 1e-4, (k, it[k], ito, dt, ang)
        assert (int(e[k]), int(c[k])) == O.reg_iterate(oa, T[k], q, res, 0)[2:], k


def test_order_independence_and_repeatability(scene):
    reg, oa, q, res = scene
    reg.reg_.flags = 0
    reg.reg_.prepare_registration(q)
    poses = pose_list(40)
    a = batch(reg, poses, 60, res)
    b = batch(reg, poses, 60, res)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    perm = np.random.default_rng(5).permutation(40)
    p = batch(reg, poses[perm], 60, res)
    for x, y in zip(a, p):
        assert np.array_equal(x[perm].view(np.uint32) if x.dtype == np.float32 else x[perm], y.view(np.uint32) if y.dtype == np.float32 else y)


def test_batch_leaves_the_single_route_alone(scene):
    """register_cloud before and after a batch on the same handle: identical bytes, identical last sums, in both loop modes"""
    import warpsense_amd as W
    reg, oa, q, res = scene
    reg.reg_.flags = 0
    reg.reg_.prepare_registration(q)
    P = S.perturbation(*POSES[2])
    try:
        for mode in (W.WS_REG_LOOP_RESIDENT, W.WS_REG_LOOP_LAUNCHES):
            reg.reg_.set_loop(mode)
            T0, it0 = reg.reg_.register_cloud(reg.tsdf().device_map(), P, MAX_ITERATIONS, IT_WEIGHT_GRADIENT, EPSILON, res)
            s0 = reg.reg_.last_sums()
            batch(reg, pose_list(9), 30, res)
            s1 = reg.reg_.last_sums()
            T1, it1 = reg.reg_.register_cloud(reg.tsdf().device_map(), P, MAX_ITERATIONS, IT_WEIGHT_GRADIENT, EPSILON, res)
            assert it0 == it1 == ORACLE_ITERATIONS[2] and T0.tobytes() == T1.tobytes()
            for x, y in zip(s0, s1):
                assert np.array_equal(x, y)
    finally:
        reg.reg_.set_loop(W.WS_REG_LOOP_RESIDENT)


@pytest.mark.timeout(60, method="thread")
def test_batch_after_the_resident_server(scene):
    """perform_registration leaves a resident server on the stream (idle time raised to 2 s here): the batch asks it to leave
    instead of waiting behind it, and is right"""
    import ctypes as C
    import time
    reg, oa, q, res = scene
    r = reg.reg_
    r.flags = 0
    r.prepare_registration(q)
    poses = pose_list(5)
    want = batch(reg, poses, 30, res)
    launches = C.c_int32(0)
    assert r._L.ws_debug_reg_server(r.handle, 1, 2_000_000, C.byref(launches)) == 0
    try:
        hgec = r.perform_registration(reg.tsdf().device_map(), poses[1], res)
        t0 = time.perf_counter()
        got = batch(reg, poses, 30, res)
        dt = time.perf_counter() - t0
        assert dt < 1.0, dt  # (2 s if it had queued behind the idle server)
        for x, y in zip(want, got):
            assert x.tobytes() == y.tobytes()
        # and the server route still answers afterwards
        again = r.perform_registration(reg.tsdf().device_map(), poses[1], res)
        assert np.array_equal(hgec[0], again[0]) and hgec[2:] == again[2:]
    finally:
        r._L.ws_debug_reg_server(r.handle, 1, 50, C.byref(launches))


def test_invalid_arguments(scene):
    import ctypes as C
    reg, oa, q, res = scene
    r = reg.reg_
    L = r._L
    T = np.zeros((2, 16), dtype=np.float32)
    out = np.zeros((2, 16), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    m = reg.tsdf().device_map()
    args = (5, C.c_float(0.1), C.c_float(0.03))
    WS_ERR_INVALID = -1
    assert L.ws_register_cloud_batch(r.handle, m, None, 2, *args, res, 0, p(out), None, None, None) == WS_ERR_INVALID
    assert L.ws_register_cloud_batch(r.handle, m, p(T), 2, *args, res, 0, None, None, None, None) == WS_ERR_INVALID
    assert L.ws_register_cloud_batch(r.handle, m, p(T), 2, *args, 0, 0, p(out), None, None, None) == WS_ERR_INVALID
    assert L.ws_register_cloud_batch(r.handle, m, None, 0, *args, res, 0, None, None, None, None) == 0
    T, it, e, c = batch(reg, np.zeros((0, 4, 4), dtype=np.float32), 5, res)
    assert T.shape == (0, 4, 4) and it.shape == (0,)


def test_relocalize_on_the_kidnap_case():
    """the candidate the oracle-side host test predicted, and the oracle's pose for that candidate within 1e-4 m / 1e-4 rad"""
    import warpsense_amd as W
    reg, oa, pts, res = R.build_scene(scans=2)
    q, truth, guess = kidnap_case(pts)
    reg.params_.registration.max_iterations = KIDNAP_MAX_ITERATIONS
    pose, best, table = reg.relocalize(q, guess, min_fraction=KIDNAP_MIN_FRACTION, **KIDNAP_LATTICE)
    assert best == KIDNAP_BEST and len(table["pose"]) == 125
    assert np.array_equal(pose, table["pose"][best])
    prm = reg.params_.registration
    To, ito, _ = O.register_cloud(oa, q, table["start"][best], KIDNAP_MAX_ITERATIONS, prm.it_weight_gradient, prm.epsilon, res)
    dt, ang = R.pose_error(pose, To)
    assert table["iterations"][best] == ito and dt < 1e-4 and ang < 1e-4, (dt, ang)
    dt, ang = R.pose_error(pose, truth)
    assert dt < 1e-2 and ang < 1e-2, (dt, ang)
    # from the wrong guess alone (candidate 0) the same registration stays lost
    assert R.pose_error(table["pose"][0], truth)[0] > 0.5
    # nobody reaches an impossible fraction
    with pytest.raises(W.WsError):
        reg.relocalize(q, guess, min_fraction=1.01, **KIDNAP_LATTICE)
