"""ws_map_clearance (the rules are stated in include/warpsense_hip.h) against clearance_model.py applied to the distance records of
distance_model.py: raw bytes of the trajectory records, the pose records and `best`.  Every scene is checked on the CPU before the
device is asked.

The shapes (T, P, K) are those at which the kernel can go wrong: one sample; a body of 64 spheres (a group is a whole wave); 67 poses of 3
spheres (groups of 4 lanes, 64 poses a round: more than one round, the last one nearly empty); 300 poses of one sphere (more than 256
samples per workgroup).  The conditions of clearance_model.conditions hold for the shapes with T >= 2 (of two trajectories one hits, and the other is
the best); the one-sample shape must still have its sample inside the box."""
import ctypes as C

import numpy as np
import pytest

import clearance_model as CM
import distance_model as DM
from frontier_scenes import RES
from query_model import same
from reach_scenes import R, make_window, random_box

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
ROTATED = dict(pos=(3, -2, 5), offset=(7, 4, 9))  # every axis of the ring wraps inside the window
SOFT = 60
# (T, P, K): seed, steps of the walk in voxels, largest radius in mm -- picked on the CPU so that the model meets the conditions
SCENES = {(1, 1, 1): (1, 0.4, 40), (3, 5, 64): (4, 0.4, 40), (70, 67, 3): (1, 0.15, 40), (2, 300, 1): (15, 0.05, 40)}
assert R * RES >= 40 + SOFT


def scene(shape, lo, ext):
    T, P, K = shape
    seed, walk, radius = SCENES[shape]
    rng = np.random.default_rng(seed)
    return CM.draw_poses(rng, T, P, lo, ext, RES, walk), CM.draw_body(rng, K, RES, radius)


def bytes_equal(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check_scene(shape, want, best):
    if shape[0] >= 2:
        CM.conditions(want, best, shape[0])
    else:
        assert np.any(want["min_margin"] != CM.NONE)


def compare(w, rec, lo, columns, shape, poses, body, **kw):
    """the model first, then the device: host form and device form, with and without pose records"""
    want, want_pp, best = CM.score(rec, lo, columns, RES, poses, body, SOFT)
    _, _, best_ok = CM.score(rec, lo, columns, RES, poses, body, SOFT, outside_ok=True)
    check_scene(shape, want, best)
    got = w.clearance(poses, body, SOFT, per_pose=True)
    assert bytes_equal(got.records, want.astype(got.records.dtype)) and bytes_equal(got.poses, want_pp.astype(got.poses.dtype)) and got.best == best
    plain = w.clearance(poses, body, SOFT, outside_ok=True)
    assert plain.poses is None and bytes_equal(plain.records, got.records) and plain.best == best_ok
    return want, want_pp, best, best_ok


@pytest.fixture(scope="module")
def random_window():
    box = random_box()
    t, lo, hi = make_window(box, **ROTATED)
    assert np.any(lo < 0)  # negative world coordinates
    yield t, lo, hi, box
    t.close()


@pytest.mark.parametrize("shape", list(SCENES))
def test_volume_matches_the_model(random_window, shape):
    t, lo, hi, box = random_window
    rec, _ = DM.model_box(box, R)
    poses, body = scene(shape, lo, box.shape)
    w = t.avg_map()
    assert same(w.distance(max_dist_vox=R), rec)
    compare(w, rec, lo, False, shape, poses, body)


@pytest.mark.parametrize("shape", list(SCENES))
def test_columns_match_the_model_and_z_is_ignored(random_window, shape):
    t, lo, hi, box = random_window
    zlo, zhi = np.array([lo[0], lo[1], lo[2] + 19]), np.array([hi[0], hi[1], lo[2] + 20])  # the unknown top layer and the one below: some columns are unknown
    rec, _ = DM.model_box(box[:, :, 19:21], R, columns=True)
    poses, body = scene(shape, lo, box.shape)
    poses[::2, :, 11] += 100000  # z of a pose does not count
    w = t.avg_map()
    assert same(w.distance(lo=zlo, hi=zhi, max_dist_vox=R, columns=True), rec)
    compare(w, rec, zlo, True, shape, poses, body)


@pytest.mark.parametrize("shape", list(SCENES))
def test_unknown_occupied_makes_unknown_samples_hits(random_window, shape):
    """Here a tenth of the voxels are sites, and a body of 64 spheres meets one at every pose: no seed gives the (3, 5, 64) scene a
    trajectory without a hit, so `best` is -1 there.  What this run is about is asserted on the model instead: every unknown sample is a
    hit, some are there, and from three trajectories on some trajectory hits and some has outside samples."""
    t, lo, hi, box = random_window
    rec, _ = DM.model_box(box, R, unknown_occupied=True)
    poses, body = scene(shape, lo, box.shape)
    w = t.avg_map()
    assert same(w.distance(max_dist_vox=R, unknown_occupied=True), rec)
    want, want_pp, best = CM.score(rec, lo, False, RES, poses, body, SOFT)
    assert np.all(want["hits"] >= want["unknown"])  # an unknown record is a site: d2 = 0
    if shape[0] >= 2:
        assert np.any(want["unknown"] > 0) and np.any(want["hits"] > 0) and np.any(want["outside"] > 0)
    got = w.clearance(poses, body, SOFT, per_pose=True)
    assert bytes_equal(got.records, want.astype(got.records.dtype)) and bytes_equal(got.poses, want_pp.astype(got.poses.dtype)) and got.best == best


@pytest.mark.parametrize("shape", list(SCENES))
def test_over_a_ground_distance_result(random_window, shape):
    """The records are those the bridge left on the device (its own tests hold them to the ground model): the seeds cannot be picked for
    them without a GPU, so of the conditions only those are asserted that the scene has by construction."""
    t, lo, hi, box = random_window
    w = t.avg_map()
    g = w.ground(clear_vox=2)
    rec = w.ground_distance(max_step_q8=512, max_dist_vox=R)  # the bridge REPLACES the distance result; its records are the model's input
    assert rec.shape == box.shape[:2] and len(np.unique(rec >> 30)) >= 2
    poses, body = scene(shape, lo, box.shape)
    want, want_pp, best = CM.score(rec, g.lo, True, RES, poses, body, SOFT)
    assert np.any(want["min_margin"] != CM.NONE) and (shape[0] < 2 or np.any(want["outside"] > 0))
    got = w.clearance(poses, body, SOFT, per_pose=True)
    assert bytes_equal(got.records, want.astype(got.records.dtype)) and bytes_equal(got.poses, want_pp.astype(got.poses.dtype)) and got.best == best


def test_device_form_download_prefixes_and_device_tensors(random_window):
    import torch
    t, lo, hi, box = random_window
    shape = (70, 67, 3)
    rec, _ = DM.model_box(box, R)
    poses, body = scene(shape, lo, box.shape)
    w = t.avg_map()
    assert same(w.distance(max_dist_vox=R), rec)
    host = w.clearance(poses, body, SOFT, per_pose=True)
    dev = w.clearance(torch.from_numpy(poses).cuda(), body, SOFT, per_pose=True, device=True)
    assert dev.best == host.best
    assert dev.records.cpu().numpy().tobytes() == host.records.tobytes() and dev.poses.cpu().numpy().tobytes() == host.poses.tobytes()
    # prefixes: the totals are always reported, nothing is written beyond the capacities
    L, T, P = t._L, shape[0], shape[1]
    a = np.full(5, 0x55, dtype=host.records.dtype)
    b = np.full(9, 0x55, dtype=host.poses.dtype)
    filler_a, filler_b = a[0].tobytes(), b[0].tobytes()
    n, m = C.c_size_t(0), C.c_size_t(0)
    assert L.ws_map_clearance_download(t.handle, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 3, 7, C.byref(n), C.byref(m)) == 0
    assert (n.value, m.value) == (T, T * P)
    assert a[:3].tobytes() == host.records[:3].tobytes() and b[:7].tobytes() == host.poses.reshape(-1)[:7].tobytes()
    assert a[3].tobytes() == filler_a and b[7].tobytes() == filler_b
    assert L.ws_map_clearance_download(t.handle, None, None, 0, 0, C.byref(n), None) == 0 and n.value == T
    # without the flag the pose records are gone, and asking for them is refused
    w.clearance(poses, body, SOFT)
    assert L.ws_map_clearance_poses_dev(t.handle, C.byref(m)) is None and m.value == 0
    assert L.ws_map_clearance_download(t.handle, None, b.ctypes.data_as(C.c_void_p), 0, 7, C.byref(n), C.byref(m)) == WS_ERR_INVALID
    ms = w.clearance_timing(1)
    w.clearance(poses, body, SOFT)
    ms = w.clearance_timing(0)
    assert len(ms) == 3 and ms[1] > 0.0


def test_refusals_leave_the_last_result_and_other_queries_alone(random_window):
    t, lo, hi, box = random_window
    shape = (3, 5, 64)
    rec, _ = DM.model_box(box, R)
    poses, body = scene(shape, lo, box.shape)
    w = t.avg_map()
    dist = w.distance(max_dist_vox=R)
    seeds = (np.argwhere((rec >> 30) == 1)[:1] + lo).astype(np.int32)
    cost = w.reach(seeds)
    before = w.clearance(poses, body, SOFT, per_pose=True)
    L, h = t._L, t.handle
    pp, bp, best = poses.ctypes.data_as(C.c_void_p), body.ctypes.data_as(C.c_void_p), C.c_int64(77)

    def call(p=pp, T=3, P=5, b=bp, K=64, soft=SOFT, flags=0):
        return L.ws_map_clearance(h, p, T, P, b, K, soft, flags, C.byref(best))
    far, wide = body.copy(), body.copy()
    far[5, 1], wide[7, 3] = (1 << 20) + 1, 65536
    cases = [(call(flags=4), WS_ERR_INVALID), (call(p=None), WS_ERR_INVALID), (call(b=None), WS_ERR_INVALID), (call(K=0), WS_ERR_RANGE), (call(K=65), WS_ERR_RANGE),
             (call(P=0), WS_ERR_RANGE), (call(P=65536), WS_ERR_RANGE), (call(T=(1 << 20) + 1, P=1), WS_ERR_RANGE), (call(T=1 << 20, P=3), WS_ERR_RANGE),
             (call(soft=-1), WS_ERR_RANGE), (call(soft=65536), WS_ERR_RANGE), (call(b=far.ctypes.data_as(C.c_void_p)), WS_ERR_RANGE),
             (call(b=wide.ctypes.data_as(C.c_void_p)), WS_ERR_RANGE), (call(soft=R * RES), WS_ERR_RANGE)]  # (R res < a radius + soft)
    assert [got for got, _ in cases] == [want for _, want in cases]
    assert call(T=0) == 0 and call(p=None, T=0) == 0 and best.value == 77  # nothing written, *best left alone
    n = C.c_size_t(0)
    got = np.zeros(3, dtype=before.records.dtype)
    got_pp = np.zeros((3, 5), dtype=before.poses.dtype)
    assert L.ws_map_clearance_download(h, got.ctypes.data_as(C.c_void_p), got_pp.ctypes.data_as(C.c_void_p), 3, 15, C.byref(n), None) == 0 and n.value == 3
    assert bytes_equal(got, before.records) and bytes_equal(got_pp, before.poses)
    # the call itself leaves the distance and the reach result as they were
    d2 = np.zeros(dist.size, dtype=np.uint32)
    assert L.ws_map_distance_download(h, d2.ctypes.data_as(C.c_void_p), d2.size, C.byref(n)) == 0 and np.array_equal(d2, dist.reshape(-1))
    c2 = np.zeros(cost.size, dtype=np.uint32)
    assert L.ws_map_reach_download(h, c2.ctypes.data_as(C.c_void_p), c2.size, C.byref(n)) == 0 and np.array_equal(c2, cost.reshape(-1))


def test_no_distance_result_is_refused():
    t, lo, hi = make_window(random_box(), **ROTATED)
    try:
        poses, body = scene((1, 1, 1), lo, (20, 19, 21))
        best = C.c_int64(77)
        call = lambda T: t._L.ws_map_clearance(t.handle, poses.ctypes.data_as(C.c_void_p), T, 1, body.ctypes.data_as(C.c_void_p), 1, 0, 0, C.byref(best))
        assert call(1) == WS_ERR_INVALID and best.value == 77
        assert call(0) == 0 and best.value == 77  # no trajectory: WS_OK in front of the look at the distance result
        n = C.c_size_t(5)
        assert t._L.ws_map_clearance_records_dev(t.handle, C.byref(n)) is None and n.value == 0
    finally:
        t.close()
