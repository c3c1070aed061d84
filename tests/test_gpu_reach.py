"""ws_map_reach, ws_map_reach_lookup and ws_map_reach_paths (the rules are stated in include/warpsense_hip.h) against reach_model.py
applied to the distance records of distance_model.py.  Every comparison is on the raw bytes of costs, lookups, headers and path
records.  Every scene is checked on the CPU before the device is asked."""
import ctypes as C

import numpy as np
import pytest

import distance_model as DM
import reach_model as RM
from frontier_scenes import tunnel_box
from query_model import same
from reach_scenes import R, make_window, random_box, serpentine_box, two_rooms

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
INF = RM.INF


def params():
    from warpsense_amd import _lib
    p = (C.c_int32 * 8)()
    assert _lib.load().ws_debug_reach_params(p) == 0
    return list(p)


def raw_reach(t, seeds, clear_d2=0, flags=0, max_rounds=0):
    seeds = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
    a, b, r = C.c_size_t(77), C.c_size_t(77), C.c_uint32(77)
    rc = t._L.ws_map_reach(t.handle, None if seeds is None else seeds.ctypes.data_as(C.c_void_p), 0 if seeds is None else len(seeds), clear_d2, flags, max_rounds,
                           C.byref(a), C.byref(b), C.byref(r))
    return rc, a.value, b.value, r.value


def costs(t):
    n = C.c_size_t(0)
    assert t._L.ws_map_reach_download(t.handle, None, 0, C.byref(n)) == 0
    out = np.zeros(n.value, dtype=np.uint32)
    assert t._L.ws_map_reach_download(t.handle, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) == 0
    return out


def check_share(rec, cost, clear_d2, unknown_free, lo_share=0.05, hi_share=0.95):
    """a condition on the MODEL: a scene in which nothing or everything is reached cannot pass"""
    trav = int(np.count_nonzero(RM.traversable(rec, clear_d2, unknown_free)))
    reached = int(np.count_nonzero(cost != INF))
    assert trav > 100 and lo_share * trav <= reached <= hi_share * trav, (trav, reached, clear_d2, unknown_free)


# ------------------------------------------------------------------------------------------------ 1. random box, partial tiles
ROTATED = dict(pos=(3, -2, 5), offset=(7, 4, 9))  # every axis of the ring wraps inside the window


@pytest.fixture(scope="module")
def random_window():
    box = random_box()
    t, lo, hi = make_window(box, **ROTATED)
    rec, _ = DM.model_box(box, R)
    strict = np.argwhere(RM.traversable(rec, 9, False) & (np.arange(box.shape[0])[:, None, None] < 6))
    seeds = np.concatenate([strict[[0, len(strict) // 2, -1]] + lo, [lo - 1], [lo + (7, 3, 3)]])  # three good ones, one outside, one on the baffle
    yield t, lo, hi, box, seeds
    t.close()


@pytest.mark.parametrize("unknown_free", [False, True])
@pytest.mark.parametrize("clear_d2", [0, 1, 2, 9])
def test_random_box_matches_the_model(random_window, clear_d2, unknown_free):
    t, lo, hi, box, seeds = random_window
    rec, _ = DM.model_box(box, R)
    want, kept, reached = RM.field(rec, lo, seeds, clear_d2, unknown_free)
    check_share(rec, want, clear_d2, unknown_free)
    assert kept == 3
    w = t.avg_map()
    assert same(w.distance(max_dist_vox=R), rec)
    got = w.reach(seeds, clear_d2=clear_d2, unknown_free=unknown_free)
    print(clear_d2, unknown_free, reached, w.last_reach)
    assert same(got, want)
    assert (w.last_reach["seeded"], w.last_reach["reached"]) == (kept, reached) and w.last_reach["rounds"] >= 1
    # several seeds: the cost is the minimum over them
    single = [RM.field(rec, lo, seeds[i:i + 1], clear_d2, unknown_free)[0] for i in range(3)]
    assert np.array_equal(want, np.minimum(np.minimum(single[0], single[1]), single[2]))


def test_box_inside_the_window_tiles_start_at_the_box(random_window):
    t, lo, hi, box, seeds = random_window
    blo, bhi = lo + (3, 1, 5), hi - (2, 3, 1)  # not at a multiple of the tile from anything
    sub = box[3:box.shape[0] - 2, 1:box.shape[1] - 3, 5:box.shape[2] - 1]
    rec, _ = DM.model_box(sub, R)
    inner = np.argwhere(RM.traversable(rec, 1) & (np.arange(sub.shape[0])[:, None, None] < 3))
    seeds = np.concatenate([inner[[0, -1]] + blo, seeds[:1]])  # (the window's first voxel lies outside this box)
    want, kept, _ = RM.field(rec, blo, seeds, 1)
    check_share(rec, want, 1, False)
    assert kept == 2
    w = t.avg_map()
    assert same(w.distance(lo=blo, hi=bhi, max_dist_vox=R), rec)
    assert same(w.reach(seeds, clear_d2=1), want) and w.last_reach["seeded"] == kept


def test_columns_eight_neighbourhood_and_z_ignored(random_window):
    t, lo, hi, box, seeds = random_window
    zlo, zhi = np.array([lo[0], lo[1], lo[2] + 2]), np.array([hi[0], hi[1], lo[2] + 6])  # a height band without the unknown top layer
    rec, _ = DM.model_box(box[:, :, 2:7], R, columns=True)
    assert rec.shape == box.shape[:2]
    far = seeds.copy()
    far[:, 2] += 1000  # z of a seed does not count
    for clear_d2, unknown_free in [(0, False), (2, True)]:
        want, kept, _ = RM.field(rec, zlo, far, clear_d2, unknown_free)
        check_share(rec, want, clear_d2, unknown_free, hi_share=0.96)
        w = t.avg_map()
        assert same(w.distance(lo=zlo, hi=zhi, max_dist_vox=R, columns=True), rec)
        assert same(w.reach(far, clear_d2=clear_d2, unknown_free=unknown_free), want) and w.last_reach["seeded"] == kept
        pts = np.array([zlo, zhi + (0, 0, 50), zlo - (1, 0, 0), zlo + (5, 5, -77)], dtype=np.int32)
        assert same(w.reach_lookup(pts), RM.lookup(want, zlo, pts))
        goals = np.array([zlo + (18, 2, 9), zlo + (3, 17, -4), zlo - (0, 1, 0)], dtype=np.int32)
        hw, rw = RM.paths(want, zlo, goals, 64)
        assert hw["status"][0] == 0 and hw["status"][2] == 2
        hg, rg = w.reach_paths(goals, 64)
        assert same(hg, hw) and same(rg, rw)


# ------------------------------------------------------------------------------------------------ 2. the block scheme at work
@pytest.fixture(scope="module")
def tunnel_window():
    box, length = tunnel_box()
    t, lo, hi = make_window(box, pos=(0, 0, 0), offset=(13, 29, 7))
    rec, _ = DM.model_box(box, 1)
    seed = (np.argwhere(RM.traversable(rec))[0] + lo)[None, :]
    want, _, reached = RM.field(rec, lo, seed)
    assert reached == length  # the whole tunnel, from one end
    assert same(t.avg_map().distance(max_dist_vox=1), rec)
    yield t, lo, rec, seed, want
    t.close()


def test_zigzag_tunnel_crosses_tiles_hundreds_of_times(tunnel_window):
    t, lo, rec, seed, want = tunnel_window
    w = t.avg_map()
    got = w.reach(seed)
    assert same(got, want)
    tiles_along_an_axis = -(-40 // params()[1])
    print(w.last_reach)
    assert w.last_reach["rounds"] > tiles_along_an_axis and w.last_reach["reached"] == int(np.count_nonzero(want != INF))
    assert same(w.reach(seed), want)  # two runs, the same bytes


def test_max_rounds_one_leaves_no_result_and_the_next_call_is_right(tunnel_window):
    t, lo, rec, seed, want = tunnel_window
    w = t.avg_map()
    assert same(w.reach(seed), want)
    rc = raw_reach(t, seed, max_rounds=1)[0]
    assert rc == WS_ERR_RANGE and b"not converged" in t._L.ws_last_error()
    n = C.c_size_t(5)
    assert not t._L.ws_map_reach_dev(t.handle, C.byref(n)) and n.value == 0 and len(costs(t)) == 0  # the previous result is gone too
    out = np.zeros(1, np.uint32)
    assert t._L.ws_map_reach_lookup(t.handle, seed.astype(np.int32).ctypes.data_as(C.c_void_p), 1, 3, out.ctypes.data_as(C.c_void_p)) == WS_ERR_INVALID
    assert same(w.reach(seed), want)


def test_serpentine_inside_one_tile_needs_more_sweeps_than_a_round_has():
    p = params()
    assert p[1:4] == [8, 8, 8], p  # the scene below is one tile of the volume
    box16 = np.zeros((16, 16, 16), dtype=np.uint32)
    box16[4:12, 4:12, 4:12] = serpentine_box(8)
    t, lo, hi = make_window(box16, pos=(2, 2, 2), offset=(5, 6, 7))
    try:
        blo, bhi = lo + 4, lo + 11
        rec, _ = DM.model_box(box16[4:12, 4:12, 4:12], 1)
        want, _, reached = RM.field(rec, blo, [blo])
        hops = int(want[want != INF].max()) // 17  # no path is shorter than cost / 17 steps
        assert reached > 100 and hops > p[0], (reached, hops, p)
        w = t.avg_map()
        assert same(w.distance(lo=blo, hi=bhi, max_dist_vox=1), rec)
        assert same(w.reach([blo]), want)
        print(w.last_reach, hops)
        assert w.last_reach["rounds"] >= -(-hops // p[0]) >= 2  # one tile: only its mark on itself can have brought the later rounds
    finally:
        t.close()


def test_two_rooms_and_the_gap_in_the_wall():
    box = two_rooms()
    t, lo, hi = make_window(box, pos=(5, 5, 5), offset=(1, 2, 3))
    try:
        rec, _ = DM.model_box(box, R)
        seed = [lo + (3, 6, 6)]
        w = t.avg_map()
        w.distance(max_dist_vox=R)
        for clear_d2, crosses in [(0, True), (1, True), (4, False)]:
            want, _, _ = RM.field(rec, lo, seed, clear_d2)
            assert (want[20, 6, 6] != INF) == crosses  # (on the model first)
            assert same(w.reach(seed, clear_d2=clear_d2), want)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 3. seeds, lookup, paths
def test_all_seeds_dropped_is_ok_and_empty(random_window):
    t, lo, hi, box, seeds = random_window
    w = t.avg_map()
    w.distance(max_dist_vox=R)
    got = w.reach(seeds[3:])
    assert np.all(got == INF) and got.shape == box.shape and w.last_reach == dict(seeded=0, reached=0, rounds=0)


def test_lookup_strides_host_and_device_frontier_records(random_window):
    import torch
    t, lo, hi, box, seeds = random_window
    rec, _ = DM.model_box(box, R)
    want, _, _ = RM.field(rec, lo, seeds, 1)
    w = t.avg_map()
    w.distance(max_dist_vox=R)
    assert same(w.reach(seeds, clear_d2=1), want)
    rng = np.random.default_rng(3)
    pts = rng.integers(-3, 25, size=(500, 3)).astype(np.int32) + lo.astype(np.int32)
    pts4 = np.concatenate([pts, rng.integers(0, 2 ** 31 - 1, size=(500, 1)).astype(np.int32)], axis=1)
    ref = RM.lookup(want, lo, pts)
    assert np.any(ref != INF) and np.any(ref == INF)
    assert same(w.reach_lookup(pts), ref) and same(w.reach_lookup(pts4), ref)
    fr = w.frontier(device=True)  # (n, 4) int32 records in device memory, fed straight in
    assert fr.shape[0] > 50
    got = w.reach_lookup(fr)
    assert got.is_cuda and got.dtype == torch.int32
    assert same(got.cpu().numpy().view(np.uint32), RM.lookup(want, lo, fr.cpu().numpy()[:, :3]))


def test_paths_match_the_model_tie_cap_unreachable_and_outside(random_window):
    t, lo, hi, box, seeds = random_window
    rec, _ = DM.model_box(box, R)
    want, _, _ = RM.field(rec, lo, seeds, 0)
    w = t.avg_map()
    w.distance(max_dist_vox=R)
    assert same(w.reach(seeds), want)
    reached = np.argwhere(want != INF)
    pocket = np.argwhere(RM.traversable(rec) & (want == INF))
    goals = np.concatenate([reached[::97] + lo, pocket[:2] + lo, [lo - 5], seeds[:1]]).astype(np.int32)
    hw, rw = RM.paths(want, lo, goals, 80)
    assert set(hw["status"].tolist()) == {0, 1, 2} and hw["steps"].max() < 80 and hw["steps"].max() > 10
    hg, rg = w.reach_paths(goals, 80)
    assert same(hg, hw) and same(rg, rw)
    ties = 0
    for h, r in zip(hg, rg):
        assert RM.legal_path(r, int(h["written"]), want)
        if h["status"] == 0:
            assert h["written"] == h["steps"] + 1 and r[0]["cost"] == h["cost"] and r[h["steps"]]["cost"] == 0
    # a tie is among the goals: a voxel with two neighbours that explain its cost
    vol = np.pad(want.astype(np.int64), 1, constant_values=INF)
    for g in (goals[hw["status"] == 0] - lo + 1):
        n = sum(1 for d in RM.OFFSETS if vol[tuple(g + d)] != INF and vol[tuple(g + d)] + RM.weight(d) == vol[tuple(g)])
        ties += n > 1
    assert ties > 0
    # a cap below the path: the prefix, the true steps; cap 0: headers alone
    hw, rw = RM.paths(want, lo, goals, 5)
    assert np.any(hw["steps"] + 1 > hw["written"])
    hg, rg = w.reach_paths(goals, 5)
    assert same(hg, hw) and same(rg, rw)
    hg, rg = w.reach_paths(goals, 0)
    assert same(hg, RM.paths(want, lo, goals, 0)[0]) and rg.shape == (len(goals), 0)


# ------------------------------------------------------------------------------------------------ 4. the other queries, refusals
def test_other_results_stay_and_the_reach_outlives_a_distance_call(random_window):
    t, lo, hi, box, seeds = random_window
    w = t.avg_map()
    w.distance(max_dist_vox=R)
    surf, (vert, face), fr = w.surface(), w.mesh(), w.frontier()
    origin = (lo + (3, 3, 3)) * 50
    dirs = np.array([[1, 0, 0], [0, 1, 0], [-1, -1, 0]], dtype=np.int32) * (1 << 20)
    ray = w.raycast(origin, dirs, 5000)[0]
    smp = w.sample(np.array([origin, origin + 120]), device=False)[0]
    want, _, _ = RM.field(DM.model_box(box, R)[0], lo, seeds, 1)
    assert same(w.reach(seeds, clear_d2=1), want)
    L, h = t._L, t.handle
    n = C.c_size_t(0)

    def fetch(call, dtype, count, *lead):
        out = np.zeros(count, dtype=dtype)
        assert call(h, out.ctypes.data_as(C.c_void_p), *lead) == 0
        return out
    assert same(fetch(L.ws_map_surface_download, surf.dtype, len(surf), None, len(surf), C.byref(n)), surf)
    assert same(fetch(L.ws_map_frontier_download, fr.dtype, len(fr), None, None, len(fr), 0, C.byref(n), None), fr)
    assert same(fetch(L.ws_map_raycast_download, ray.dtype, len(ray), None, len(ray), C.byref(n)), ray)
    assert same(fetch(L.ws_map_sample_download, smp.dtype, len(smp), None, None, len(smp), 0, C.byref(n), None), smp)
    v2, f2 = np.zeros_like(vert), np.zeros_like(face)
    a, b = C.c_size_t(0), C.c_size_t(0)
    assert L.ws_map_mesh_download(h, v2.ctypes.data_as(C.c_void_p), f2.ctypes.data_as(C.c_void_p), len(v2), len(f2), C.byref(a), C.byref(b)) == 0
    assert same(v2, vert) and same(f2, face)
    d = np.zeros(box.size, np.uint32)
    assert L.ws_map_distance_download(h, d.ctypes.data_as(C.c_void_p), d.size, C.byref(n)) == 0 and same(d.reshape(box.shape), DM.model_box(box, R)[0])
    # a later distance call over another box: lookups and paths still answer from the reach result's own box
    w.distance(lo=lo + 2, hi=lo + 6, max_dist_vox=2, columns=True)
    assert same(costs(t).reshape(box.shape), want)
    pts = (np.argwhere(want != INF)[::211] + lo).astype(np.int32)
    assert same(w.reach_lookup(pts), RM.lookup(want, lo, pts))
    assert same(w.reach_paths(pts[:4], 30)[1], RM.paths(want, lo, pts[:4], 30)[1])


def test_refusals_leave_the_last_result():
    import warpsense_amd as W
    box = two_rooms()
    t, lo, hi = make_window(box)
    try:
        seed = np.array([lo + 2], dtype=np.int32)
        assert raw_reach(t, seed)[0] == WS_ERR_INVALID and b"no distance result" in t._L.ws_last_error()
        w = t.avg_map()
        rec = w.distance(max_dist_vox=R)
        want = RM.field(rec, lo, seed)[0]
        assert same(w.reach(seed), want)
        for bad in [dict(flags=2), dict(flags=0x80000001), dict(clear_d2=-1), dict(clear_d2=65026)]:
            rc = raw_reach(t, seed, **bad)[0]
            assert rc == (WS_ERR_RANGE if "clear_d2" in bad else WS_ERR_INVALID), bad
            assert same(costs(t).reshape(box.shape), want), bad
        assert raw_reach(t, None)[0] == WS_ERR_INVALID
        assert t._L.ws_map_reach(t.handle, seed.ctypes.data_as(C.c_void_p), 0, 0, 0, 0, None, None, None) == WS_ERR_INVALID
        assert t._L.ws_map_reach(t.handle, seed.ctypes.data_as(C.c_void_p), (1 << 20) + 1, 0, 0, 0, None, None, None) == WS_ERR_INVALID
        assert t._L.ws_map_reach(None, seed.ctypes.data_as(C.c_void_p), 1, 0, 0, 0, None, None, None) == WS_ERR_INVALID
        out = np.zeros(1, np.uint32)
        assert t._L.ws_map_reach_lookup(t.handle, seed.ctypes.data_as(C.c_void_p), 1, 5, out.ctypes.data_as(C.c_void_p)) == WS_ERR_INVALID
        assert same(costs(t).reshape(box.shape), want)
        assert raw_reach(t, seed, clear_d2=65025)[:3] == (0, 0, 0)  # in range: nothing keeps that clearance here
        assert W.REACH_UNREACHABLE == INF and np.all(costs(t) == INF)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 5. every one of the 26 marks
def test_each_of_the_26_neighbour_marks_is_needed():
    """3 x 3 x 3 tiles.  Per direction d two free voxels in unknown: u on the rim of the centre tile and v = u + d in the tile beyond.  From
    the seed u, v is reached only if the centre tile marks exactly the tile in direction d for the next round."""
    p = params()
    assert p[1:4] == [8, 8, 8], p
    free = np.zeros((24, 24, 24), dtype=bool)
    pairs = []
    for d in RM.OFFSETS:
        u = np.array([8 if k < 0 else 15 if k > 0 else 11 for k in d])
        free[tuple(u)] = free[tuple(u + d)] = True
        pairs.append((u, u + np.array(d), RM.weight(d)))
    from reach_scenes import pack
    t, lo, hi = make_window(pack(free, ~free), pos=(1, -1, 2), offset=(3, 5, 7))
    try:
        w = t.avg_map()
        rec = w.distance(max_dist_vox=1)
        assert same(rec, DM.model_box(pack(free, ~free), 1)[0])
        for u, v, weight in pairs:
            want, kept, reached = RM.field(rec, lo, [u + lo])
            assert (kept, reached, int(want[tuple(v)])) == (1, 2, weight)
            assert same(w.reach([u + lo]), want), (u, v)
    finally:
        t.close()
