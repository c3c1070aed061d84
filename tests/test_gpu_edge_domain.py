"""Frontier, reach and sample of the window and frontier, surface, distance and reach of the chunk store at the two ends of their
position domain, as include/warpsense_hip.h states it: a window whose last voxel is INT32_MAX or whose first is INT32_MIN, store
chunks at the keys 2^25 - 1 and -2^25 with a box of all int32, sample points on both sides of |p| = 2^30.  Every comparison is on
raw bytes against the numpy models (frontier_model, distance_model, reach_model, sample_model), and every far, top, bottom and mixed
result against the near result of the same entries moved by whole voxels.  The inputs are those of tests/edge_domain_scenes.py;
tests/test_edge_domain_host.py holds the models to the translation property and the fixtures to their edges without a GPU."""
import ctypes as C

import numpy as np
import pytest

import distance_model as DM
import edge_domain_scenes as E
import frontier_model as FM
import query_model as QM
import reach_model as RM
import reach_scenes as RS
import sample_model as H
import store_scenes as SM
import store_surface_scenes as SS
from query_model import same

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
FLAGS = ((0, False), (E.TAU, False), (0, True), (E.TAU, True))  # min_value, any_weight


def same3(got, want):
    return len(got) == len(want) == 3 and all(same(g, w) for g, w in zip(got, want))


def i3(v):
    return tuple(int(c) for c in v)


def open_window(box, name):
    return RS.make_window(box, pos=i3(E.base_pos(box.shape, name)), offset=E.OFFSET)


# ------------------------------------------------------------------------------------------------ 1. window frontier
_FRONTIER = {}


def device_frontier(size, name):
    """every result of the window at base `name`, once: {(box, min_value, any_weight): (records, labels, table)}, and what a prefix
    download and frontier_goals gave for the last of them"""
    if (size, name) not in _FRONTIER:
        import warpsense_amd as W
        t, lo, hi = open_window(E.frontier_box(size), name)
        try:
            avg, out = t.avg_map(), {}
            for box, a, b, _, _ in E.frontier_boxes(size, name):
                for min_value, any_weight in FLAGS:
                    kw = {} if a is None else dict(lo=i3(a), hi=i3(b))
                    plain = avg.frontier(min_value=min_value, any_weight=any_weight, **kw)
                    out[(box, min_value, any_weight)] = avg.frontier(min_value=min_value, any_weight=any_weight, clusters=True, **kw)
                    assert same(plain, out[(box, min_value, any_weight)][0])
            last = out[("inner", E.TAU, True)]
            n, k = C.c_size_t(0), C.c_size_t(0)
            rec, lab, tab = np.zeros(70, dtype=FM.RECORD), np.zeros(70, dtype=np.uint32), np.zeros(3, dtype=FM.CLUSTER)
            p = lambda v: v.ctypes.data_as(C.c_void_p)
            assert t._L.ws_map_frontier_download(t.handle, p(rec), p(lab), p(tab), 70, 3, C.byref(n), C.byref(k)) == 0
            assert (n.value, k.value) == (len(last[0]), len(last[2])) and same3((rec, lab, tab), tuple(v[:c] for v, c in zip(last, (70, 70, 3))))
            out["goals"] = W.frontier_goals(last[2], E.RES, 3)
        finally:
            t.close()
        _FRONTIER[(size, name)] = out
    return _FRONTIER[(size, name)]


@pytest.mark.parametrize("name", E.BASES)
@pytest.mark.parametrize("size", E.FRONTIER_SIZES, ids=str)
def test_window_frontier_matches_the_model_and_the_near_result_moved(size, name):
    got, near, s = device_frontier(size, name), device_frontier(size, "near"), E.shift(size, name)
    for box, _, _, a, b in E.frontier_boxes(size, name):
        for min_value, any_weight in FLAGS:
            want = E.frontier_model(size, name, a, b, min_value, any_weight)
            key = (box, min_value, any_weight)
            print(size, name, key, len(want[0]), len(want[2]))
            assert len(want[0]) >= 200 and len(want[2]) >= 5
            assert same3(got[key], want), key
            assert same3(got[key], E.moved_frontier(near[key], s)), key
    mine = FM.goals(got[("inner", E.TAU, True)][2], E.RES, 3)
    assert len(mine[0]) >= 2 and all(np.array_equal(m, g) and m.dtype == g.dtype for m, g in zip(mine, got["goals"]))
    if name in ("top", "bottom"):
        table = got[("null", 0, False)][2]
        assert np.any(np.all((1 if name == "top" else -1) * table["sum"] > 2 ** 33, axis=1))


# ------------------------------------------------------------------------------------------------ 2. window distance and reach
@pytest.mark.parametrize("name", E.EDGES)
@pytest.mark.parametrize("kind", ("random_odd", "random_even"))
def test_window_distance_at_the_ends_gives_the_near_bytes(kind, name):
    box = E.reach_box(kind)
    t, lo, hi = open_window(box, name)
    try:
        for kw in ({}, dict(unknown_occupied=True), dict(columns=True)):
            want, n_sites = DM.model_box(box, RS.R, **kw)
            w = t.avg_map()
            assert DM.same(w.distance(max_dist_vox=RS.R, **kw), want) and w.last_sites == n_sites, kw
            assert DM.same(w.distance(lo=i3(lo), hi=i3(hi), max_dist_vox=RS.R, **kw), want), kw
    finally:
        t.close()


_REACH = {}


def device_reach(kind, columns, name):
    """every reach result of the window at base `name`, once, each checked against the model where it is made"""
    key = (kind, columns, name)
    if key in _REACH:
        return _REACH[key]
    import torch
    full = E.reach_box(kind)
    box, lo, hi, rec, kept, dropped = E.reach_scene(kind, name, columns)
    t, wlo, whi = open_window(full, name)
    out = {}
    try:
        w = t.avg_map()
        fr = w.frontier(device=True).clone()  # the window's frontier records in device memory: (n, 4) int32
        if kind == "rooms":  # (no unknown voxel, no frontier: rows of four words near the window stand in)
            fr = torch.from_numpy((np.random.default_rng(6).integers(-3, 28, size=(300, 4)) + np.append(wlo, 0)).astype(np.int32)).cuda()
        fr_host = fr.cpu().numpy()
        assert len(fr_host) > 50
        kw = dict(lo=i3(lo), hi=i3(hi), columns=True) if columns else {}
        assert same(w.distance(max_dist_vox=RS.R, **kw), rec)
        seeds = np.concatenate([dropped[:3], kept, dropped[3:]])
        for clear_d2, unknown_free in ((0, False), (2, False), (0, True), (2, True)):
            want, n_kept, reached = RM.field(rec, lo, seeds, clear_d2, unknown_free)
            got = w.reach(seeds, clear_d2=clear_d2, unknown_free=unknown_free)
            assert same(got, want), (clear_d2, unknown_free)
            assert (w.last_reach["seeded"], w.last_reach["reached"]) == (n_kept, reached) and n_kept == len(kept)
            blo, ext, col = np.zeros(3, np.int32), np.zeros(3, np.uint32), C.c_int32(7)
            assert t._L.ws_map_reach_box(t.handle, blo.ctypes.data_as(C.c_void_p), ext.ctypes.data_as(C.c_void_p), C.byref(col)) == 0
            assert col.value == int(columns) and i3(blo)[:2] == i3(lo)[:2] and i3(ext)[:2] == rec.shape[:2] and (columns or (int(blo[2]), int(ext[2])) == (int(lo[2]), rec.shape[2]))
            # lookups: strides 3 and 4 from the host, the frontier's device records, the dropped seeds
            rng = np.random.default_rng(5)
            pts = np.clip(rng.integers(-3, 28, size=(400, 3)) + wlo, E.I32_MIN, E.I32_MAX)
            pts4 = np.concatenate([pts, rng.integers(0, 2 ** 31 - 1, size=(400, 1))], axis=1)
            ref = RM.lookup(want, lo, pts)
            assert np.any(ref != RM.INF) and np.any(ref == RM.INF)
            assert same(w.reach_lookup(pts.astype(np.int32)), ref) and same(w.reach_lookup(pts4.astype(np.int32)), ref)
            dev = w.reach_lookup(fr)
            assert dev.is_cuda and dev.dtype == torch.int32 and same(dev.cpu().numpy().view(np.uint32), RM.lookup(want, lo, fr_host[:, :3]))
            assert np.all(w.reach_lookup(dropped.astype(np.int32)) == RM.INF) and np.all(w.reach_lookup(kept.astype(np.int32)) == 0)
            # paths, one of them cut by cap_steps
            goals = E.reach_goals(want, lo, hi, RM.traversable(rec, clear_d2, unknown_free), columns)
            hw, rw = RM.paths(want, lo, goals, 12)
            hg, rg = w.reach_paths(goals.astype(np.int32), 12)
            assert same(hg, hw) and same(rg, rw), (clear_d2, unknown_free)
            out[(clear_d2, unknown_free)] = (got, hg, rg, set(hw["status"].tolist()), bool(np.any(hw["steps"] + 1 > hw["written"])))
    finally:
        t.close()
    _REACH[key] = out
    return out


REACH_CASES = [(kind, columns) for kind in E.REACH_SHAPES for columns in (False, True) if not (kind == "rooms" and columns)]


@pytest.mark.parametrize("name", E.BASES)
@pytest.mark.parametrize("kind,columns", REACH_CASES)
def test_window_reach_lookup_and_paths_match_the_model_and_the_near_result_moved(kind, columns, name):
    got, near = device_reach(kind, columns, name), device_reach(kind, columns, "near")
    s = E.shift(E.REACH_SHAPES[kind], name)
    statuses, cut = set(), False
    for key, (cost, hdr, steps, status, was_cut) in got.items():
        cost0, hdr0, steps0, _, _ = near[key]
        statuses |= status
        cut |= was_cut
        assert same(cost, cost0) and same(hdr, hdr0), key
        written = np.arange(steps.shape[1])[None, :] < hdr["written"][:, None]
        for k, n in enumerate("xy" if columns else "xyz"):
            assert np.array_equal(steps[n][written].astype(np.int64), steps0[n][written].astype(np.int64) + s[k]), (key, n)
        assert np.array_equal(steps["cost"], steps0["cost"])
    assert cut and ({0, 2} <= statuses) and (kind == "rooms" or statuses == {0, 1, 2})
    if name in E.EDGES:
        _, hdr, steps, _, _ = got[(0, False)]
        written = np.arange(steps.shape[1])[None, :] < hdr["written"][:, None]
        ends = dict(x=E.I32_MIN if name == "bottom" else E.I32_MAX, y=E.I32_MAX if name == "top" else E.I32_MIN)
        assert any(np.any(steps[n][written] == end) for n, end in ends.items())  # a path record at the end of int32
        if columns and name != "bottom":
            assert hdr["status"][0] == 0 and steps["z"][0, 0] == E.I32_MIN  # z is echoed from the goal


# ------------------------------------------------------------------------------------------------ 3. window sample
def run_sample(ring, pos, res, pts):
    """host form and _dev form of both weight rules on a window of `ring`'s entries at pos: [(records, counts, gradient, selection)]"""
    import torch
    import warpsense_amd as W
    t = W.TSDFCuda(W.DeviceMap(E.SAMPLE_SIZE, ring.offset, np.ascontiguousarray(ring.data.reshape(-1)), i3(pos)), H.TAU, E.MW, res)
    out = []
    try:
        p32 = pts.astype(np.int32)
        p_dev = torch.from_numpy(p32).cuda()
        for any_weight in (False, True):
            kw = dict(band_mm=E.BAND, any_weight=any_weight, gradient=True, select=("free", "surface"))
            host = t.avg_map().sample(p32, **kw)
            dev = t.avg_map().sample(p_dev, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(host, dev))
            out.append(host)
    finally:
        t.close()
    return out


@pytest.mark.parametrize("case", E.SAMPLE_CASES, ids=E.sample_id)
def test_window_sample_on_both_sides_of_the_plane(case):
    res = case[0]
    pos, ring, pts, live, dead = E.sample_case(case)
    near_ring, near_pts, s = E.sample_near(case)
    both = E.live_in_both(case)
    got, near = run_sample(ring, pos, res, pts), run_sample(near_ring, E.SAMPLE_NEAR, res, near_pts)
    for any_weight in (False, True):
        want = H.model(ring, res, pts, E.BAND, any_weight, select=(H.FREE, H.SURFACE))
        g = got[int(any_weight)]
        print(E.sample_id(case), any_weight, g[1].tolist())
        assert H.same(g, want), any_weight
        assert np.array_equal(g[1], want[1]) and want[1].min() >= 16
        assert not np.any(np.any(np.abs(g[3].astype(np.int64)) >= E.LIMIT, axis=1))  # no dead point among the selected
        assert np.all(g[0]["cls"][live] != H.UNKNOWN) and not g[0][dead].tobytes().strip(b"\0")
        n = near[int(any_weight)]
        assert g[0][both].tobytes() == n[0][both].tobytes() and np.array_equal(g[2][both], n[2][both])


# ------------------------------------------------------------------------------------------------ 4. the store
@pytest.mark.parametrize("where", ("top", "bottom"))
def test_store_frontier_and_surface_of_a_block_at_the_end_of_int32(where):
    chunks = E.block_chunks(where)
    store = SM.make_store(chunks)
    try:
        for a, b, lo, hi in E.block_boxes(where):
            kw = {} if a is None else dict(lo=i3(a), hi=i3(b))
            for min_value, any_weight in ((0, False), (E.TAU, True)):
                want = E.store_frontier_model(chunks, lo, hi, min_value, any_weight)
                assert len(want[0]) >= 200 and same3(store.frontier(min_value=min_value, any_weight=any_weight, clusters=True, **kw), want), (a is None, min_value)
            want = SS.model_store(chunks, E.TAU, E.RES, lo, hi)
            assert len(want[0]) > 100 and SS.same2(store.surface(E.TAU, E.RES, marker=True, **kw), want), a is None
        near = SM.make_store(E.block_chunks("near"))
        try:
            s = SM.bounding_box(chunks)[0] - SM.bounding_box(E.block_chunks("near"))[0]
            assert same3(store.frontier(clusters=True), E.moved_frontier(near.frontier(clusters=True), s))
        finally:
            near.close()
    finally:
        store.close()


def test_store_frontier_of_the_adversarial_pairs_in_the_box_of_all_int32():
    store = SM.make_store(E.pair_chunks())
    try:
        want = E.pair_model()
        got = store.frontier(lo=i3(E.ALL_INT32[0]), hi=i3(E.ALL_INT32[1]), clusters=True)
        assert same(got[0], want[0]), "records: a mask bit across the ends of int32?"
        assert same3(got, want), "clusters: plates at y = INT32_MAX and y = INT32_MIN joined?"
    finally:
        store.close()


@pytest.mark.parametrize("where", ("top", "bottom"))
def test_store_and_loaded_window_give_the_same_bytes_at_the_end_of_int32(where):
    """a 127^3 window whose last (first) voxel is the block's, loaded with ws_store_load_box: it holds the block but for one plane per
    axis, and the window rule (every voxel in int32) holds"""
    import warpsense_amd as W
    chunks = E.block_chunks(where)
    blo, bhi = SM.bounding_box(chunks)
    store = SM.make_store(chunks)
    t = None
    try:
        view = W.LocalMap(127, 127, 127, E.TAU, 0).device_map()
        view.pos_[:] = (bhi - 63) if where == "top" else (blo + 63)
        t = W.TSDFCuda(view, E.TAU, E.MW, E.RES)
        lo, hi = QM.window(view.size_, view.pos_)
        assert (np.all(hi == E.I32_MAX) if where == "top" else np.all(lo == E.I32_MIN)) and (store.default_raw >> 16) == 0
        store.load_box(t, i3(lo), i3(hi))
        for a, b in ((lo, hi), (lo + (3, 70, 9), hi - (60, 2, 11))):
            for min_value, any_weight in ((0, False), (E.TAU, True)):
                kw = dict(lo=i3(a), hi=i3(b), min_value=min_value, any_weight=any_weight, clusters=True)
                got_store = store.frontier(**kw)
                assert len(got_store[0]) > 100 and same3(got_store, t.avg_map().frontier(**kw)), (i3(a), min_value)
                assert same3(got_store, E.store_frontier_model(chunks, a, b, min_value, any_weight))
            assert SS.same2(store.surface(E.TAU, E.RES, lo=i3(a), hi=i3(b), marker=True), t.avg_map().surface(lo=i3(a), hi=i3(b), marker=True))
    finally:
        if t is not None:
            t.close()
        store.close()


def test_store_distance_reach_and_paths_at_the_top_give_the_near_bytes():
    top, near = SM.make_store(E.block_chunks("top")), SM.make_store(E.block_chunks("near"))
    try:
        (a, b), (a0, b0) = E.corner_box("top"), E.corner_box("near")
        s = a - a0
        for kw, clear_d2, unknown_free in ((dict(), 1, False), (dict(columns=True), 0, True), (dict(unknown_occupied=True), 2, False)):
            want, _ = DM.model_box(SM.assemble(E.block_chunks("near"), a0, b0), RS.R, **kw)
            assert DM.same(top.distance(lo=i3(a), hi=i3(b), max_dist_vox=RS.R, **kw), want) and DM.same(near.distance(lo=i3(a0), hi=i3(b0), max_dist_vox=RS.R, **kw), want)
            trav = np.argwhere(RM._volume(RM.traversable(want, clear_d2, unknown_free)))
            base0 = a0 * np.array([1, 1, 0 if "columns" in kw else 1])  # (a column's z does not count)
            seeds0 = np.concatenate([trav[[0, len(trav) // 2]] + base0, [a0 - 1]])
            seeds = seeds0 + s
            field, kept, reached = RM.field(want, a0, seeds0, clear_d2, unknown_free)
            assert kept == 2 and reached > 100
            got, got0 = top.reach(seeds, clear_d2=clear_d2, unknown_free=unknown_free), near.reach(seeds0, clear_d2=clear_d2, unknown_free=unknown_free)
            assert same(got, field) and same(got0, field) and top.last_reach == near.last_reach, kw
            vol = RM._volume(field)
            last = np.argwhere(vol != RM.INF)
            last = last[last[:, 0] == vol.shape[0] - 1]  # reached in the last plane of x
            assert len(last), kw
            goals0 = np.concatenate([last[[0, -1]] + base0, [a0 - 2], trav[-1:] + base0])
            hw, rw = RM.paths(field, a0, goals0, 16)
            (hg, rg), (h0, r0) = top.reach_paths((goals0 + s).astype(np.int32), 16), near.reach_paths(goals0.astype(np.int32), 16)
            assert same(h0, hw) and same(r0, rw) and same(hg, hw) and hw["status"][0] == 0 and hw["status"][2] == 2
            assert rg["x"][0, 0] == E.I32_MAX  # the goal in the last plane of x: a path record at INT32_MAX
            written = np.arange(16)[None, :] < hw["written"][:, None]
            for k, n in enumerate("xy" if "columns" in kw else "xyz"):
                assert np.array_equal(rg[n][written].astype(np.int64), rw[n][written].astype(np.int64) + s[k])
            assert np.array_equal(rg["cost"], rw["cost"])
            assert same(top.reach_lookup((goals0 + s).astype(np.int32)), RM.lookup(field, a0, goals0))
    finally:
        top.close()
        near.close()


# ------------------------------------------------------------------------------------------------ 5. refusals that stay refusals
@pytest.mark.parametrize("end", ("top", "bottom"))
def test_a_window_one_voxel_beyond_int32_is_refused_and_the_last_results_stay(end):
    """the window at the end of int32 answers; moved one voxel further on x (ws_map_set_params does not ask) frontier, distance and
    sample are WS_ERR_RANGE, nothing is launched and the last results stay readable; moved back, they answer again"""
    size = E.FRONTIER_SIZES[0]
    box = E.frontier_box(size)
    t, lo, hi = open_window(box, end)
    try:
        L, h, avg = t._L, t.handle, t.avg_map()
        p = lambda v: v.ctypes.data_as(C.c_void_p)
        pts = np.random.default_rng(2).integers(-2 ** 30 - 5, 2 ** 30 + 5, (300, 3)).astype(np.int32)  # (far from this window: the refusal is the point)
        fr = avg.frontier(clusters=True)
        dist = avg.distance(max_dist_vox=3)
        smp = avg.sample(pts, gradient=True)
        assert same3(fr, FM.frontier(box, lo)) and DM.same(dist, DM.model_box(box, 3)[0])
        pos = E.base_pos(size, end)
        beyond = pos.copy()
        beyond[0] += 1 if end == "top" else -1
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        size32, off32 = i32(size), i32(E.OFFSET)
        assert L.ws_map_set_params(h, 0, p(size32), p(i32(beyond)), p(off32)) == 0
        n, k, cnt = C.c_size_t(77), C.c_size_t(77), np.full(4, 77, dtype=np.uint64)
        assert L.ws_map_frontier(h, 0, None, None, 0, 2, C.byref(n), C.byref(k)) == WS_ERR_RANGE and (n.value, k.value) == (77, 77)
        assert L.ws_map_distance(h, 0, None, None, 3, 0, C.byref(n)) == WS_ERR_RANGE and n.value == 77
        assert L.ws_map_sample(h, 0, p(pts), len(pts), 0, 2, p(cnt)) == WS_ERR_RANGE and cnt.tolist() == [77] * 4
        assert b"int32" in L.ws_last_error()
        rec, lab, tab = np.zeros(len(fr[0]), FM.RECORD), np.zeros(len(fr[0]), np.uint32), np.zeros(len(fr[2]), FM.CLUSTER)
        assert L.ws_map_frontier_download(h, p(rec), p(lab), p(tab), len(rec), len(tab), C.byref(n), C.byref(k)) == 0 and same3((rec, lab, tab), fr)
        d = np.zeros(dist.size, np.uint32)
        assert L.ws_map_distance_download(h, p(d), d.size, C.byref(n)) == 0 and n.value == d.size and same(d.reshape(dist.shape), dist)
        r, g = np.zeros(len(pts), dtype=H.SAMPLE), np.zeros((len(pts), 3), dtype=np.int32)
        assert L.ws_map_sample_download(h, p(r), p(g), None, len(pts), 0, C.byref(n), None) == 0 and n.value == len(pts)
        assert same(r, smp[0]) and same(g, smp[2])
        assert L.ws_map_set_params(h, 0, p(size32), p(i32(pos)), p(off32)) == 0
        assert same3(avg.frontier(clusters=True), fr) and same(avg.sample(pts, gradient=True)[0], smp[0])
    finally:
        t.close()
