"""ws_store_reach, ws_store_reach_lookup and ws_store_reach_paths: the reach over the distance records of the chunk store against
reach_model.py on the dense box of the chunks (store_distance_scenes.model), and against ws_map_reach on a window that holds the same
voxels.  Raw bytes throughout."""
import ctypes as C

import numpy as np
import pytest

import distance_model as D
import query_model as QM
import reach_model as RM
import store_distance_scenes as SDS
from store_distance_scenes import MW, RES, TAU, WINDOW_SEED, make_store, seam_chunks

pytestmark = pytest.mark.gpu
INF = RM.INF
CS = SDS.CS


def test_seam_with_an_absent_chunk_blocked_by_default_passable_when_unknown_is_free():
    chunks = seam_chunks()
    store = make_store(chunks)
    try:
        lo, hi = np.array([-12, -10, -14]), np.array([9, 11, 9])  # around the common corner of the eight chunks; (0, 0, -1) is absent
        rec, _ = SDS.model(chunks, lo, hi, 3, any_weight=True)
        absent = np.zeros(rec.shape, dtype=bool)
        absent[12:, 10:, :14] = True
        assert np.all((rec[absent] >> 30) == 0)  # what the store does not have is unknown
        seeds = (np.argwhere(RM.traversable(rec, 1))[[0, -1]] + lo)
        assert D.same(store.distance(lo=lo, hi=hi, max_dist_vox=3, any_weight=True), rec)
        for unknown_free in (False, True):
            want, kept, reached = RM.field(rec, lo, seeds, 1, unknown_free)
            assert kept == 2 and reached > 1000
            assert np.all(want[absent] == INF) != unknown_free and (np.count_nonzero(want[absent] != INF) > 500) == unknown_free
            got = store.reach(seeds, clear_d2=1, unknown_free=unknown_free)
            assert QM.same(got, want) and store.last_reach["reached"] == reached and store.last_reach["seeded"] == kept
            goals = (np.argwhere(absent)[::301] + lo).astype(np.int32)
            assert QM.same(store.reach_lookup(goals), RM.lookup(want, lo, goals))
            hw, rw = RM.paths(want, lo, goals, 48)
            hg, rg = store.reach_paths(goals, 48)
            assert QM.same(hg, hw) and QM.same(rg, rw) and ((0 in hw["status"]) if unknown_free else set(hw["status"].tolist()) == {1})
    finally:
        store.close()


def test_chunks_a_million_voxels_apart_in_one_box_do_not_reach_each_other():
    import warpsense_amd as W
    far = 15625  # x 64 = 1 000 000 voxels
    free = W.pack_entry(np.full(CS ** 3, TAU), np.ones(CS ** 3, np.int32)).astype(np.uint32)
    store = make_store({(0, 0, 0): free, (far, 0, 0): free})
    try:
        lo, hi = np.array([60, 0, 0]), np.array([far * CS + 3, 1, 1])
        rec = store.distance(lo=lo, hi=hi, max_dist_vox=1)
        cls = rec >> 30
        assert rec.shape == (far * CS - 56, 2, 2) and np.all(cls[:4] == 1) and np.all(cls[-4:] == 1) and np.all(cls[4:-4] == 0)
        for seed, near in (((61, 0, 1), True), ((far * CS + 2, 1, 0), False)):
            want, kept, reached = RM.field(rec, lo, [seed])
            assert (kept, reached) == (1, 16)
            got = store.reach([seed])
            assert QM.same(got, want) and store.last_reach["reached"] == 16
            assert np.all(got[:4] != INF) == near and np.all(got[-4:] != INF) == (not near)
    finally:
        store.close()


def test_the_empty_store():
    import warpsense_amd as W
    store = W.DeviceGlobalMap(TAU, 0)
    try:
        L, h = store._L, store.handle
        seed = np.array([[1, 2, 3]], dtype=np.int32)
        a, b, r = C.c_size_t(7), C.c_size_t(7), C.c_uint32(7)
        call = lambda flags=0: L.ws_store_reach(h, seed.ctypes.data_as(C.c_void_p), 1, 0, flags, 0, C.byref(a), C.byref(b), C.byref(r))
        assert call() == -1 and b"no distance result" in L.ws_last_error()
        assert store.distance(max_dist_vox=2).size == 0  # no box and no chunk: no records
        assert call() == 0 and (a.value, b.value, r.value) == (0, 0, 0)
        n = C.c_size_t(9)
        assert not L.ws_store_reach_dev(h, C.byref(n)) and n.value == 0
        assert list(store.reach_lookup(seed)) == [INF] and tuple(store.reach_paths(seed, 2)[0][0]) == (INF, 0, 0, 2)
        rec = store.distance(lo=(0, 0, 0), hi=(9, 8, 7), max_dist_vox=2)  # a box of nothing but absent voxels
        assert np.all(rec >> 30 == 0)
        assert np.all(store.reach(seed) == INF) and store.last_reach == dict(seeded=0, reached=0, rounds=0)
        want, _, _ = RM.field(rec, (0, 0, 0), seed, 0, True)
        assert QM.same(store.reach(seed, unknown_free=True), want) and store.last_reach["reached"] == 720
    finally:
        store.close()


def test_same_bytes_as_the_window():
    import warpsense_amd as W
    lm = W.LocalMap(65, 65, 65, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    try:
        lo, hi = QM.window(lm.size, lm.pos)
        t.avg_map().insert_box(lo, hi, D.draw_entries((65,) * 3, WINDOW_SEED))
        store.save_box(t, lo, hi)
        store.drop_chunk((0, -1, 0))
        store.load_box(t, lo, hi)  # the voxels of the dropped chunk come back as fill_entry
        chunks = {k: store.chunk(k) for k in store.keys()}
        avg = t.avg_map()
        a, b = np.array([-12, -20, -5]), np.array([14, 2, 12])
        for kw, clear_d2, unknown_free in ((dict(any_weight=True), 1, False), (dict(any_weight=True, columns=True), 0, True), (dict(), 2, True)):
            rec, _ = SDS.model(chunks, a, b, 3, **kw)
            seeds = np.argwhere(RM._volume(RM.traversable(rec, clear_d2, unknown_free)))[[0, -1]] + a
            want, kept, reached = RM.field(rec, a, seeds, clear_d2, unknown_free)
            assert kept == 2 and reached > 100
            assert D.same(avg.distance(lo=a, hi=b, max_dist_vox=3, **kw), rec) and D.same(store.distance(lo=a, hi=b, max_dist_vox=3, **kw), rec)
            got_w, got_s = avg.reach(seeds, clear_d2=clear_d2, unknown_free=unknown_free), store.reach(seeds, clear_d2=clear_d2, unknown_free=unknown_free)
            assert QM.same(got_w, got_s) and QM.same(got_s, want), kw
            assert (avg.last_reach["seeded"], avg.last_reach["reached"]) == (store.last_reach["seeded"], store.last_reach["reached"]) == (kept, reached)
            pts = np.random.default_rng(4).integers(-25, 20, size=(300, 4)).astype(np.int32)
            assert QM.same(avg.reach_lookup(pts), store.reach_lookup(pts)) and QM.same(store.reach_lookup(pts), RM.lookup(want, a, pts[:, :3]))
            goals = np.concatenate([pts[::10, :3], (np.argwhere(RM._volume(want) != INF)[::max(reached // 12, 1)] + a).astype(np.int32)])
            (hw, rw), (hs, rs) = avg.reach_paths(goals, 40), store.reach_paths(goals, 40)
            assert QM.same(hw, hs) and QM.same(rw, rs)
            hm, rm = RM.paths(want, a, goals, 40)
            assert QM.same(hs, hm) and QM.same(rs, rm) and np.any(hm["status"] == 0)
    finally:
        store.close()
        t.close()
