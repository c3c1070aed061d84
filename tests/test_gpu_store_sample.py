"""ws_store_sample — the point sample of the global map in device memory (the rules are stated in include/warpsense_hip.h) against
the numpy model of tests/sample_model.py applied to the `Chunks` field of store_raycast_scenes: host copies of the chunks, absent
chunks and voxels outside the box not valid.  Every comparison is on the raw bytes of the records, the gradient and the selection."""
import ctypes as C

import numpy as np
import pytest

import query_model as QM
import sample_model as H
import store_raycast_scenes as SH
import store_scenes as SM

pytestmark = pytest.mark.gpu
TAU, RES, MW = SM.TAU, SM.RES, SM.MW
CS = 64
BAND = TAU // 2
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
KW = dict(gradient=True, select=("unknown", "free"))
SEL = (H.UNKNOWN, H.FREE)


@pytest.fixture(scope="module")
def seam_store():
    store = SM.make_store(SM.seam_chunks())
    yield store
    store.close()


@pytest.fixture(scope="module")
def seam_points():
    return H.store_points(seed=3)


# ------------------------------------------------------------------------------------------------ 1. the seam chunks
def test_seam_chunks_match_the_model(seam_store, seam_points):
    import torch
    import warpsense_amd as W
    pts = seam_points
    p32 = pts.astype(np.int32)
    for any_weight in (False, True):
        want = H.model(SH.Chunks(SM.seam_chunks()), RES, pts, BAND, any_weight, select=SEL)
        got = seam_store.sample(RES, p32, BAND, any_weight=any_weight, **KW)
        print(any_weight, got[1].tolist())
        assert H.same(got, want), any_weight
        assert H.same(seam_store.sample(RES, torch.from_numpy(p32).cuda(), BAND, any_weight=any_weight, **KW), want)  # the _dev form; twice the same bytes
    # points in the absent chunk are UNKNOWN with raw 0; next to it the raw entry is given (test_sample_host counts both kinds)
    rec = want[0]
    in_absent = np.all(((pts // RES) >> 6) == np.asarray(SM.ABSENT), axis=1)
    assert in_absent.sum() >= 16 and not rec["raw"][in_absent].any() and np.all(rec["cls"][in_absent] == H.UNKNOWN)
    # resolution 1 (half = 0: every point is its own voxel's sample), which only the store admits
    pts1 = H.store_points(seed=4, res=1)
    want1 = H.model(SH.Chunks(SM.seam_chunks()), 1, pts1, BAND, True, select=SEL)
    assert want1[1].min() >= 16 and H.same(seam_store.sample(1, pts1.astype(np.int32), BAND, any_weight=True, **KW), want1)
    # a non-zero weight in fill_entry: absent stays invalid
    store = W.DeviceGlobalMap(TAU, 5, segment_chunks=2)
    for key in sorted(SM.seam_chunks()):
        store.put_chunk(key, SM.seam_chunks()[key])
    assert (store.default_raw >> 16) == 5
    assert H.same(store.sample(RES, p32, BAND, any_weight=True, **KW), want)
    store.close()


# ------------------------------------------------------------------------------------------------ 2. boxes that cut a chunk
def test_boxes(seam_store, seam_points):
    pts = seam_points
    for name, (lo, hi) in SH.BOXES.items():
        want = H.model(SH.Chunks(SM.seam_chunks(), lo, hi), RES, pts, BAND, True, select=SEL)
        got = seam_store.sample(RES, pts.astype(np.int32), BAND, lo=lo, hi=hi, any_weight=True, **KW)
        print(name, got[1].tolist())
        assert H.same(got, want), name
    lo, hi = SM.bounding_box(SM.seam_chunks())
    assert H.same(seam_store.sample(RES, pts.astype(np.int32), BAND, lo=lo, hi=hi, **KW), seam_store.sample(RES, pts.astype(np.int32), BAND, **KW))


# ------------------------------------------------------------------------------------------------ 3. far-apart chunks
FAR = [(2 ** 24 - 2, 0, -(2 ** 24 - 1)), (-(2 ** 24 - 1), 5, 7)]  # at res 1 their voxels reach +-2^30, the limit of a live point


def test_far_apart_chunks_with_keys_near_2_24():
    import mesh_model as M
    chunks = {key: M.draw_entries((CS,) * 3, seed=500 + i) for i, key in enumerate(FAR)}
    store = SM.make_store(chunks, segment_chunks=0)
    rng = np.random.default_rng(9)
    try:
        parts, wants = [], []
        for key in FAR:
            lo = np.asarray(key, dtype=np.int64) * CS
            p = lo + rng.integers(-2, CS + 2, (512, 3))
            p = p[np.all(np.abs(p) < 2 ** 30, axis=1)]
            parts.append(p)
            wants.append(H.model(SH.Chunks({key: chunks[key]}, base=key), 1, p, BAND, True, select=SEL))
        pts = np.concatenate(parts)
        got = store.sample(1, pts.astype(np.int32), BAND, any_weight=True, **KW)
        want = (np.concatenate([w[0] for w in wants]), sum(w[1] for w in wants), np.concatenate([w[2] for w in wants]), np.concatenate([w[3] for w in wants]))
        print(got[1].tolist())
        assert want[1].min() >= 16 and H.same(got, want)
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 4. the window's bytes
def test_same_bytes_as_the_window_sample(seam_store, seam_points):
    import warpsense_amd as W
    lm = W.LocalMap(129, 129, 129, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    lo, hi = QM.window(lm.size, lm.pos)
    assert tuple(lo) == (-64,) * 3 and tuple(hi) == (64,) * 3 and (seam_store.default_raw >> 16) == 0  # fill_entry has weight 0
    seam_store.load_box(t, lo, hi)
    p32 = seam_points.astype(np.int32)
    for any_weight in (False, True):
        got_window = t.avg_map().sample(p32, band_mm=BAND, any_weight=any_weight, **KW)
        got_store = seam_store.sample(RES, p32, BAND, lo=lo, hi=hi, any_weight=any_weight, **KW)
        # The same bytes in all three arrays -- but for `raw` where the nearest voxel lies in the absent chunk: there the store's rule gives
        # 0 (no such voxel) and the window holds what ws_store_load_box wrote, fill_entry.  Nothing else differs.
        g = seam_points // RES
        present = np.array([tuple(int(c) for c in k) in SM.seam_chunks() for k in g >> 6])
        g_absent = ~present & np.all((g >= lo) & (g <= hi), axis=1)  # (the absent one of the eight, and the plane of voxels 64 of the window)
        win_rec = got_window[0].copy()
        assert g_absent.sum() >= 16 and np.all(win_rec["raw"][g_absent] == seam_store.default_raw) and not got_store[0]["raw"][g_absent].any()
        win_rec["raw"][g_absent] = 0
        assert H.same(got_store, (win_rec, got_window[1], got_window[2], got_window[3])) and got_store[1].min() >= 16
        assert H.same(got_store, H.model(SH.Chunks(SM.seam_chunks(), lo, hi), RES, seam_points, BAND, any_weight, select=SEL))
    t.close()


# ------------------------------------------------------------------------------------------------ 5. refusals, and what outlives them
def test_refusals_and_results_that_survive_later_changes(seam_points):
    import warpsense_amd as W
    chunks = SM.seam_chunks()
    store = SM.make_store(chunks)
    L = store._L
    p32 = np.ascontiguousarray(seam_points[:900].astype(np.int32))
    rec, counts, grad, sel = store.sample(RES, p32, BAND, any_weight=True, **KW)
    vp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.c_void_p)
    cnt = np.full(4, 77, dtype=np.uint64)
    lo3, hi3 = np.array([-5, -5, -5], dtype=np.int32), np.array([5, 5, 5], dtype=np.int32)

    def call(lo=None, hi=None, n=10, band=BAND, res=RES, flags=0, p=p32):
        a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
        return L.ws_store_sample(store.handle, None if a is None else a.ctypes.data_as(C.c_void_p), None if b is None else b.ctypes.data_as(C.c_void_p),
                                 None if p is None else p.ctypes.data_as(C.c_void_p), n, band, res, flags, cnt.ctypes.data_as(C.c_void_p))

    def last_is_intact():
        a, b, c = np.zeros(900, dtype=H.SAMPLE), np.zeros((900, 3), dtype=np.int32), np.zeros((len(sel), 3), dtype=np.int32)
        n, ns = C.c_size_t(0), C.c_size_t(0)
        assert L.ws_store_sample_download(store.handle, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), 900, len(sel),
                                          C.byref(n), C.byref(ns)) == 0
        return (n.value, ns.value) == (900, len(sel)) and QM.same(a, rec) and QM.same(b, grad) and QM.same(c, sel)

    assert call(lo=lo3) == WS_ERR_INVALID and call(hi=hi3) == WS_ERR_INVALID and call(lo=hi3, hi=lo3) == WS_ERR_INVALID  # one NULL; hi < lo
    assert call(band=0) == WS_ERR_INVALID and call(band=-1) == WS_ERR_INVALID and call(res=0) == WS_ERR_INVALID and call(flags=64) == WS_ERR_INVALID
    assert call(p=None) == WS_ERR_INVALID and L.ws_store_sample(None, None, None, p32.ctypes.data_as(C.c_void_p), 10, BAND, RES, 0, None) == WS_ERR_INVALID
    assert call(res=1025) == WS_ERR_RANGE and call(n=2 ** 27 + 1) == WS_ERR_RANGE
    assert cnt.tolist() == [77] * 4 and last_is_intact()
    assert call(lo=lo3, hi=hi3) == 0 and int(cnt.sum()) == 10
    rec, counts, grad, sel = store.sample(RES, p32, BAND, any_weight=True, **KW)
    # later saves and drops leave the result as it is
    lm = W.LocalMap(33, 33, 33, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    store.save_box(t, *QM.window(lm.size, lm.pos))
    store.drop_chunk(sorted(chunks)[0])
    assert last_is_intact()
    # n == 0
    assert call(n=0, p=None) == 0 and cnt.tolist() == [0] * 4
    n = C.c_size_t(5)
    assert L.ws_store_sample_records_dev(store.handle, C.byref(n)) is None and n.value == 0
    # an empty store: every point UNKNOWN, raw 0
    empty = W.DeviceGlobalMap(TAU, 0)
    r = empty.sample(RES, p32, BAND, **KW)
    assert r[1].tolist() == [900, 0, 0, 0] and not r[0].tobytes().strip(b"\0") and not r[2].any() and np.array_equal(r[3], p32)
    empty.close(), t.close(), store.close()


# ------------------------------------------------------------------------------------------------ 6. after a real walk
def test_after_a_real_walk_points_in_the_part_the_window_has_left():
    """The walk of test_gpu_store_mesh (three scans, ws_shift_device between them).  The first scan's points lie where the window was:
    TSDFMapping.global_sample answers for all of them from the chunks, byte for byte the model on the written-back global map, while
    the window no longer knows those it has left."""
    import warpsense_amd as W
    from window_routes import _params
    size = (65, 65, 65)
    g = W.GlobalMap(TAU, 0)
    lm = W.LocalMap(*size, TAU, 0, g)
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
    with pytest.raises(W.WsError):
        W.TSDFMapping(_params(size), W.LocalMap(*size, TAU, 0)).global_sample(np.zeros((1, 3), dtype=np.int32))
    for k, pos in enumerate(SM.WALK):
        if k:
            tm.shift_map_device(pos)
        tm.update_tsdf(SM.walk_scan(k), pos_rm=pos, up_rm=(0, 0, 32768))
    pts = np.ascontiguousarray(SM.walk_scan(0)[::4], dtype=np.int32)
    lo, hi = lm.window()
    assert lo[0] > 0  # the window has moved on
    left = np.any((pts // RES < lo) | (pts // RES > hi), axis=1)
    got = tm.global_sample(pts, gradient=True, select=("surface",))  # band: tau
    got_w = tm.sample(pts, gradient=True, select=("surface",))
    assert tm.tsdf().stats()["error_flags"] == 0
    tm.write_back()
    chunks = {k: v.reshape(-1) for k, v in g.chunks.items()}
    assert sorted(chunks) == sorted(store.keys())
    want = H.model(SH.Chunks(chunks), RES, pts, TAU, select=(H.SURFACE,))
    surf_left = int(np.count_nonzero(left & (want[0]["cls"] == H.SURFACE)))
    print("points", len(pts), "outside the window", int(left.sum()), "of them SURFACE in the chunks", surf_left, "counts", want[1].tolist(), got_w[1].tolist())
    assert left.sum() >= 16 and surf_left >= 16 and H.same(got, want)
    # the window: UNKNOWN with raw 0 for what it has left, the store's bytes inside it wherever the cell lies inside it
    assert np.all(got_w[0]["cls"][left] == H.UNKNOWN) and not got_w[0]["raw"][left].any()
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    tm.tsdf().avg_map().to_host(host)
    import raycast_model as R
    assert H.same(got_w, H.model(R.Ring(host.data_, host.size_, host.pos_, host.offset_), RES, pts, TAU, select=(H.SURFACE,)))
    both = (got_w[0]["cls"] != H.UNKNOWN)
    assert both.sum() >= 16 and QM.same(got_w[0][both], got[0][both])
    store.close()
