"""ws_store_surface — the surface cloud of the global map in device memory (the rules are stated in include/warpsense_hip.h) against
the numpy model that ws_map_surface is held to (surface_model.model_box), applied to a dense array assembled from host copies of
the chunks with every voxel of an absent chunk set to raw 0 (store_scenes.assemble).  Every comparison is on the raw bytes of
the records and of the marker floats."""
import ctypes as C

import numpy as np
import pytest

import query_model as QM
import store_scenes as SM
from store_surface_scenes import BAND, CS, CW, MW, RES, TAU, check_far_inputs, check_seam_inputs, far_chunks, model_store, same2, seam_chunks, seam_model
import surface_model as G

pytestmark = pytest.mark.gpu
WS_ERR_INVALID = -1


@pytest.fixture(scope="module")
def seam_store():
    """the seven chunks in a store whose segments hold two chunks each; no test changes its chunks"""
    store = SM.make_store(seam_chunks())
    yield store
    store.close()


def raw_surface(store, lo, hi, band, tau, res, flags=0):
    n = C.c_size_t(7)
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    rc = store._L.ws_store_surface(store.handle, p(a), p(b), band, tau, res, flags, C.byref(n))
    return rc, n.value


def total(store):
    n = C.c_size_t(0)
    assert store._L.ws_store_surface_download(store.handle, None, None, 0, C.byref(n)) == 0
    return n.value


# ------------------------------------------------------------------------------------------------ 1. the default box
def test_default_box_matches_the_model(seam_store):
    check_seam_inputs()
    assert sorted(seam_store.keys()) == sorted(seam_chunks()) and len(seam_store.keys()) == 7
    for band in (None, BAND):
        got, want = seam_store.surface(TAU, RES, band=band, marker=True), seam_model(band=band)
        print(band, len(want[0]))
        assert len(want[0]) > 1000 and same2(got, want), band
        assert QM.same(seam_store.surface(TAU, RES, band=band), want[0])
    assert len(seam_model(band=BAND)[0]) < len(seam_model()[0])
    assert same2(seam_store.surface(TAU, RES, band=0, marker=True), seam_model())  # band <= 0 means tau
    assert same2(seam_store.surface(TAU, RES, lo=(-CS,) * 3, hi=(CS - 1,) * 3, marker=True), seam_model())  # the bounding box
    # the marker follows the caller's tau and resolution, the records do not
    got = seam_store.surface(2 * TAU, 3 * RES, band=TAU, marker=True)
    assert same2(got, model_store(seam_chunks(), 2 * TAU, 3 * RES, band=TAU)) and QM.same(got[0], seam_model()[0])


# ------------------------------------------------------------------------------------------------ 2. boxes
CUT = ((-40, -29, -50), (37, 45, 20))  # cuts all seven chunks (and the absent one) with unaligned faces
FAR_OUTSIDE = ((-100_000, -70, -3_000_000), (90, 2_000_000, 130))  # holds every present chunk: the model is that of the bounding box
BOXES = {"one voxel": None, "cut": CUT, "in the absent chunk": ((1, 1, -60), (60, 60, -2)), "far outside": FAR_OUTSIDE}


def test_boxes(seam_store):
    rec = seam_model()[0]
    one = tuple(int(rec[n][len(rec) // 2]) for n in "xyz")  # a voxel that qualifies
    for name, box in BOXES.items():
        a, b = box if box else (one, one)
        m = (None, None) if name == "far outside" else (a, b)
        for band in (None, BAND):
            want = seam_model(*m, band)
            got = seam_store.surface(TAU, RES, lo=a, hi=b, band=band, marker=True)
            assert same2(got, want), (name, band)
        n = len(seam_model(*m)[0])
        assert {"one voxel": n == 1, "cut": n > 1000, "in the absent chunk": n == 0, "far outside": n > 1000}[name], (name, n)
    a, b = CUT
    keys = {tuple(int(c) for c in k) for k in np.stack([seam_model(a, b)[0][n] // CS for n in "xyz"], axis=1)}
    assert keys == set(seam_chunks())
    assert raw_surface(seam_store, (1000, 1000, 1000), (1100, 1100, 1100), 0, TAU, RES) == (0, 0)  # meets no present chunk
    assert raw_surface(seam_store, (-2 ** 31,) * 3, (2 ** 31 - 1,) * 3, 0, TAU, RES) == (0, len(rec))  # any box in int32 voxel space


# ------------------------------------------------------------------------------------------------ 3. the window's bytes
def test_same_bytes_as_the_window_surface(seam_store):
    import warpsense_amd as W
    lm = W.LocalMap(127, 127, 127, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    lo, hi = QM.window(lm.size, lm.pos)
    assert tuple(lo) == (-63,) * 3 and tuple(hi) == (63,) * 3 and (seam_store.default_raw >> 16) == 0  # fill_entry has weight 0
    seam_store.load_box(t, lo, hi)
    for a, b in [(lo, hi), CUT, ((-63, -5, -7), (63, 4, 9))]:
        for band in (None, BAND):
            got_window = t.avg_map().surface(lo=a, hi=b, band=band, marker=True)
            got_store = seam_store.surface(TAU, RES, lo=a, hi=b, band=band, marker=True)
            assert len(got_store[0]) > 1000 and same2(got_store, got_window) and same2(got_store, seam_model(tuple(a), tuple(b), band)), (a, b, band)
    t.close()


def test_far_apart_chunks_cost_three_chunks():
    chunks = far_chunks()
    lo, hi = check_far_inputs()
    store = SM.make_store(chunks, segment_chunks=0)
    try:
        parts = [G.model_box(chunks[key].reshape(CS, CS, CS), np.asarray(key, dtype=np.int64) * CS, TAU, RES) for key in sorted(chunks)]
        want = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])  # ascending cx: the chunks follow each other
        # The first call on this store allocates its scratch, its tables and its outputs.  What the header's cost rule allows: 32 KB of
        # masks and totals and 32 bytes of tables per listed chunk, and 44 bytes (record and marker) per record with an eighth of
        # slack, at most 3 x 64^3 records: 39 MB, in nine allocations of at most 2 MB of rounding each.  A pass over the box would
        # need 10^15 bytes.
        import torch
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        got = store.surface(TAU, RES, marker=True)
        taken = free_before - torch.cuda.mem_get_info()[0]
        print("device memory taken by the first call:", taken)
        assert taken <= 64 << 20, taken
        assert len(want[0]) > 3000 and same2(got, want)
        x, y, z = (got[0][n].astype(np.int64) for n in "xyz")
        step = np.stack([np.diff(x), np.diff(y), np.diff(z)], axis=1)
        first = np.argmax(step != 0, axis=1)
        assert np.all(step.any(axis=1)) and np.all(step[np.arange(len(step)), first] > 0)  # strictly ascending (x, y, z)
        assert int(np.diff(x).max()) > 1_000_000  # across the gaps
        assert same2(store.surface(TAU, RES, lo=lo, hi=hi, marker=True), want)
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 5. directory dynamics
def test_empty_dropped_put_and_old_results():
    import warpsense_amd as W
    from window_routes import _params
    empty = W.DeviceGlobalMap(TAU, 0)
    n = C.c_size_t(9)
    assert raw_surface(empty, None, None, 0, TAU, RES) == (0, 0) and raw_surface(empty, (-5, -5, -5), (5, 5, 5), 0, TAU, RES, flags=1) == (0, 0)
    assert empty._L.ws_store_surface_records_dev(empty.handle, C.byref(n)) is None and n.value == 0
    rec, mk = empty.surface(TAU, RES, marker=True)
    assert rec.shape == (0,) and rec.dtype == G.REC and mk.shape == (0, 7)
    only = (3, -2, 1)
    data = G.draw_entries(CW, seed=91).astype(np.uint32)
    empty.put_chunk(only, data)
    want = model_store({only: data}, TAU, RES)
    assert len(want[0]) > 1000 and same2(empty.surface(TAU, RES, marker=True), want)  # a call after put_chunk sees the chunk
    empty.drop_chunk(only)
    assert raw_surface(empty, None, None, 0, TAU, RES) == (0, 0) and total(empty) == 0  # ... and after drop_chunk its absence
    empty.close()

    chunks = dict(seam_chunks())
    store = SM.make_store(chunks, segment_chunks=2)
    try:
        gone = (-1, 0, 0)
        store.drop_chunk(gone)
        del chunks[gone]
        want = model_store(chunks, TAU, RES)
        assert 1000 < len(want[0]) < len(seam_model()[0]) and same2(store.surface(TAU, RES, marker=True), want)
        fresh = (1, 0, 0)
        chunks[fresh] = G.draw_entries(CW, seed=77).astype(np.uint32)
        store.put_chunk(fresh, chunks[fresh])
        want = model_store(chunks, TAU, RES)
        assert same2(store.surface(TAU, RES, marker=True), want)
        # the device result stays as it is while the store goes on: a save that creates and overwrites chunks, a load, a shift, and
        # the three other queries
        drec, dmk = store.surface(TAU, RES, marker=True, device=True)
        assert tuple(drec.shape) == (len(want[0]), 4) and tuple(dmk.shape) == (len(want[0]), 7)
        size = (21, 17, 13)
        lm = W.LocalMap(*size, TAU, 0, W.GlobalMap(TAU, 0))
        tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
        t = tm.tsdf()
        lo, hi = QM.window(lm.size, lm.pos)
        t.avg_map().insert_box(lo, hi, G.draw_entries(int(np.prod(size)), seed=5))
        store.save_box(t, lo, hi)
        store.load_box(t, lo, hi)
        tm.shift_map_device((4, -3, 2))
        store.mesh(RES)
        store.raycast(RES, (0, 0, 0), np.array([[1, 0, 0], [0, -1, 1]], dtype=np.int32), 2000)
        store.distance(lo=(-8, -8, -8), hi=(7, 7, 7), max_dist_vox=4)
        tm.wait_shift()
        assert np.array_equal(drec.cpu().numpy().view(np.uint8).reshape(-1), want[0].view(np.uint8).reshape(-1))
        assert np.array_equal(dmk.cpu().numpy().view(np.uint8).reshape(-1), want[1].view(np.uint8).reshape(-1))
        assert drec.data_ptr() == store._L.ws_store_surface_records_dev(store.handle, C.byref(n)) and n.value == len(want[0])
        assert dmk.data_ptr() == store._L.ws_store_surface_marker_dev(store.handle, C.byref(n)) and n.value == len(want[0])
        chunks = {k: store.chunk(k) for k in store.keys()}
        assert len(chunks) > 7 and same2(store.surface(TAU, RES, marker=True), model_store(chunks, TAU, RES))  # the save created chunks
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 6. repeatability, partial downloads
def test_repeatable_partial_downloads_and_device_tensors(seam_store):
    rec, mk = seam_store.surface(TAU, RES, marker=True)
    assert same2(seam_store.surface(TAU, RES, marker=True), (rec, mk)) and same2((rec, mk), seam_model())
    cap = len(rec) // 3
    assert cap > 10
    prec, pmk = np.zeros(cap + 1, dtype=G.REC), np.zeros((cap + 1, 7), dtype=G.F)
    n = C.c_size_t(0)
    L, h = seam_store._L, seam_store.handle
    assert L.ws_store_surface_download(h, prec.ctypes.data_as(C.c_void_p), pmk.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
    assert n.value == len(rec) and QM.same(prec[:cap], rec[:cap]) and QM.same(pmk[:cap], mk[:cap])
    assert not prec[cap:].view(np.uint8).any() and not pmk[cap:].any()  # a prefix, nothing beyond the capacity
    assert L.ws_store_surface_download(h, None, None, 0, C.byref(n)) == 0 and n.value == len(rec)
    only_mk = np.zeros((len(rec), 7), dtype=G.F)
    assert L.ws_store_surface_download(h, None, only_mk.ctypes.data_as(C.c_void_p), len(rec), C.byref(n)) == 0 and QM.same(only_mk, mk)
    drec, dmk = seam_store.surface(TAU, RES, marker=True, device=True)
    assert drec.is_cuda and dmk.is_cuda and tuple(drec.shape) == (len(rec), 4) and tuple(dmk.shape) == (len(rec), 7)
    assert drec.data_ptr() == L.ws_store_surface_records_dev(h, C.byref(n)) and n.value == len(rec)
    assert dmk.data_ptr() == L.ws_store_surface_marker_dev(h, C.byref(n)) and n.value == len(rec)
    assert np.array_equal(drec.cpu().numpy().view(np.uint8).reshape(-1), rec.view(np.uint8).reshape(-1))
    assert np.array_equal(dmk.cpu().numpy().view(np.uint8), mk.view(np.uint8))
    # without the flag there is no marker to hand out
    seam_store.surface(TAU, RES)
    assert L.ws_store_surface_marker_dev(h, C.byref(n)) is None and n.value == 0
    assert L.ws_store_surface_download(h, None, only_mk.ctypes.data_as(C.c_void_p), len(rec), C.byref(n)) == WS_ERR_INVALID
    seam_store.surface_timing(1)
    seam_store.surface(TAU, RES, marker=True)
    ms = seam_store.surface_timing(0)
    assert len(ms) == 3 and all(v > 0.0 for v in ms)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing_and_keep_the_last_result(seam_store):
    a, b = CUT
    drec, dmk = seam_store.surface(TAU, RES, lo=a, hi=b, marker=True, device=True)
    want = seam_model(a, b)
    before = total(seam_store)
    assert before == len(want[0]) > 1000
    seam_store.surface_timing(1)  # armed: a call that launches leaves times behind
    refused = {
        "lo alone": ((0, 0, 0), None, 0, TAU, RES, 0), "hi alone": (None, (0, 0, 0), 0, TAU, RES, 0), "hi < lo": ((0, 0, 0), (0, -1, 0), 0, TAU, RES, 0),
        "tau 0": (None, None, 0, 0, RES, 0), "tau < 0": (None, None, 5, -TAU, RES, 0), "resolution 0": (None, None, 0, TAU, 0, 0),
        "resolution < 0": (None, None, 0, TAU, -RES, 0), "unknown flag": (None, None, 0, TAU, RES, 2), "unknown flags": (None, None, 0, TAU, RES, 0x80000001),
    }
    for name, args in refused.items():
        assert raw_surface(seam_store, *args)[0] == WS_ERR_INVALID, name
        assert seam_store.surface_timing() == (0.0, 0.0, 0.0), name  # nothing was launched
        assert total(seam_store) == before, name
    seam_store.surface_timing(0)
    n = C.c_size_t(0)
    assert drec.data_ptr() == seam_store._L.ws_store_surface_records_dev(seam_store.handle, C.byref(n)) and n.value == before
    assert np.array_equal(drec.cpu().numpy().view(np.uint8).reshape(-1), want[0].view(np.uint8).reshape(-1))
    assert np.array_equal(dmk.cpu().numpy().view(np.uint8).reshape(-1), want[1].view(np.uint8).reshape(-1))


# ------------------------------------------------------------------------------------------------ 8. after real use
def test_after_real_use():
    import warpsense_amd as W
    from window_routes import _params
    size = (65, 65, 65)
    g = W.GlobalMap(TAU, 0)
    lm = W.LocalMap(*size, TAU, 0, g)
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
    with pytest.raises(W.WsError):
        W.TSDFMapping(_params(size), W.LocalMap(*size, TAU, 0)).global_surface_cloud()
    for k, pos in enumerate(SM.WALK):
        if k:
            tm.shift_map_device(pos)
        tm.update_tsdf(SM.walk_scan(k), pos_rm=pos, up_rm=(0, 0, 32768))
    rec, mk = tm.global_surface_cloud(marker=True)
    assert tm.tsdf().stats()["error_flags"] == 0
    lo, hi = lm.window()
    outside = [k for k in store.keys() if any(k[d] * CS + CS - 1 < lo[d] or k[d] * CS > hi[d] for d in range(3))]
    assert len(outside) >= 2, store.keys()
    tm.write_back()
    chunks = {k: v.reshape(-1) for k, v in g.chunks.items()}
    assert sorted(chunks) == sorted(store.keys())
    want = model_store(chunks, TAU, RES)
    left = int(np.count_nonzero(rec["x"] < lo[0]))  # what the window has left is in the cloud
    print(len(store.keys()), len(want[0]), left)
    assert len(want[0]) > 1000 and same2((rec, mk), want) and left > 100
    assert QM.same(tm.global_surface_cloud(band=TAU // 2), model_store(chunks, TAU, RES, band=TAU // 2)[0])
    store.close()
