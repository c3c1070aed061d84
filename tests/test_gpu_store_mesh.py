"""ws_store_mesh — the mesh of the global map in device memory (the rules are stated in include/warpsense_hip.h) against the numpy
model that ws_map_mesh is held to (test_gpu_mesh.model_box), applied to a dense array assembled from host copies of the chunks with
every voxel of an absent chunk set to raw 0.  Every comparison is on the raw bytes of the vertex records and of the face indices."""
import ctypes as C

import numpy as np
import pytest

import mesh_model as M
import query_model as QM
from store_scenes import CS, CUT_BOXES, CW, MW, RES, TAU, WALK, _SEAM, bounding_box, check_seam_inputs, crossing_faces, far_chunks, make_store, model_store, raw_mesh, seam_chunks, seam_model, seam_world, split, walk_scan

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5


@pytest.fixture(scope="module")
def seam_store():
    """the seven chunks in a store whose segments hold two chunks each; no test changes its chunks"""
    store = make_store(seam_chunks())
    yield store
    store.close()


def totals(store):
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    assert store._L.ws_store_mesh_download(store.handle, None, None, 0, 0, C.byref(gv), C.byref(gf)) == 0
    return gv.value, gf.value


# ------------------------------------------------------------------------------------------------ 1. seams
def test_seams_match_the_model(seam_store):
    check_seam_inputs()
    assert sorted(seam_store.keys()) == sorted(seam_chunks()) and len(seam_store.keys()) == 7
    for any_weight in (False, True):
        got = seam_store.mesh(RES, any_weight=any_weight)
        want = seam_model(any_weight)
        print(any_weight, len(want[0]), len(want[1]))
        assert M.same(got, want), any_weight
    # faces across chunk borders exist: a face whose vertices lie on both sides of the plane x = 0, y = 0 or z = 0
    vert, face = seam_model(False)
    for name in ("x_mm", "y_mm", "z_mm"):
        q = vert[name][face.astype(np.int64)].astype(np.int64) - RES // 2
        assert np.count_nonzero((q.min(axis=1) < 0) & (q.max(axis=1) > 0)) > 10, name


def test_sphere_over_eight_chunks_is_closed():
    seam_world()
    store = make_store(split(_SEAM["sphere"]))
    try:
        got = store.mesh(RES)
        want = M.model_box(_SEAM["sphere"], (-CS,) * 3, RES)
        assert len(want[0]) > 100 and len(want[1]) > 100 and M.same(got, want)
        rep = M.mesh_report(*got)
        assert rep["closed"] and rep["chi"] == 2 and rep["unreferenced"] == 0, rep
    finally:
        store.close()


def test_same_bytes_as_the_window_mesh(seam_store):
    import warpsense_amd as W
    lm = W.LocalMap(129, 129, 129, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    lo, hi = QM.window(lm.size, lm.pos)
    assert tuple(lo) == (-64,) * 3 and tuple(hi) == (64,) * 3 and (seam_store.default_raw >> 16) == 0  # fill_entry has weight 0
    seam_store.load_box(t, lo, hi)
    for a, b in [((-64,) * 3, (63,) * 3)] + CUT_BOXES:
        want = seam_model(False, a, b)
        got_window, got_store = t.avg_map().mesh(lo=a, hi=b), seam_store.mesh(RES, lo=a, hi=b)
        assert len(want[0]) > 100 and len(want[1]) > 100, (a, b)
        assert M.same(got_store, got_window) and M.same(got_store, want), (a, b)
    t.close()


# ------------------------------------------------------------------------------------------------ 3. boxes
def test_boxes(seam_store):
    boxes = {
        "starts in a negative chunk": ((-50, -64, -64), (63, 63, 63)),
        "ends mid-chunk": ((-64, -64, -64), (30, 17, 41)),
        "exceeds the chunks on all sides": ((-100, -90, -70), (90, 100, 130)),
        "cut": CUT_BOXES[0],
    }
    for name, (a, b) in boxes.items():
        for any_weight in ((False, True) if name == "cut" else (False,)):
            want = seam_model(any_weight, a, b)
            got = seam_store.mesh(RES, lo=a, hi=b, any_weight=any_weight)
            assert len(want[0]) > 100 and len(want[1]) > 100 and M.same(got, want), (name, any_weight)
            assert int(got[1].max()) < len(got[0])  # faces of a box refer to vertices of that box
    assert M.same(seam_store.mesh(RES, lo=(-64,) * 3, hi=(63,) * 3), seam_model(False))  # the default box is the bounding box
    for name, (a, b) in {"one voxel thick": ((-64, -64, 0), (63, 63, 0)), "one voxel": ((5, 3, 2), (5, 3, 2)),
                         "in the absent chunk": ((1, 1, -60), (60, 60, -2)), "far away": ((1000, 1000, 1000), (1100, 1100, 1100))}.items():
        assert raw_mesh(seam_store, a, b, RES) == (0, 0, 0), name
        v, f = seam_store.mesh(RES, lo=a, hi=b)
        assert v.shape == (0,) and f.shape == (0, 3)
    seam_store.mesh(RES)
    before = totals(seam_store)
    assert before[0] > 100
    assert raw_mesh(seam_store, (0, 0, 0), (0, -1, 0), RES)[0] == WS_ERR_INVALID
    assert raw_mesh(seam_store, (0, 0, 0), None, RES)[0] == WS_ERR_INVALID and raw_mesh(seam_store, None, (0, 0, 0), RES)[0] == WS_ERR_INVALID
    assert raw_mesh(seam_store, None, None, 0)[0] == WS_ERR_INVALID and raw_mesh(seam_store, None, None, -50)[0] == WS_ERR_INVALID
    assert raw_mesh(seam_store, None, None, RES, flags=2)[0] == WS_ERR_INVALID
    assert totals(seam_store) == before  # a refused call leaves the last result
    import warpsense_amd as W
    empty = W.DeviceGlobalMap(TAU, 0)
    assert raw_mesh(empty, None, None, RES) == (0, 0, 0) and raw_mesh(empty, (-5, -5, -5), (5, 5, 5), RES) == (0, 0, 0)
    n = C.c_size_t(9)
    assert empty._L.ws_store_mesh_vertices_dev(empty.handle, C.byref(n)) is None and n.value == 0
    empty.close()


def test_far_apart_chunks_cost_three_chunks():
    chunks = far_chunks()
    lo, hi = bounding_box(chunks)
    assert float(np.prod((hi - lo + 1).astype(np.float64))) > 1e12  # no dense pass over the box can run
    assert all((abs(int(c)) + 1) * RES < 2 ** 31 for c in list(lo) + list(hi))
    store = make_store(chunks, segment_chunks=0)
    try:
        for any_weight in (False, True):
            verts, faces, base = [], [], 0
            for key in sorted(chunks):  # ascending cx: the chunks' cells follow each other in the output order
                v, f = M.model_box(chunks[key].reshape(CS, CS, CS), np.asarray(key, dtype=np.int64) * CS, RES, any_weight)
                assert len(v) > 100 and len(f) > 100, key
                verts.append(v), faces.append(f + np.uint32(base))
                base += len(v)
            got = store.mesh(RES, any_weight=any_weight)
            assert M.same(got, (np.concatenate(verts), np.concatenate(faces))), any_weight
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 5. directory dynamics
def test_drop_put_and_old_results():
    import warpsense_amd as W
    chunks = dict(seam_chunks())
    store = make_store(chunks, segment_chunks=2)
    try:
        assert store.capacity() >= 6 and len(chunks) == 7  # three segments and more
        assert M.same(store.mesh(RES), seam_model(False))
        gone = (-1, 0, 0)
        store.drop_chunk(gone)
        del chunks[gone]
        want = model_store(chunks, RES)
        got = store.mesh(RES)
        assert len(want[1]) > 100 and len(want[1]) < len(seam_model(False)[1]) and M.same(got, want)
        # nothing is left of the cells that need the dropped chunk (cell x <= -2, y >= 0, z >= 0 among them); they were there before
        octant = lambda v: np.count_nonzero((v["x_mm"] < -RES) & (v["y_mm"] > RES) & (v["z_mm"] > RES))
        assert octant(seam_model(False)[0]) > 100 and octant(got[0]) == 0
        slots = store.capacity()
        fresh = (1, 0, 0)
        chunks[fresh] = M.draw_entries((CS,) * 3, seed=77)
        store.put_chunk(fresh, chunks[fresh])
        assert store.capacity() == slots and store.count() == 7  # the slot of the dropped chunk
        want = model_store(chunks, RES)
        assert len(want[1]) > 100 and M.same(store.mesh(RES), want)
        # the result of a call stays readable while the store goes on: a save_box that creates and overwrites chunks
        dv, df = store.mesh(RES, device=True)
        assert tuple(dv.shape) == (len(want[0]), 4) and tuple(df.shape) == (len(want[1]), 3)
        lm = W.LocalMap(21, 17, 13, TAU, 0)
        t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
        lo, hi = QM.window(lm.size, lm.pos)
        t.avg_map().insert_box(lo, hi, M.draw_entries(tuple(int(s) for s in lm.size), seed=5))
        store.save_box(t, lo, hi)
        assert np.array_equal(dv.cpu().numpy().view(np.uint8).reshape(-1), want[0].view(np.uint8).reshape(-1))
        assert np.array_equal(df.cpu().numpy().view(np.uint8).reshape(-1), want[1].view(np.uint8).reshape(-1))
        n = C.c_size_t(0)
        assert dv.data_ptr() == store._L.ws_store_mesh_vertices_dev(store.handle, C.byref(n)) and n.value == len(want[0])
        chunks = {k: store.chunk(k) for k in store.keys()}
        assert len(chunks) == 9 and M.same(store.mesh(RES), model_store(chunks, RES))  # the save created (-1, 0, 0) and (0, 0, -1)
        t.close()
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 6. repeatability, partial downloads
def test_repeatable_and_partial_downloads(seam_store):
    vert, face = seam_store.mesh(RES)
    assert M.same(seam_store.mesh(RES), (vert, face)) and M.same((vert, face), seam_model(False))
    cv, cf = len(vert) // 3, len(face) // 2
    assert cv > 10 and cf > 10
    pv, pf = np.zeros(cv + 1, dtype=M.VERT), np.zeros((cf + 1, 3), dtype=np.uint32)
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    L, h = seam_store._L, seam_store.handle
    assert L.ws_store_mesh_download(h, pv.ctypes.data_as(C.c_void_p), pf.ctypes.data_as(C.c_void_p), cv, cf, C.byref(gv), C.byref(gf)) == 0
    assert (gv.value, gf.value) == (len(vert), len(face)) and QM.same(pv[:cv], vert[:cv]) and QM.same(pf[:cf], face[:cf])
    assert not pv[cv:].view(np.uint8).any() and not pf[cf:].any()  # a prefix, nothing beyond the capacity
    assert L.ws_store_mesh_download(h, None, None, 0, 0, C.byref(gv), C.byref(gf)) == 0 and (gv.value, gf.value) == (len(vert), len(face))
    only_f = np.zeros((len(face), 3), dtype=np.uint32)
    assert L.ws_store_mesh_download(h, None, only_f.ctypes.data_as(C.c_void_p), 0, len(face), C.byref(gv), C.byref(gf)) == 0 and QM.same(only_f, face)
    ms = seam_store.mesh_timing(1)
    seam_store.mesh(RES)
    ms = seam_store.mesh_timing(0)
    assert len(ms) == 3 and all(v > 0.0 for v in ms)


# ------------------------------------------------------------------------------------------------ 7. WS_ERR_RANGE
def test_range_errors_launch_nothing():
    from window_routes import same_store, store_state
    far = 671090  # 64 * 671090 * 50 mm is beyond int32
    assert (CS * far + 1) * RES > 2 ** 31 - 1 and CS * far + CS - 1 < 2 ** 31
    chunks = {(0, 0, 0): far_chunks()[(0, 0, 0)]}
    store = make_store(chunks)
    try:
        want = model_store(chunks, RES)
        assert M.same(store.mesh(RES), want) and len(want[0]) > 100
        store.put_chunk((far, 0, 0), np.zeros(CW, dtype=np.uint32))
        before, before_totals = store_state(store), totals(store)
        assert raw_mesh(store, None, None, RES)[0] == WS_ERR_RANGE  # decided on the bounding box
        assert raw_mesh(store, (0, 0, 0), (CS * far, 10, 10), RES)[0] == WS_ERR_RANGE
        assert raw_mesh(store, (-CS * far, 0, 0), (10, 10, 10), RES)[0] == WS_ERR_RANGE
        assert same_store(store_state(store), before) and totals(store) == before_totals == (len(want[0]), len(want[1]))
        assert M.same(store.mesh(RES, lo=(0, 0, 0), hi=(63, 63, 63)), want)  # an explicit box that fits is served
        # at 1 mm the bounding box fits int32: 43 million voxels long, two chunks of work (the far chunk has no valid voxel)
        assert M.same(store.mesh(1), M.model_box(chunks[(0, 0, 0)].reshape(CS, CS, CS), (0, 0, 0), 1))
    finally:
        store.close()


def test_after_real_use():
    import warpsense_amd as W
    from window_routes import _params
    size = (65, 65, 65)
    g = W.GlobalMap(TAU, 0)
    lm = W.LocalMap(*size, TAU, 0, g)
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
    with pytest.raises(W.WsError):
        W.TSDFMapping(_params(size), W.LocalMap(*size, TAU, 0)).global_mesh()
    for k, pos in enumerate(WALK):
        if k:
            tm.shift_map_device(pos)
        tm.update_tsdf(walk_scan(k), pos_rm=pos, up_rm=(0, 0, 32768))
    vert, face = tm.global_mesh()
    assert tm.tsdf().stats()["error_flags"] == 0
    lo, hi = lm.window()
    outside = [k for k in store.keys() if any(k[d] * CS + CS - 1 < lo[d] or k[d] * CS > hi[d] for d in range(3))]
    assert len(outside) >= 2, store.keys()
    tm.write_back()
    chunks = {k: v.reshape(-1) for k, v in g.chunks.items()}
    assert sorted(chunks) == sorted(store.keys())
    want = model_store(chunks, RES)
    print(len(store.keys()), len(want[0]), len(want[1]), crossing_faces(vert, face, RES))
    assert len(want[1]) > 100 and M.same((vert, face), want)
    assert crossing_faces(vert, face, RES) >= 1
    assert M.same(tm.global_mesh(any_weight=True), model_store(chunks, RES, any_weight=True))
    store.close()
