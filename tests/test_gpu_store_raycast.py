"""ws_store_raycast — the ray cast of the global map in device memory (the rules are stated in include/warpsense_hip.h) against the
numpy model that ws_map_raycast is held to (raycast_model.model), applied to the `Chunks` field of store_raycast_scenes: host
copies of the chunks, absent chunks and voxels outside the box not valid.  Every comparison is on the raw bytes of the records and
of the gradient, for all rays.  The ray sets are those of test_store_raycast_host, which checks without a GPU that each has hits and
no-hits in the model."""
import ctypes as C

import numpy as np
import pytest

import mesh_model as M
import query_model as QM
import raycast_model as R
from store_raycast_scenes import raw_cast
import store_raycast_scenes as H
import store_scenes as SM

pytestmark = pytest.mark.gpu
TAU, RES, MW = SM.TAU, SM.RES, SM.MW
CS = 64
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5


def cast(store, case, gradient=True):
    return store.raycast(RES, case["origin"], np.asarray(case["dirs"]).astype(np.int32), case["range"], lo=case.get("lo"), hi=case.get("hi"),
                         any_weight=case.get("any_weight", False), gradient=gradient, targets=case.get("targets", False))


def check(store, case):
    want = H.want(case)
    got = cast(store, case)
    assert R.same(got, want), (case["name"], H.hits_of(got[0]), H.hits_of(want[0]))
    assert store.last_hits == H.hits_of(want[0]), case["name"]


@pytest.fixture(scope="module")
def seam_store():
    store = SM.make_store(SM.seam_chunks())
    yield store
    store.close()


def result(store, n_cap=None):
    """(rays, records, device pointer) of the last result, through the download entry"""
    L, n = store._L, C.c_size_t(0)
    ptr = L.ws_store_raycast_records_dev(store.handle, C.byref(n))
    rec = np.zeros(n.value if n_cap is None else n_cap, dtype=R.RAY)
    got = C.c_size_t(0)
    assert L.ws_store_raycast_download(store.handle, rec.ctypes.data_as(C.c_void_p), None, len(rec), C.byref(got)) == 0 and got.value == n.value
    return n.value, rec, ptr


# ------------------------------------------------------------------------------------------------ 1. the seam chunks
def test_seam_chunks_match_the_model(seam_store):
    import torch
    for case in H.seam_cases():
        check(seam_store, case)
    # the device form, and without the gradient
    case = H.seam_cases()[1]
    d_dev = torch.from_numpy(np.asarray(case["dirs"]).astype(np.int32)).cuda()
    got = seam_store.raycast(RES, case["origin"], d_dev, case["range"], gradient=True)
    assert R.same(got, H.want(case))
    rec, grad = cast(seam_store, case, gradient=False)
    assert grad is None and QM.same(rec, H.want(case)[0])
    # hits whose cell straddles a chunk border exist on every axis, and the sphere is where it should be
    rec = H.want(H.seam_cases()[0])[0]
    b = (np.stack([rec["x_mm"], rec["y_mm"], rec["z_mm"]], axis=1)[rec["range_mm"] >= 0] - RES // 2) // RES
    assert all(np.count_nonzero((b[:, k] & 63) == 63) > 0 for k in range(3))


# ------------------------------------------------------------------------------------------------ 2. nothing in the way
def test_nothing_in_the_way():
    """Eight rows of three chunks with the middle one absent (test_store_raycast_host.gap_chunks), the origin stepped in 1 mm
    increments over two march steps.  test_store_raycast_host shows on the model that p_{k-1} of the +x, +y, +z axis hits is the
    FIRST sample behind the gap at every phase, so a jump that lands one sample late loses those hits (shown once on a build whose
    resume() returned one more: at the first origin 14 of the model's 24 hits were left and the test failed).  A jump that lands
    one sample EARLY lands on a sample whose base voxel is still in the absent chunk: its cell is invalid, the march walks on from
    there, and the records are the same by construction -- no test on records can tell."""
    store = SM.make_store(H.gap_chunks(), segment_chunks=4)
    try:
        n_hits = 0
        for case in H.gap_cases():
            check(store, case)
            n_hits += store.last_hits
        assert n_hits > 20 * len(H.gap_cases())
        check(store, dict(H.gap_cases()[3], name="gap any", any_weight=True))
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 3. the window's bytes
def test_same_bytes_as_the_window_raycast(seam_store):
    import warpsense_amd as W
    lm = W.LocalMap(129, 129, 129, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    lo, hi = QM.window(lm.size, lm.pos)
    assert tuple(lo) == (-64,) * 3 and tuple(hi) == (64,) * 3 and (seam_store.default_raw >> 16) == 0  # fill_entry has weight 0
    seam_store.load_box(t, lo, hi)
    cases = H.seam_cases()
    for case in (cases[0], cases[1], cases[2], cases[7]):  # three origins: inside, outside the sphere, outside every chunk; the grazing rays
        d = np.asarray(case["dirs"]).astype(np.int32)
        kw = dict(any_weight=case.get("any_weight", False), gradient=True)
        got_window = t.avg_map().raycast(case["origin"], d, case["range"], **kw)
        got_store = seam_store.raycast(RES, case["origin"], d, case["range"], lo=lo, hi=hi, **kw)
        assert R.same(got_store, got_window) and R.same(got_store, H.want(case)), case["name"]
        assert H.hits_of(got_store[0]) > 2 and np.any(got_store[1] != 0)
    t.close()


# ------------------------------------------------------------------------------------------------ 4. boxes
def test_boxes(seam_store):
    for case in H.box_cases():
        check(seam_store, case)
    base = H.seam_cases()[0]
    inside_box = dict(base, name="seam in pos 768", dirs=base["dirs"][:768])
    assert R.same(cast(seam_store, inside_box), H.want(H.box_cases()[-1]))  # the default box against the explicit bounding box


# ------------------------------------------------------------------------------------------------ 5. far-apart chunks
def test_far_apart_chunks_and_a_long_gap():
    store = SM.make_store(SM.far_chunks(), segment_chunks=0)
    try:
        lo, hi = SM.bounding_box(SM.far_chunks())
        assert float(np.prod((hi - lo + 1).astype(np.float64))) > 1e12  # nothing that follows the box's volume can run
        for case in H.far_cases():
            check(store, case)
            check(store, dict(case, name=case["name"] + " box", lo=lo, hi=hi))
        places = C.c_size_t(0)
        assert store._L.ws_debug_store_raycast_table(None, 3, None, 0, C.byref(places)) == 0 and places.value == 8  # sized by the three chunks
    finally:
        store.close()
    store = SM.make_store(H.range_chunks())
    try:
        case = H.range_case()
        check(store, case)
        rec = H.want(case)[0]
        assert np.all(rec["range_mm"][:3] > 12 * CS * RES) and np.all(rec["x_mm"][:3] >= 13 * CS * RES)  # the rays hit the far chunk
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing_and_leave_the_last_result(seam_store):
    import warpsense_amd as W
    case = H.seam_cases()[3]
    want = H.want(case)
    check(seam_store, case)
    n0, rec0, ptr0 = result(seam_store)
    assert n0 == len(want[0]) and QM.same(rec0, want[0])
    d = np.ascontiguousarray(np.asarray(case["dirs"]).astype(np.int32))
    o = case["origin"]
    call = lambda **kw: raw_cast(seam_store, kw.pop("origin", o), d, kw.pop("n", len(d)), kw.pop("rng", 3000), **kw)[0]
    assert call(rng=0) == WS_ERR_INVALID and call(rng=-5) == WS_ERR_INVALID and call(flags=8) == WS_ERR_INVALID
    assert call(res=0) == WS_ERR_INVALID and call(res=-50) == WS_ERR_INVALID
    assert call(lo=(0, 0, 0)) == WS_ERR_INVALID and call(hi=(0, 0, 0)) == WS_ERR_INVALID and call(lo=(0, 0, 0), hi=(0, -1, 0)) == WS_ERR_INVALID
    assert call(res=1025) == WS_ERR_RANGE and call(n=2 ** 27 + 1) == WS_ERR_RANGE
    assert call(origin=(0, 2 ** 31 - 1 - 3000 - 2 * RES + 1, 0)) == WS_ERR_RANGE
    assert call(origin=(0, 0, -(2 ** 31 - 1 - 3000 - 2 * RES + 1))) == WS_ERR_RANGE
    n1, rec1, ptr1 = result(seam_store)
    assert (n1, ptr1) == (n0, ptr0) and QM.same(rec1, rec0)  # nothing was launched, the last result stays
    assert call(origin=(0, -(2 ** 31 - 1 - 3000 - 2 * RES), 0)) == 0  # the edge of the range is served ...
    assert call(res=1024) == 0
    n = C.c_size_t(9)
    # n == 0: WS_OK, nothing written
    assert raw_cast(seam_store, o, d, 0, 3000) == (0, 0)
    assert seam_store._L.ws_store_raycast_records_dev(seam_store.handle, C.byref(n)) is None and n.value == 0
    # an empty store, and a box that meets no chunk: WS_OK, every record a no-hit
    empty = W.DeviceGlobalMap(TAU, 0)
    assert empty._L.ws_store_raycast_records_dev(empty.handle, C.byref(n)) is None and n.value == 0
    for store, kw in ((empty, {}), (empty, dict(lo=(-5, -5, -5), hi=(5, 5, 5))), (seam_store, dict(lo=(1000, 1000, 1000), hi=(1100, 1100, 1100)))):
        rec, grad = store.raycast(RES, o, d, 3000, any_weight=True, gradient=True, **kw)
        assert store.last_hits == 0 and np.all(rec["range_mm"] == -1) and not np.any(grad) and not np.any(rec["x_mm"])
    empty.close()


# ------------------------------------------------------------------------------------------------ 7. buffers
def test_buffers_repeat_prefix_and_old_results():
    import warpsense_amd as W
    chunks = dict(SM.seam_chunks())
    store = SM.make_store(chunks, segment_chunks=2)
    try:
        case = H.seam_cases()[1]
        want = H.want(case)
        check(store, case)
        check(store, case)  # the same bytes twice
        vert, face = store.mesh(RES)  # the mesh's buffers are apart
        L, h = store._L, store.handle
        n, got = C.c_size_t(0), C.c_size_t(0)
        k = len(want[0]) // 3
        part_r, part_g = np.zeros(k + 1, dtype=R.RAY), np.zeros((k + 1, 3), dtype=np.int32)
        assert L.ws_store_raycast_download(h, part_r.ctypes.data_as(C.c_void_p), part_g.ctypes.data_as(C.c_void_p), k, C.byref(got)) == 0
        assert got.value == len(want[0]) and QM.same(part_r[:k], want[0][:k]) and QM.same(part_g[:k], want[1][:k])
        assert not part_r[k:].view(np.uint8).any() and not part_g[k:].any()  # a prefix, nothing beyond the capacity
        assert L.ws_store_raycast_download(h, None, None, 0, C.byref(got)) == 0 and got.value == len(want[0])
        ptr_r, ptr_g = L.ws_store_raycast_records_dev(h, C.byref(n)), L.ws_store_raycast_gradient_dev(h, C.byref(n))
        assert ptr_r and ptr_g and n.value == len(want[0])
        # the result stays readable while the store goes on: a save_box that creates and overwrites chunks, a drop, a put into its slot
        lm = W.LocalMap(21, 17, 13, TAU, 0)
        t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
        lo, hi = QM.window(lm.size, lm.pos)
        t.avg_map().insert_box(lo, hi, M.draw_entries(tuple(int(s) for s in lm.size), seed=5))
        store.save_box(t, lo, hi)
        slots = store.capacity()
        store.drop_chunk((-1, 0, 0))
        store.put_chunk((1, 0, 0), M.draw_entries((CS,) * 3, seed=77))
        assert store.capacity() == slots
        assert M.same(store.mesh(RES, lo=(-64,) * 3, hi=(-1,) * 3), store.mesh(RES, lo=(-64,) * 3, hi=(-1,) * 3))
        full_r, full_g = np.zeros(len(want[0]), dtype=R.RAY), np.zeros((len(want[0]), 3), dtype=np.int32)
        assert L.ws_store_raycast_download(h, full_r.ctypes.data_as(C.c_void_p), full_g.ctypes.data_as(C.c_void_p), len(full_r), C.byref(got)) == 0
        assert R.same((full_r, full_g), want)
        assert (L.ws_store_raycast_records_dev(h, C.byref(n)), L.ws_store_raycast_gradient_dev(h, C.byref(n))) == (ptr_r, ptr_g)
        # ... and the next call sees the store as it is now
        now = {key: store.chunk(key) for key in store.keys()}
        assert len(now) == 8  # the save created (0, 0, -1)
        fresh = dict(case, name="seam sphere after the changes", chunks=lambda: now)
        assert not QM.same(H.want(fresh)[0], want[0])
        check(store, fresh)
        # without WS_RAYCAST_GRADIENT there is no gradient to fetch
        cast(store, case, gradient=False)
        assert L.ws_store_raycast_gradient_dev(h, C.byref(n)) is None and n.value == 0
        assert L.ws_store_raycast_download(h, part_r.ctypes.data_as(C.c_void_p), part_g.ctypes.data_as(C.c_void_p), 5, C.byref(got)) == WS_ERR_INVALID
        ms = store.raycast_timing(1)
        cast(store, case)
        ms = store.raycast_timing(0)
        assert len(ms) == 3 and all(v > 0.0 for v in ms)
        t.close()
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 8. after real use
def walk_pose(k):
    pose = np.eye(4)
    pose[:3, 3] = np.asarray(SM.WALK[k], dtype=np.float64) * RES / 1000.0
    return pose


def test_after_real_use():
    import warpsense_amd as W
    from window_routes import _params
    from warpsense_amd import synthetic as S
    size = (65, 65, 65)
    g = W.GlobalMap(TAU, 0)
    lm = W.LocalMap(*size, TAU, 0, g)
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
    with pytest.raises(W.WsError):
        W.TSDFMapping(_params(size), W.LocalMap(*size, TAU, 0)).global_raycast(np.eye(4))
    for k, pos in enumerate(SM.WALK):
        if k:
            tm.shift_map_device(pos)
        tm.update_tsdf(SM.walk_scan(k), pos_rm=pos, up_rm=(0, 0, 32768))
    dirs = S.os1_128_dirs().reshape(-1, 3)[::64]
    assert len(dirs) == 2048
    first = walk_pose(0)
    rec, grad = tm.global_raycast(first, dirs, gradient=True)
    rec_w, _ = tm.raycast(first, dirs, max_range_mm=tm._global_range_mm((0, 0, 0)))
    assert tm.tsdf().stats()["error_flags"] == 0
    lo, hi = lm.window()
    assert lo[0] > 0  # the window has moved on: the first pose lies outside it
    tm.write_back()
    chunks = {k: v.reshape(-1) for k, v in g.chunks.items()}
    assert sorted(chunks) == sorted(store.keys())
    o, d = W.TSDFMapping.raycast_rays(first, dirs)
    rng = tm._global_range_mm(o)
    want = R.model(H.Chunks(chunks), RES, o, d, rng)
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    tm.tsdf().avg_map().to_host(host)
    want_w = R.model_of(host, RES, o, d, rng)
    print("global hits", H.hits_of(want[0]), "window hits", H.hits_of(want_w[0]), "of", len(d), "range", rng)
    assert H.hits_of(want[0]) > H.hits_of(want_w[0]) and H.hits_of(want[0]) > 200  # the model says the global cast sees more
    assert R.same((rec, grad), want) and QM.same(rec_w, want_w[0])
    assert H.hits_of(rec) > H.hits_of(rec_w)
    assert R.same(tm.global_raycast(first, dirs, any_weight=True, gradient=True), R.model(H.Chunks(chunks), RES, o, d, rng, True))
    # the residual of the last scan at the last pose: the window's values wherever both hit inside the window
    last = walk_pose(2)
    pts = SM.walk_scan(2)
    r_w, r_g = tm.scan_residual(pts, last), tm.global_scan_residual(pts, last)
    both = ~np.isnan(r_w) & ~np.isnan(r_g)
    print("residual: window hits", int((~np.isnan(r_w)).sum()), "global hits", int((~np.isnan(r_g)).sum()), "both", int(both.sum()))
    assert both.sum() > 1000 and np.array_equal(r_w[both], r_g[both])
    assert (~np.isnan(r_g)).sum() >= (~np.isnan(r_w)).sum()
    store.close()
