"""ws_store_distance — the distance field of the global map in device memory (the rules are stated in include/warpsense_hip.h)
against the numpy model that ws_map_distance is held to (distance_model.model_box), applied to a dense box assembled from host
copies of the chunks (store_scenes.assemble) with every voxel of an absent chunk raw 0: weight 0, unknown.  Every comparison
is bit for bit on the raw uint32 records, and on the site count.

tests/test_store_distance_host.py holds the assembled-box model against the brute-force minimum and checks the input condition of
every draw used here (SEEDS) without a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import distance_model as D
import query_model as QM
from store_distance_scenes import CS, CUT_BOXES, CW, FLAGS, MW, PILLAR_Y, PILLAR_Y_SEED, PILLAR_Z, PILLAR_Z_SEED, RANGES, RES, SEAM_SEED, TAU, WINDOW_SEED, make_store, model, pillar_chunks, seam_chunks, seam_model
import store_scenes as SM

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
KMAX, KMIN = (2 ** 31 - 1) // CS, -(2 ** 31) // CS  # the last and the first chunk key of int32 voxel space


@pytest.fixture(scope="module")
def seam_store():
    """seven chunks around the origin, (0, 0, -1) absent, in segments of two chunks; no test changes its chunks"""
    store = make_store(seam_chunks())
    yield store
    store.close()


def raw_distance(store, lo, hi, R, flags=0):
    sites = C.c_size_t(77)
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    rc = store._L.ws_store_distance(store.handle, p(a), p(b), R, flags, C.byref(sites))
    return rc, sites.value


def result(store):
    """the records of the last call as the store holds them now"""
    n = C.c_size_t(0)
    assert store._L.ws_store_distance_download(store.handle, None, 0, C.byref(n)) == 0
    rec = np.zeros(n.value, dtype=np.uint32)
    assert store._L.ws_store_distance_download(store.handle, rec.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) == 0 and n.value == rec.size
    return rec


def check(store, chunks, lo, hi, R, what, **kw):
    want, n_sites = model(chunks, *(SM.bounding_box(chunks) if lo is None else (lo, hi)), R, **kw)
    got = store.distance(lo=lo, hi=hi, max_dist_vox=R, **kw)
    assert D.same(got, want) and store.last_sites == n_sites, (what, lo, hi, R, kw, store.last_sites, n_sites)
    return got


@pytest.mark.parametrize("box", range(len(CUT_BOXES)))
def test_seams_cut_boxes_every_flag_and_range(seam_store, box):
    lo, hi = CUT_BOXES[box]
    assert all(a < 0 <= b for a, b in zip(lo, hi)) and any(a % CS and (b + 1) % CS for a, b in zip(lo, hi))
    compared = 0
    for kw, R in itertools.product(FLAGS, RANGES):
        want, n_sites = seam_model(lo, hi, R, **kw)
        got = seam_store.distance(lo=lo, hi=hi, max_dist_vox=R, **kw)
        assert D.same(got, want) and seam_store.last_sites == n_sites, (lo, hi, kw, R)
        compared += 1
    assert compared == 8 * 5
    # the absent chunk shows: class 0 everywhere in it, and sites only under UNKNOWN_OCCUPIED
    rec = seam_store.distance(lo=lo, hi=hi, max_dist_vox=3)
    hole = rec[-lo[0]:, -lo[1]:, :-lo[2]]
    assert hole.size > 0 and np.all(hole >> np.uint32(30) == 0)
    rec = seam_store.distance(lo=lo, hi=hi, max_dist_vox=3, unknown_occupied=True)
    assert not np.any(rec[-lo[0]:, -lo[1]:, :-lo[2]])


@pytest.mark.parametrize("unknown_occupied", (False, True))
def test_seams_whole_block(seam_store, unknown_occupied):
    lo, hi = (-CS,) * 3, (CS - 1,) * 3
    for R in (3, 40):
        want, n_sites = seam_model(lo, hi, R, unknown_occupied=unknown_occupied)
        got = seam_store.distance(max_dist_vox=R, unknown_occupied=unknown_occupied)  # the default box is the bounding box
        assert got.shape == (128,) * 3 and D.same(got, want) and seam_store.last_sites == n_sites, (R, unknown_occupied)
        if unknown_occupied:
            assert n_sites >= CW  # every voxel of the absent chunk


# ------------------------------------------------------------------------------------------------ 2. long lines
def test_long_lines_along_z_with_a_hole():
    """1 x 1 x 5 chunks, the middle one absent: five chunk steps per column and z lines past one 256-output segment of the row pass"""
    chunks = pillar_chunks(PILLAR_Z, PILLAR_Z_SEED)
    store = make_store(chunks)
    try:
        lo, hi = (20, 30, -150), (39, 49, 149)
        for R, kw in ((7, {}), (40, {}), (7, dict(unknown_occupied=True)), (40, dict(any_weight=True, unknown_occupied=True)), (40, dict(columns=True))):
            got = check(store, chunks, lo, hi, R, "pillar z", **kw)
            if not kw.get("columns"):
                hole = got[:, :, 150:150 + CS]  # world z 0 .. 63
                assert hole.shape == (20, 20, CS) and np.all(hole >> np.uint32(30) == 0)
                assert not np.any(hole) if kw.get("unknown_occupied") else np.all(hole & np.uint32(0xFFFFFF) > 0)
        got = check(store, chunks, None, None, 7, "pillar z, bounding box")
        assert got.shape == (CS, CS, 5 * CS)
    finally:
        store.close()


def test_long_lines_along_y_under_columns_with_a_hole():
    """1 x 5 x 1 chunks, the middle one absent, under COLUMNS: y lines past one 256-output segment of the row pass"""
    chunks = pillar_chunks(PILLAR_Y, PILLAR_Y_SEED)
    store = make_store(chunks)
    try:
        lo, hi = (20, -150, 30), (39, 149, 49)
        for R, kw in ((7, {}), (40, {}), (40, dict(unknown_occupied=True)), (255, dict(any_weight=True))):
            got = check(store, chunks, lo, hi, R, "pillar y", columns=True, **kw)
            hole = got[:, 150:150 + CS]
            assert hole.shape == (20, CS) and np.all(hole >> np.uint32(30) == 0)
            assert not np.any(hole) if kw.get("unknown_occupied") else np.all(hole & np.uint32(0xFFFFFF) > 0)
        check(store, chunks, lo, hi, 40, "pillar y, 3-D")
        # a column that lies partly in the hole and partly in a present chunk: z is cut by the box, y crosses the hole
        check(store, chunks, (0, 60, 0), (63, 70, 63), 7, "pillar y, across the hole's face", columns=True, unknown_occupied=True)
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 3. partial steps
PARTIAL = {
    "one voxel thick in x": ((5, -40, -30), (5, 45, 20)),
    "one voxel thick in y": ((-40, -1, -30), (45, -1, 20)),
    "one voxel thick in z": ((-40, -30, 0), (45, 20, 0)),
    "one voxel": ((-1, -1, 0), (-1, -1, 0)),
    "inside one chunk": ((-50, 10, 7), (-20, 40, 44)),
    "z from chunk offset 63 to offset 0 of the next chunk": ((-30, -30, -1), (20, 20, 0)),
    "z of one lane at the end of a chunk": ((-30, -30, 63), (20, 20, 63)),
    "exceeds the chunks on all sides": ((-70, -66, -65), (10, 70, 64)),
}


@pytest.mark.parametrize("name", sorted(PARTIAL))
def test_partial_steps(seam_store, name):
    lo, hi = PARTIAL[name]
    for R in (3, 40):
        for kw in (FLAGS if R == 3 else (FLAGS[0], dict(unknown_occupied=True, columns=True))):
            check(seam_store, seam_chunks(), lo, hi, R, name, **kw)


# ------------------------------------------------------------------------------------------------ 4. the window's bytes
def test_same_bytes_as_the_window():
    import warpsense_amd as W
    lm = W.LocalMap(65, 65, 65, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    try:
        lo, hi = QM.window(lm.size, lm.pos)
        assert tuple(lo) == (-32,) * 3 and tuple(hi) == (32,) * 3 and (store.default_raw >> 16) == 0  # fill_entry has weight 0
        t.avg_map().insert_box(lo, hi, D.draw_entries((65,) * 3, WINDOW_SEED))
        store.save_box(t, lo, hi)
        assert store.count() == 8
        store.drop_chunk((0, -1, 0))
        store.load_box(t, lo, hi)  # the voxels of the dropped chunk come back as fill_entry
        chunks = {k: store.chunk(k) for k in store.keys()}
        avg = t.avg_map()
        for a, b in ((tuple(lo), tuple(hi)), ((-20, -31, -5), (30, 2, 17))):
            for R, kw in ((7, {}), (7, dict(unknown_occupied=True, any_weight=True)), (40, dict(columns=True)), (40, {})):
                got_window = avg.distance(lo=a, hi=b, max_dist_vox=R, **kw)
                got_store = store.distance(lo=a, hi=b, max_dist_vox=R, **kw)
                assert D.same(got_store, got_window) and store.last_sites == avg.last_sites, (a, b, R, kw)
                want, n_sites = model(chunks, a, b, R, **kw)
                assert D.same(got_store, want) and store.last_sites == n_sites
        assert model(chunks, lo, hi, 7)[1] >= 3
    finally:
        store.close()
        t.close()


# ------------------------------------------------------------------------------------------------ 5. far positions
@pytest.mark.parametrize("corner", [(KMAX, KMAX, KMAX), (KMIN + 1, KMIN + 1, KMIN + 1), (KMAX, KMIN + 1, KMAX)])
def test_far_positions_give_the_records_of_the_near_case(seam_store, corner):
    """the seam chunks under keys moved by whole chunks so that the block ends at the last (begins at the first) chunk of int32 voxel
    space on each axis: translation by whole chunks leaves the records as they are"""
    store = make_store(seam_chunks(), shift=corner)
    try:
        assert all(max(k[d] for k in store.keys()) == KMAX or min(k[d] for k in store.keys()) == KMIN for d in range(3))
        move = lambda v: tuple(int(c + CS * s) for c, s in zip(v, corner))
        for (lo, hi), R, kw in ((CUT_BOXES[0], 7, {}), (CUT_BOXES[0], 40, dict(unknown_occupied=True, any_weight=True)),
                                (CUT_BOXES[1], 40, dict(columns=True)), (((-CS,) * 3, (CS - 1,) * 3), 3, {})):
            want, n_sites = seam_model(lo, hi, R, **kw)
            near = seam_store.distance(lo=lo, hi=hi, max_dist_vox=R, **kw)
            far = store.distance(lo=move(lo), hi=move(hi), max_dist_vox=R, **kw)
            assert D.same(far, near) and D.same(far, want) and store.last_sites == n_sites, (corner, lo, hi, R, kw)
        got = store.distance(max_dist_vox=3)  # the default box reaches the end of int32 voxel space
        assert D.same(got, seam_model((-CS,) * 3, (CS - 1,) * 3, 3)[0])
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 6. store semantics
def test_empty_store_and_boxes_without_chunks(seam_store):
    import warpsense_amd as W
    empty = W.DeviceGlobalMap(TAU, 0)
    try:
        n = C.c_size_t(9)
        assert empty._L.ws_store_distance_dev(empty.handle, C.byref(n)) is None and n.value == 0  # nothing before the first call
        assert raw_distance(empty, None, None, 7) == (0, 0) and result(empty).size == 0
        for columns in (False, True):
            rec = empty.distance(max_dist_vox=7, columns=columns)
            assert rec.size == 0 and empty.last_sites == 0
        lo, hi = (-5, -6, -7), (5, 6, 70)
        rec = empty.distance(lo=lo, hi=hi, max_dist_vox=7)
        assert rec.shape == (11, 13, 78) and np.all(rec == 49) and empty.last_sites == 0  # all unknown, no site
        rec = empty.distance(lo=lo, hi=hi, max_dist_vox=7, unknown_occupied=True)
        assert not np.any(rec) and empty.last_sites == 11 * 13 * 78  # every voxel a site
        rec = empty.distance(lo=lo, hi=hi, max_dist_vox=7, unknown_occupied=True, columns=True)
        assert rec.shape == (11, 13) and not np.any(rec) and empty.last_sites == 11 * 13
        assert np.all(empty.distance(lo=lo, hi=hi, max_dist_vox=7, columns=True) == 49) and empty.last_sites == 0
    finally:
        empty.close()
    # a box that meets no present chunk: in the absent chunk, and far away
    for lo, hi in (((1, 1, -60), (60, 60, -2)), ((1000, 1000, 1000), (1020, 1030, 1100))):
        for kw in (dict(), dict(unknown_occupied=True), dict(columns=True), dict(columns=True, unknown_occupied=True)):
            check(seam_store, seam_chunks(), lo, hi, 7, "no present chunk", **kw)
        assert np.all(seam_store.distance(lo=lo, hi=hi, max_dist_vox=7) == 49)


def test_drop_put_and_old_results():
    chunks = dict(seam_chunks())
    store = make_store(chunks)
    try:
        lo, hi = CUT_BOXES[0]
        first = check(store, chunks, lo, hi, 7, "before")
        gone = (-1, 0, 0)
        store.drop_chunk(gone)
        del chunks[gone]
        assert np.array_equal(result(store), first.reshape(-1))  # the old result stays until the next call
        second = check(store, chunks, lo, hi, 7, "after the drop")
        assert not D.same(second, first) and np.all(second[:-lo[0], -lo[1]:, -lo[2]:] >> np.uint32(30) == 0)
        fresh = D.draw_entries((CS,) * 3, SEAM_SEED)
        chunks[gone] = fresh
        store.put_chunk(gone, fresh)
        assert np.array_equal(result(store), second.reshape(-1))
        third = check(store, chunks, lo, hi, 7, "after the put")
        assert not D.same(third, second)
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 7. results and downloads
def test_repeatable_partial_downloads_and_apart_from_the_other_results(seam_store):
    import mesh_model as M
    import raycast_model as RC
    import warpsense_amd as W
    L, h = seam_store._L, seam_store.handle
    lo, hi = CUT_BOXES[0]
    rec = seam_store.distance(lo=lo, hi=hi, max_dist_vox=7)
    assert D.same(seam_store.distance(lo=lo, hi=hi, max_dist_vox=7), rec) and D.same(rec, seam_model(lo, hi, 7)[0])
    dev = seam_store.distance(lo=lo, hi=hi, max_dist_vox=7, device=True)
    assert dev.is_cuda and tuple(dev.shape) == rec.shape and np.array_equal(dev.cpu().numpy().view(np.uint32), rec)
    n = C.c_size_t(0)
    assert dev.data_ptr() == L.ws_store_distance_dev(h, C.byref(n)) and n.value == rec.size
    # a prefix comes back and the total is always reported
    part = np.zeros(1001, dtype=np.uint32)
    assert L.ws_store_distance_download(h, part.ctypes.data_as(C.c_void_p), 1000, C.byref(n)) == 0
    assert n.value == rec.size and np.array_equal(part[:1000], rec.reshape(-1)[:1000]) and part[1000] == 0
    assert L.ws_store_distance_download(h, None, 0, C.byref(n)) == 0 and n.value == rec.size
    big = np.zeros(rec.size + 5, dtype=np.uint32)
    assert L.ws_store_distance_download(h, big.ctypes.data_as(C.c_void_p), big.size, C.byref(n)) == 0
    assert n.value == rec.size and np.array_equal(big[:rec.size], rec.reshape(-1)) and not big[rec.size:].any()
    # the store's mesh and ray-cast results and a window's distance result survive a store distance call, and the other way round
    lm = W.LocalMap(15, 15, 15, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    wlo, whi = QM.window(lm.size, lm.pos)
    t.avg_map().insert_box(wlo, whi, D.draw_entries((15,) * 3, 22))
    wrec = t.avg_map().distance(max_dist_vox=7)
    vert, face = seam_store.mesh(RES, any_weight=True)
    o, d = RC.random_rays((128,) * 3, seed=3, lo=(-CS,) * 3, n=300)
    rays, _ = seam_store.raycast(RES, o, d.astype(np.int32), 3000, any_weight=True)
    assert len(vert) > 0 and len(face) > 0
    col = seam_store.distance(lo=lo, hi=hi, max_dist_vox=40, columns=True)
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    pv, pf = np.zeros(len(vert), dtype=M.VERT), np.zeros((len(face), 3), dtype=np.uint32)
    assert L.ws_store_mesh_download(h, pv.ctypes.data_as(C.c_void_p), pf.ctypes.data_as(C.c_void_p), len(vert), len(face), C.byref(gv), C.byref(gf)) == 0
    assert M.same((pv, pf), (vert, face))
    pr = np.zeros(300, dtype=RC.RAY)
    assert L.ws_store_raycast_download(h, pr.ctypes.data_as(C.c_void_p), None, 300, C.byref(n)) == 0 and n.value == 300 and QM.same(pr, rays)
    got = np.zeros(wrec.size, dtype=np.uint32)
    assert t._L.ws_map_distance_download(t.handle, got.ctypes.data_as(C.c_void_p), got.size, C.byref(n)) == 0 and np.array_equal(got, wrec.reshape(-1))
    seam_store.mesh(RES)
    seam_store.raycast(RES, o, d[:10].astype(np.int32), 3000)
    t.avg_map().distance(max_dist_vox=3, columns=True)
    assert np.array_equal(result(seam_store), col.reshape(-1)) and D.same(col, seam_model(lo, hi, 40, columns=True)[0])
    t.close()
    # the timing entry: four figures, the last one zero for columns
    assert seam_store.distance_timing(1) == (0.0,) * 4
    seam_store.distance(lo=lo, hi=hi, max_dist_vox=7)
    assert all(v > 0 for v in seam_store.distance_timing(-1))
    seam_store.distance(lo=lo, hi=hi, max_dist_vox=7, columns=True)
    ms = seam_store.distance_timing(0)
    assert len(ms) == 4 and all(v > 0 for v in ms[:3])


# ------------------------------------------------------------------------------------------------ 8. error codes
def test_error_codes_leave_the_last_result_and_launch_nothing():
    from window_routes import same_store, store_state
    import warpsense_amd as W
    chunks = {(0, 0, 0): seam_chunks()[(0, 0, 0)]}
    store = make_store(chunks)
    try:
        lo, hi = (-18, -18, -1), (81, 81, 63)
        last = check(store, chunks, lo, hi, 7, "the last result")
        before = store_state(store)
        I32 = (-2 ** 31, 2 ** 31 - 1)
        refused = [
            ("R = 0", WS_ERR_RANGE, (lo, hi, 0, 0)), ("R = 256", WS_ERR_RANGE, (lo, hi, 256, 0)), ("R = 0, default box", WS_ERR_RANGE, (None, None, 0, 0)),
            ("an unknown flag bit", WS_ERR_INVALID, (lo, hi, 7, 8)), ("an unknown flag bit next to known ones", WS_ERR_INVALID, (None, None, 7, 0x17)),
            ("lo is NULL", WS_ERR_INVALID, (None, hi, 7, 0)), ("hi is NULL", WS_ERR_INVALID, (lo, None, 7, 0)),
            ("hi < lo", WS_ERR_INVALID, ((0, 0, 0), (5, -1, 5), 7, 0)), ("hi < lo under COLUMNS", WS_ERR_INVALID, ((0, 0, 5), (5, 5, 4), 7, 4)),
            ("2^32 records", WS_ERR_RANGE, ((0, 0, 0), (2047, 2047, 1023), 7, 0)),
            ("all of int32 in z, 3-D", WS_ERR_RANGE, ((-18, -18, I32[0]), (81, 81, I32[1]), 7, 0)),
            ("2^32 columns", WS_ERR_RANGE, ((0, 0, 0), (65535, 65535, 0), 7, 4)),
            ("all of int32 voxel space", WS_ERR_RANGE, ((I32[0],) * 3, (I32[1],) * 3, 7, 0)),
        ]
        for name, want_rc, (a, b, R, flags) in refused:
            rc, sites = raw_distance(store, a, b, R, flags)
            assert rc == want_rc, (name, rc)
            assert np.array_equal(result(store), last.reshape(-1)), name
        with pytest.raises(W.WsError):
            store.distance(max_dist_vox=0)
        with pytest.raises(W.WsError):
            store.distance(lo=(0, 0, 0), max_dist_vox=7)
        assert same_store(store_state(store), before)
        # the x, y box of the refused 3-D call under COLUMNS, all of int32 in z, over one chunk: accepted.  Every column holds unknown
        # voxels whichever way the box is cut below z = 0, so the rules give the records of the box that starts at z = -1
        for kw in (dict(), dict(unknown_occupied=True), dict(any_weight=True)):
            want, n_sites = model(chunks, lo, hi, 7, columns=True, **kw)
            got = store.distance(lo=(-18, -18, I32[0]), hi=(81, 81, I32[1]), max_dist_vox=7, columns=True, **kw)
            assert got.shape == (100, 100) and D.same(got, want) and store.last_sites == n_sites, kw
        occupied_columns = int(np.count_nonzero(D.sites_and_classes(chunks[(0, 0, 0)].reshape(CS, CS, CS), columns=True)[0]))
        assert raw_distance(store, (0, 0, 0), (2047, 2047, 1022), 7, 4) == (0, occupied_columns) and occupied_columns > 100  # 2^22 columns
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 9. after real use
def test_after_real_use():
    """the three-position walk of test_gpu_store_mesh.test_after_real_use: the window shifts through the device global map"""
    import warpsense_amd as W
    from window_routes import _params
    size = (65, 65, 65)
    lm = W.LocalMap(*size, TAU, 0, W.GlobalMap(TAU, 0))
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
    with pytest.raises(W.WsError):
        W.TSDFMapping(_params(size), W.LocalMap(*size, TAU, 0)).global_distance_field()
    try:
        for k, pos in enumerate(SM.WALK):
            if k:
                tm.shift_map_device(pos)
            tm.update_tsdf(SM.walk_scan(k), pos_rm=pos, up_rm=(0, 0, 32768))
        lo, hi = lm.window()
        band = (int(lo[2]) + 20, int(hi[2]) - 20)
        col = tm.global_distance_field(max_dist_m=1.0, columns=True)  # saves the window into the chunks first
        assert tm.tsdf().stats()["error_flags"] == 0
        chunks = {k: store.chunk(k) for k in store.keys()}
        outside = [k for k in chunks if any(k[d] * CS + CS - 1 < lo[d] or k[d] * CS > hi[d] for d in range(3))]
        assert len(outside) >= 2, sorted(chunks)
        blo, bhi = SM.bounding_box(chunks)
        want, n_sites = model(chunks, blo, bhi, 20, columns=True)
        assert n_sites > 100 and D.same(col, want) and store.last_sites == n_sites
        assert D.same(store.distance(max_dist_vox=20, columns=True), want)
        # the 2-D cost map of the robot's height band over the whole store, and a 3-D cut box that is in no single window
        a, b = (int(blo[0]), int(blo[1]), band[0]), (int(bhi[0]), int(bhi[1]), band[1])
        want, n_sites = model(chunks, a, b, 20, columns=True)
        assert D.same(tm.global_distance_field(lo=a, hi=b, max_dist_m=1.0, columns=True), want) and store.last_sites == n_sites
        a, b = (-20, -40, -30), (70, 10, 30)
        for kw in (dict(), dict(unknown_occupied=True)):
            want, n_sites = model(chunks, a, b, 8, **kw)
            got = tm.global_distance_field(lo=a, hi=b, max_dist_m=0.4, **kw)  # 400 mm / 50 mm = 8 voxels
            assert n_sites > 100 and D.same(got, want) and store.last_sites == n_sites, kw
            assert D.same(store.distance(lo=a, hi=b, max_dist_vox=8, **kw), want)
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 10. lifecycle
def test_create_distance_destroy_gives_its_memory_back():
    """in the manner of tests/test_gpu_lifecycle.py: free device memory after a cycle must not lie below the figure after the cycle
    before it by more than that file's margin; the first cycle warms the runtime's pools and is left out"""
    import torch
    import warpsense_amd as W
    from lifecycle_model import CYCLES, MARGIN
    chunks = {k: seam_chunks()[k] for k in ((-1, -1, -1), (0, 0, 0))}
    free = []
    for _ in range(CYCLES):
        store = make_store(chunks)
        rec = store.distance(max_dist_vox=7)                            # records, planes, the counter, the chunk table
        assert rec.shape == (128,) * 3 and store.last_sites > 0
        assert store.distance(lo=(-3, -3, -3), hi=(2, 2, 2), max_dist_vox=3, columns=True).shape == (6, 6)
        store.distance_timing(1)
        store.distance(lo=(-3, -3, -3), hi=(2, 2, 2), max_dist_vox=3)  # the events
        store.close()
        W.Context.default().sync()
        torch.cuda.synchronize()
        free.append(int(torch.cuda.mem_get_info()[0]))
    drops = [free[k] - free[k + 1] for k in range(CYCLES - 1)]
    print(f"store distance lifecycle: free bytes after each cycle {free}, drops after the first {drops}, margin {MARGIN}")
    assert max(drops) <= MARGIN, (free, drops)
