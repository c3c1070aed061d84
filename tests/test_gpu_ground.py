"""ws_map_ground / ws_store_ground and the bridge ws_*_ground_distance (the rules are stated in include/warpsense_hip.h) against the
numpy model written from those rules (ground_model.py): device bytes for records and counts, on the smallest shapes at which the walk
can still go wrong -- levels at lz = 62, 63 and 0 of three stacked chunks, headroom across a chunk border and into an absent chunk,
boxes cut in mid-chunk, rotated rings -- and the planner over a ramp and a kerb.  tests/test_ground_host.py holds the model against
answers written out by hand, without a GPU."""
import ctypes as C

import numpy as np
import pytest

import distance_model as D
import ground_model as G
import ground_scenes as S
import query_model as QM
import reach_model as RM
import store_scenes as SM

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
INF = 0xFFFFFFFF


@pytest.fixture(scope="module")
def stack():
    store = S.make_store(S.stack_chunks())
    yield store
    store.close()


@pytest.fixture(scope="module")
def holed():
    """the stack without its middle layer of chunks"""
    store = S.make_store(S.stack_chunks(absent_layer=1))
    yield store
    store.close()


def check_store(store, absent, lo, hi, H, what="", **kw):
    want, counts = S.stack_model(absent, lo, hi, H, **kw)
    got = store.ground(lo=lo, hi=hi, clear_vox=H, **kw)
    assert G.same(got.records, want) and np.array_equal(got.counts, counts), (what, lo, hi, H, kw, got.counts, counts)
    assert got.lo == tuple(lo) and got.ext == tuple(b - a + 1 for a, b in zip(lo, hi))
    return got


def at(result, x, y):
    r = result.records[x - result.lo[0], y - result.lo[1]]
    return int(r["w"]) >> 30, int(r["z"])


# ------------------------------------------------------------------------------------------------ 1. the store
@pytest.mark.parametrize("H", (1, 3, 20, 64))
def test_store_three_stacked_chunks_every_flag(stack, H):
    lo, hi = S.FULL_BOX
    for kw in S.FLAGS:
        got = check_store(stack, None, lo, hi, H, "stack", **kw)
    base = check_store(stack, None, lo, hi, H)
    # the planted floors are found where they were planted, as long as their free space holds the headroom
    for name, (x, y, z, free) in S.PLANTED.items():
        assert at(base, x, y) == ((G.GROUND, z) if free >= H else (G.BLOCKED, 0)), (name, H)
    assert int(base.counts[G.GROUND]) >= 3


def test_store_headroom_into_an_absent_chunk(stack, holed):
    lo, hi = S.FULL_BOX
    for H in (2, 3, 40, 64):
        for kw in ({}, dict(unknown_headroom=True), dict(unknown_headroom=True, top=True), dict(top=True, any_weight=True)):
            check_store(holed, 1, lo, hi, H, "holed", **kw)
    x, y, z, _ = S.PLANTED["lz 62"]          # z + 1 = 63 is free, everything above lies in the absent layer
    assert at(check_store(holed, 1, lo, hi, 1), x, y) == (G.GROUND, z)
    assert at(check_store(holed, 1, lo, hi, 2), x, y) == (G.BLOCKED, 0)
    assert at(check_store(holed, 1, lo, hi, 64, unknown_headroom=True), x, y) == (G.GROUND, z)
    x, y, z, _ = S.PLANTED["lz 63"]          # z + 1 is a voxel of an absent chunk: never a level
    assert at(check_store(holed, 1, lo, hi, 1, unknown_headroom=True), x, y) == (G.BLOCKED, 0)
    x, y, z, _ = S.PLANTED["free ends at the border"]  # present chunks: the voxels above the free space are unknown entries
    assert at(check_store(stack, None, lo, hi, 3), x, y) == (G.GROUND, z) and at(check_store(stack, None, lo, hi, 4), x, y) == (G.BLOCKED, 0)
    assert at(check_store(stack, None, lo, hi, 64, unknown_headroom=True), x, y) == (G.GROUND, z)


def test_store_boxes_cut_in_mid_chunk(stack, holed):
    for H in (1, 7, 64):
        for kw in ({}, dict(unknown_headroom=True), dict(top=True)):
            check_store(stack, None, (-5, -3, 20), (3, 2, 150), H, "cut at both ends", **kw)
            check_store(holed, 1, (-5, -3, 70), (3, 2, 120), H, "inside the absent layer", **kw)     # over no chunk at all
            check_store(holed, 1, (-5, -3, 30), (3, 2, 120), H, "the top lies in the absent layer", **kw)
            check_store(holed, 1, (-5, -3, 70), (3, 2, 170), H, "the bottom lies in the absent layer", **kw)
    x, y, z, free = S.PLANTED["mid-chunk"]
    H = 7
    assert at(check_store(stack, None, (x - 1, y - 1, 90), (x, y, z + H), H), x, y) == (G.GROUND, z)        # z + H = hi_z qualifies
    assert at(check_store(stack, None, (x - 1, y - 1, 90), (x, y, z + H - 1), H), x, y) == (G.BLOCKED, 0)   # z + H = hi_z + 1 does not
    assert at(check_store(stack, None, (x - 1, y - 1, z), (x, y, z + H), H), x, y) == (G.GROUND, z)          # z = lo_z
    assert at(check_store(stack, None, (x - 1, y - 1, z + 1), (x, y, z + 20), H), x, y) == (G.VOID, 0)
    x, y, z, free = S.PLANTED["lz 63, headroom to the top"]
    assert at(check_store(stack, None, (x, y, 0), (x, y, 191), 64), x, y) == (G.GROUND, z)                   # a 1 x 1 box
    assert at(check_store(stack, None, (x, y, 0), (x, y, 190), 64), x, y) == (G.BLOCKED, 0)
    assert at(check_store(stack, None, (x, y, 127), (x, y, 191), 64, top=True), x, y) == (G.GROUND, z)


def test_store_negative_keys_and_the_default_box(stack):
    shift = (-3, -2, -5)
    far = S.make_store(S.stack_chunks(), shift=shift)
    try:
        move = lambda v: tuple(int(c + S.CS * s) for c, s in zip(v, shift))
        for (lo, hi), H, kw in ((S.FULL_BOX, 3, {}), (S.FULL_BOX, 64, dict(unknown_headroom=True)), (((-5, -3, 20), (3, 2, 150)), 20, dict(top=True, any_weight=True))):
            want, counts = S.stack_model(None, lo, hi, H, **kw)
            got = far.ground(lo=move(lo), hi=move(hi), clear_vox=H, **kw)
            moved = want.copy()
            moved["z"] = np.where(want["w"] >> 30 == G.GROUND, want["z"] + S.CS * shift[2], 0)
            assert G.same(got.records, moved) and np.array_equal(got.counts, counts) and got.lo == move(lo), (lo, hi, H, kw)
    finally:
        far.close()
    # the default box is the bounding box of the chunks; a column's level does not depend on the box's x and y extent, its step on its
    # eight neighbours only
    whole = stack.ground(clear_vox=3)
    assert whole.records.shape == (128, 128) and whole.lo == (-64, -64, 0) and whole.ext == (128, 128, 192) and int(whole.counts.sum()) == 128 * 128
    lo, hi = S.FULL_BOX
    want, _ = S.stack_model(None, lo, hi, 3)
    part = whole.records[lo[0] + 64:hi[0] + 65, lo[1] + 64:hi[1] + 65]
    assert np.array_equal(part["z"], want["z"]) and np.array_equal(part["w"] & 0xC00000FF, want["w"] & 0xC00000FF)
    assert np.array_equal(part["w"][1:-1, 1:-1], want["w"][1:-1, 1:-1])
    rlo, rhi = S.REGION_LO, tuple(a + n - 1 for a, n in zip(S.REGION_LO, S.REGION_SHAPE))
    assert int(whole.counts[G.UNKNOWN]) == 128 * 128 - 12 * 8 + int(S.stack_model(None, rlo, rhi, 3)[1][G.UNKNOWN])  # the region holds the only entries


def test_store_without_chunks(stack):
    import warpsense_amd as W
    empty = W.DeviceGlobalMap(S.TAU, 0)
    try:
        n = C.c_size_t(9)
        assert empty._L.ws_store_ground_dev(empty.handle, C.byref(n)) is None and n.value == 0  # nothing before the first call
        with pytest.raises(W.WsError):
            empty.ground_distance(256)                                                            # no ground result yet
        g = empty.ground(clear_vox=3)
        assert g.records.shape == (0, 0) and not g.counts.any()                                  # zero columns is WS_OK
        assert empty.ground_distance(256).shape == (0, 0)
        g = empty.ground(lo=(-5, -6, -7), hi=(3, -1, 70), clear_vox=3, unknown_headroom=True)
        assert g.records.shape == (9, 6) and not g.records["z"].any() and not g.records["w"].any() and g.counts.tolist() == [54, 0, 0, 0]
    finally:
        empty.close()
    g = stack.ground(lo=(1000, 1000, 1000), hi=(1008, 1005, 1100), clear_vox=64)  # a box over no chunk at all
    assert not g.records["w"].any() and g.counts.tolist() == [54, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 2. the window
WINDOW = ((32, 32, 32), (3, -2, 5), (17, 19, 21))
TALL = ((6, 5, 150), (-2, 1, 40), (1, 3, 97))  # three steps of the column walk, and the ring's seam in z inside the second


@pytest.mark.parametrize("size,pos,off", (WINDOW, TALL))
def test_window_on_a_shifted_and_wrapped_ring(size, pos, off):
    box = S.window_box(size, 4200 + size[2], 40 if size[2] == 32 else 70)
    t, lo, hi = S.make_window(size, pos, off, box)
    try:
        avg = t.avg_map()
        assert all(o != 0 for o in off)
        inner = (tuple(int(a + 2) for a in lo), (lo[0] + 10, lo[1] + 7, hi[2] - 1)) if size[2] == 32 else ((lo[0], lo[1], lo[2] + 30), (hi[0], hi[1], lo[2] + 135))
        for H in ((1, 4, 28, 31) if size[2] == 32 else (1, 20, 64)):
            for kw in S.FLAGS:
                want, counts = G.model_box(box.reshape(size), lo, H, **kw)
                got = avg.ground(clear_vox=H, **kw)  # the whole window
                assert G.same(got.records, want) and np.array_equal(got.counts, counts) and got.lo == lo and got.ext == tuple(size), ("window", H, kw)
            for kw in (S.FLAGS[0], S.FLAGS[3], S.FLAGS[6]):
                a, b = inner
                cut = box.reshape(size)[tuple(slice(a[k] - lo[k], b[k] - lo[k] + 1) for k in range(3))]
                want, counts = G.model_box(cut, a, H, **kw)
                got = avg.ground(lo=a, hi=b, clear_vox=H, **kw)
                assert G.same(got.records, want) and np.array_equal(got.counts, counts), ("inner", H, kw)
        g = avg.ground(clear_vox=1)
        nz = size[2]
        assert at(g, lo[0] + 1, lo[1] + 1) == (G.GROUND, lo[2] + 2) and at(g, lo[0] + 2, lo[1] + 1) == (G.GROUND, lo[2] + nz - 2)
        assert at(g, lo[0] + 3, lo[1] + 2) == (G.BLOCKED, 0)
        # negative weights are entries under ANY_WEIGHT only: the two results differ
        assert not G.same(avg.ground(clear_vox=1, any_weight=True).records, g.records)
    finally:
        t.close()


def test_window_gives_the_bytes_of_the_store(stack):
    """the box of the stack that a 32 x 32 x 150 window holds: the same records from ws_map_ground and ws_store_ground"""
    import warpsense_amd as W
    size, pos, off = (32, 32, 150), (0, 0, 80), (5, 7, 11)
    lo, hi = QM.window(size, pos)
    t, lo, hi = S.make_window(size, pos, off, SM.assemble(S.stack_chunks(), lo, hi))
    try:
        for H, kw in ((3, {}), (64, dict(unknown_headroom=True)), (20, dict(top=True, any_weight=True))):
            a, b = (-5, -3, lo[2]), (3, 2, hi[2])
            w, s = t.avg_map().ground(lo=a, hi=b, clear_vox=H, **kw), stack.ground(lo=a, hi=b, clear_vox=H, **kw)
            assert G.same(w.records, s.records) and np.array_equal(w.counts, s.counts) and int(w.counts[G.GROUND]) > 0, (H, kw)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 3. refusals and results
def raw_ground(L, name, handle, lead, lo, hi, H, flags):
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    counts = np.full(4, 77, dtype=np.uint64)
    return getattr(L, name)(handle, *lead, p(a), p(b), H, flags, counts.ctypes.data_as(C.c_void_p))


def downloaded(L, name, handle):
    n = C.c_size_t(0)
    assert getattr(L, name)(handle, None, 0, C.byref(n)) == 0
    rec = np.zeros(n.value, dtype=G.REC)
    assert getattr(L, name)(handle, rec.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) == 0 and n.value == rec.size
    return rec


def test_store_refusals_leave_the_last_results(stack):
    from window_routes import same_store, store_state
    L, h = stack._L, stack.handle
    lo, hi = S.FULL_BOX
    last = check_store(stack, None, lo, hi, 3).records.copy()
    dist = stack.ground_distance(300, max_dist_vox=5)
    before = store_state(stack)
    I32 = (-2 ** 31, 2 ** 31 - 1)
    for name, want_rc, (a, b, H, flags) in [
            ("H = 0", WS_ERR_RANGE, (lo, hi, 0, 0)), ("H = 65", WS_ERR_RANGE, (lo, hi, 65, 0)), ("H = 65, default box", WS_ERR_RANGE, (None, None, 65, 0)),
            ("an unknown flag bit", WS_ERR_INVALID, (lo, hi, 3, 8)), ("lo is NULL", WS_ERR_INVALID, (None, hi, 3, 0)), ("hi is NULL", WS_ERR_INVALID, (lo, None, 3, 0)),
            ("hi < lo", WS_ERR_INVALID, ((0, 0, 5), (5, 5, 4), 3, 0)), ("2^32 columns", WS_ERR_RANGE, ((0, 0, 0), (65535, 65535, 0), 3, 0)),
            ("all of int32 voxel space", WS_ERR_RANGE, ((I32[0],) * 3, (I32[1],) * 3, 3, 0))]:
        assert raw_ground(L, "ws_store_ground", h, (), a, b, H, flags) == want_rc, name
        assert G.same(downloaded(L, "ws_store_ground_download", h).reshape(last.shape), last), name
    sites = C.c_size_t(0)
    for name, want_rc, (step, R, flags) in [("step = -1", WS_ERR_RANGE, (-1, 5, 0)), ("step = 65536", WS_ERR_RANGE, (65536, 5, 0)), ("R = 0", WS_ERR_RANGE, (300, 0, 0)),
                                           ("R = 256", WS_ERR_RANGE, (300, 256, 0)), ("COLUMNS is implied, not accepted", WS_ERR_INVALID, (300, 5, 4)),
                                           ("ANY_WEIGHT", WS_ERR_INVALID, (300, 5, 1)), ("an unknown bit", WS_ERR_INVALID, (300, 5, 8))]:
        assert L.ws_store_ground_distance(h, step, R, flags, C.byref(sites)) == want_rc, name
        got = np.zeros(dist.size, dtype=np.uint32)
        n = C.c_size_t(0)
        assert L.ws_store_distance_download(h, got.ctypes.data_as(C.c_void_p), got.size, C.byref(n)) == 0 and n.value == dist.size and np.array_equal(got, dist.reshape(-1)), name
    assert same_store(store_state(stack), before)
    # all of int32 in z over the stack: accepted, and the records of the box that ends where the chunks end
    got = stack.ground(lo=(lo[0], lo[1], I32[0]), hi=(hi[0], hi[1], I32[1]), clear_vox=64, unknown_headroom=True)
    want, counts = S.stack_model(None, (lo[0], lo[1], -64), (hi[0], hi[1], 320), 64, unknown_headroom=True)
    assert G.same(got.records, want) and np.array_equal(got.counts, counts)
    # the ground result survives a distance call and the other way round
    kept = stack.ground(lo=lo, hi=hi, clear_vox=3).records.copy()
    d3 = stack.distance(lo=(-5, -3, 0), hi=(3, 2, 20), max_dist_vox=3)
    assert G.same(downloaded(L, "ws_store_ground_download", h).reshape(kept.shape), kept)
    stack.ground(lo=(0, 0, 0), hi=(2, 2, 70), clear_vox=5)
    got = np.zeros(d3.size, dtype=np.uint32)
    n = C.c_size_t(0)
    assert L.ws_store_distance_download(h, got.ctypes.data_as(C.c_void_p), got.size, C.byref(n)) == 0 and np.array_equal(got, d3.reshape(-1))
    # device tensors alias the buffers; the timing entry gives two figures
    dev = stack.ground(lo=lo, hi=hi, clear_vox=3, device=True)
    assert dev.records.is_cuda and tuple(dev.records.shape) == (9, 6, 2) and np.array_equal(dev.records.cpu().numpy().view(np.uint32).reshape(-1), kept.view(np.uint32).reshape(-1))
    assert dev.records.data_ptr() == L.ws_store_ground_dev(h, C.byref(n)) and n.value == 54
    assert stack.ground_timing(1) == (0.0, 0.0)
    stack.ground(lo=lo, hi=hi, clear_vox=3)
    assert all(v > 0 for v in stack.ground_timing(0))


def test_window_refusals_leave_the_last_results():
    size, pos, off = WINDOW
    box = S.window_box(size, 4232, 40)
    t, lo, hi = S.make_window(size, pos, off, box)
    try:
        import warpsense_amd as W
        L, h, avg = t._L, t.handle, t.avg_map()
        n = C.c_size_t(9)
        assert L.ws_map_ground_dev(h, C.byref(n)) is None and n.value == 0
        with pytest.raises(W.WsError):
            avg.ground_distance(256)
        last = avg.ground(clear_vox=4).records.copy()
        dist = avg.ground_distance(300, max_dist_vox=5)
        want, sites = G.bridge_model(last, 300, 5)
        assert D.same(dist, want) and avg.last_sites == sites
        out = (hi[0] + 1, hi[1], hi[2])
        for name, want_rc, (which, a, b, H, flags) in [
                ("H = 0", WS_ERR_RANGE, (0, None, None, 0, 0)), ("H = 65", WS_ERR_RANGE, (0, lo, hi, 65, 0)), ("an unknown flag bit", WS_ERR_INVALID, (0, lo, hi, 3, 8)),
                ("which = 2", WS_ERR_INVALID, (2, lo, hi, 3, 0)), ("lo is NULL", WS_ERR_INVALID, (0, None, hi, 3, 0)), ("hi < lo", WS_ERR_INVALID, (0, hi, lo, 3, 0)),
                ("outside the window", WS_ERR_INVALID, (0, lo, out, 3, 0))]:
            assert raw_ground(L, "ws_map_ground", h, (which,), a, b, H, flags) == want_rc, name
            assert G.same(downloaded(L, "ws_map_ground_download", h).reshape(last.shape), last), name
        s = C.c_size_t(0)
        for name, want_rc, (step, R, flags) in [("step = -1", WS_ERR_RANGE, (-1, 5, 0)), ("step = 65536", WS_ERR_RANGE, (65536, 5, 0)), ("R = 256", WS_ERR_RANGE, (300, 256, 0)),
                                               ("COLUMNS", WS_ERR_INVALID, (300, 5, 4)), ("ANY_WEIGHT", WS_ERR_INVALID, (300, 5, 1))]:
            assert L.ws_map_ground_distance(h, step, R, flags, C.byref(s)) == want_rc, name
            got = np.zeros(dist.size, dtype=np.uint32)
            assert L.ws_map_distance_download(h, got.ctypes.data_as(C.c_void_p), got.size, C.byref(n)) == 0 and n.value == dist.size and np.array_equal(got, dist.reshape(-1)), name
        # the ground result survives a distance call and the other way round; both maps have the one result
        d3 = avg.distance(max_dist_vox=3, columns=True)
        assert G.same(downloaded(L, "ws_map_ground_download", h).reshape(last.shape), last)
        new = t.new_map().ground(clear_vox=4)
        assert int(new.counts[G.GROUND]) == 0
        got = np.zeros(d3.size, dtype=np.uint32)
        assert L.ws_map_distance_download(h, got.ctypes.data_as(C.c_void_p), got.size, C.byref(n)) == 0 and np.array_equal(got, d3.reshape(-1))
        assert avg.ground_timing(1) == (0.0, 0.0)
        avg.ground(clear_vox=4)
        assert all(v > 0 for v in avg.ground_timing(0))
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 4. the bridge to the planner
def test_bridge_records_are_the_models_classes_through_the_column_transform(stack):
    lo, hi = S.FULL_BOX
    for H, kw in ((3, {}), (1, dict(any_weight=True)), (20, dict(unknown_headroom=True))):
        rec = check_store(stack, None, lo, hi, H, **kw).records
        for step, R, unknown_occupied in ((0, 1, False), (256, 3, False), (700, 7, True), (65535, 40, False), (65535, 255, True)):
            want, sites = G.bridge_model(rec, step, R, unknown_occupied)
            got = stack.ground_distance(step, max_dist_vox=R, unknown_occupied=unknown_occupied)
            assert D.same(got, want) and stack.last_sites == sites, (H, kw, step, R, unknown_occupied)
    # a box over no chunk: every column unknown
    stack.ground(lo=(1000, 1000, 1000), hi=(1008, 1005, 1100), clear_vox=3)
    assert np.all(stack.ground_distance(256, max_dist_vox=3) == 9) and stack.last_sites == 0
    assert not np.any(stack.ground_distance(256, max_dist_vox=3, unknown_occupied=True)) and stack.last_sites == 54


def ramp_checks(ground, ground_distance, distance, reach, origin):
    """the ramp scene at world `origin` through the new route and through the height band"""
    ox, oy, oz = origin
    nx, ny, nz = S.RAMP_SHAPE
    lo, hi = (ox, oy, oz), (ox + nx - 1, oy + ny - 1, oz + nz - 1)
    g = ground(lo=lo, hi=hi, clear_vox=8)
    want, counts = G.model_box(S.ramp_world(), lo, 8)
    assert G.same(g.records, want) and counts.tolist() == [0, nx * ny, 0, 0]
    assert int(g.step_q8.max()) == 256 and at(g, ox, oy) == (G.GROUND, oz + S.LOWER_Z) and at(g, ox + nx - 1, oy) == (G.GROUND, oz + S.UPPER_Z)
    seed = np.array([[ox + 1, oy + 2, oz + S.LOWER_Z + 1]], dtype=np.int32)
    d = ground_distance(300, max_dist_vox=2)
    want_d, sites = G.bridge_model(want, 300, 2)
    assert D.same(d, want_d) and sites == 0
    cost = reach(seed)
    want_cost, kept, reached = RM.field(want_d, lo, seed)
    assert np.array_equal(cost, want_cost) and kept == 1 and reached == nx * ny
    assert int(cost[nx - 1, 2]) == 10 * (nx - 2) and int(want_cost[nx - 1, 2]) == 10 * (nx - 2)  # straight up the ramp: 28 face steps
    # a robot that climbs less than one voxel per column stays below
    d = ground_distance(200, max_dist_vox=2)
    assert D.same(d, G.bridge_model(want, 200, 2)[0])
    cost = reach(seed)
    assert int(cost[nx - 1, 2]) == INF and int(cost[3, 2]) == 20
    # the same scene through the height band of the robot on the lower floor: the ramp is a wall where it enters the band
    band_lo, band_hi = (ox, oy, oz + S.BAND[0]), (ox + nx - 1, oy + ny - 1, oz + S.BAND[1])
    d = distance(lo=band_lo, hi=band_hi, max_dist_vox=2, columns=True)
    assert D.same(d, D.model_box(S.ramp_world()[:, :, S.BAND[0]:S.BAND[1] + 1], 2, columns=True)[0])
    cost = reach(seed)
    assert int(cost[3, 2]) == 20 and int(cost[nx - 1, 2]) == INF and np.all(cost[9:] == INF)


def test_ramp_and_kerb_on_the_store():
    origin = (60, 62, 40)  # the scene crosses a chunk border on every axis
    store = S.make_store(S.world_chunks(S.ramp_world(), origin))
    try:
        ramp_checks(store.ground, store.ground_distance, store.distance, lambda seed: store.reach(seed), origin)
    finally:
        store.close()
    store = S.make_store(S.world_chunks(S.kerb_world(), origin))
    try:
        nx, ny, nz = S.KERB_SHAPE
        lo, hi = origin, tuple(o + n - 1 for o, n in zip(origin, S.KERB_SHAPE))
        g = store.ground(lo=lo, hi=hi, clear_vox=8)
        want, _ = G.model_box(S.kerb_world(), lo, 8)
        assert G.same(g.records, want) and np.all(g.step_q8[5:7] == 512) and int(g.step_q8[:5].max()) == 0
        assert np.array_equal(g.traversable(2 * S.RES, S.RES), g.step_q8 <= 512) and not g.traversable(S.RES, S.RES)[5:7].any()
        assert g.height_mm(S.RES)[0, 0] == (origin[2] + 6 + 128 / 256) * S.RES
        seed = np.array([[lo[0], lo[1], 0]], dtype=np.int32)
        for step, blocked in ((256, True), (768, False)):  # a kerb of two voxels blocks with 256 and passes with 768
            d = store.ground_distance(step, max_dist_vox=2)
            want_d, _ = G.bridge_model(want, step, 2)
            cost = store.reach(seed)
            assert D.same(d, want_d) and np.array_equal(cost, RM.field(want_d, lo, seed)[0])
            assert (int(cost[nx - 1, 0]) == INF) == blocked and int(cost[4, 0]) == 40
    finally:
        store.close()


def test_ramp_on_the_window():
    size, pos, off = (32, 8, 32), (0, 0, 0), (9, 3, 20)
    lo, hi = QM.window(size, pos)
    box = np.zeros(size, dtype=np.uint32)
    box[1:31, 1:6, :] = S.ramp_world()
    t, lo, hi = S.make_window(size, pos, off, box)
    try:
        avg = t.avg_map()
        ramp_checks(avg.ground, avg.ground_distance, avg.distance, lambda seed: avg.reach(seed), (lo[0] + 1, lo[1] + 1, lo[2]))
    finally:
        t.close()


def test_mapping_ground_reach():
    """TSDFMapping.ground_reach chains ground -> ground_distance -> reach and returns the reach result"""
    import warpsense_amd as W
    size = (33, 9, 33)
    lm = W.LocalMap(*size, S.TAU, 0)
    params = W.Params(W.MapParams(resolution=S.RES, max_distance=S.TAU / 1000.0, max_weight=10, size=tuple(s * S.RES / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    lo, hi = lm.window()
    a = (int(lo[0]) + 1, int(lo[1]) + 1, int(lo[2]))
    b = tuple(o + n - 1 for o, n in zip(a, S.RAMP_SHAPE))
    tm.tsdf().avg_map().insert_box(a, b, S.ramp_world().reshape(-1))
    seed_mm = np.array([[(a[0] + 1) * S.RES + 3, (a[1] + 2) * S.RES + 3, 0]])
    cost = tm.ground_reach(seed_mm, robot_height_m=0.4, max_step_m=0.06, clearance_m=0.0, lo=a, hi=b)   # 8 voxels, 307/256 voxel
    want, _ = G.model_box(S.ramp_world(), a, 8)
    want_cost = RM.field(G.bridge_model(want, 307, 1)[0], a, np.array([[a[0] + 1, a[1] + 2, 0]]))[0]
    assert np.array_equal(cost, want_cost) and int(cost[-1, 2]) == 280 and tm.last_reach["reached"] == 150 and tm.last_ground.tolist() == [0, 150, 0, 0]
    assert int(tm.ground_reach(seed_mm, robot_height_m=0.4, max_step_m=0.03, lo=a, hi=b)[-1, 2]) == INF
    g = tm.ground(robot_height_m=0.4, lo=a, hi=b)
    assert G.same(g.records, want)
    with pytest.raises(W.WsError):
        tm.global_ground()


def test_mapping_global_ground_and_the_keywords_of_ground_reach():
    """TSDFMapping.global_ground flushes the window into the device global map and asks the store; ground_reach hands unknown_headroom,
    top and unknown_occupied on: over a box one column wider than the ramp the unknown rim is a row of sites"""
    import warpsense_amd as W
    from window_routes import _params
    size = (33, 9, 33)
    lm = W.LocalMap(*size, S.TAU, 0, W.GlobalMap(S.TAU, 0))
    store = W.DeviceGlobalMap(S.TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size, S.RES, S.TAU), lm, device_global_map=store)
    try:
        lo, hi = lm.window()
        a = (int(lo[0]) + 2, int(lo[1]) + 2, int(lo[2]))
        b = tuple(o + n - 1 for o, n in zip(a, S.RAMP_SHAPE))
        tm.tsdf().avg_map().insert_box(a, b, S.ramp_world().reshape(-1))
        want, counts = G.model_box(S.ramp_world(), a, 8)
        g = tm.global_ground(robot_height_m=0.4, lo=a, hi=b)
        assert store.count() > 0 and G.same(g.records, want) and np.array_equal(g.counts, counts) and g.lo == a
        assert G.same(store.ground(lo=a, hi=b, clear_vox=8).records, want) and G.same(tm.ground(robot_height_m=0.4, lo=a, hi=b).records, want)
        whole = tm.global_ground(robot_height_m=0.4)  # the bounding box of the chunks
        assert whole.counts[G.GROUND] == counts[G.GROUND] and whole.records.shape[0] % S.CS == 0
        # one column more on every side in x and y: unknown columns around the ramp
        a2, b2 = (a[0] - 1, a[1] - 1, a[2]), (b[0] + 1, b[1] + 1, b[2])
        box = np.zeros(tuple(n + 2 for n in S.RAMP_SHAPE[:2]) + (S.RAMP_SHAPE[2],), dtype=np.uint32)
        box[1:-1, 1:-1, :] = S.ramp_world()
        kw = dict(unknown_headroom=True, top=True)
        want2, counts2 = G.model_box(box, a2, 8, **kw)
        assert counts2.tolist() == [2 * 32 + 2 * 5, 150, 0, 0]
        seed_mm = np.array([[(a[0] + 1) * S.RES, (a[1] + 2) * S.RES, 0]])
        seed = np.array([[a[0] + 1, a[1] + 2, 0]])
        for unknown_occupied, clearance_m in ((True, 0.1), (False, 0.1), (True, 0.0)):
            cost = tm.ground_reach(seed_mm, robot_height_m=0.4, max_step_m=0.06, clearance_m=clearance_m, lo=a2, hi=b2, unknown_occupied=unknown_occupied, **kw)
            vox = 2 if clearance_m else 0
            d = G.bridge_model(want2, 307, vox + 1, unknown_occupied)[0]
            want_cost, _, reached = RM.field(d, a2, seed, clear_d2=vox * vox)
            assert np.array_equal(cost, want_cost) and tm.last_reach["reached"] == reached and tm.last_ground.tolist() == counts2.tolist(), (unknown_occupied, clearance_m)
            # with a clearance of two voxels the rim of sites takes the outer ring of the ramp's columns away
            assert reached == (28 * 3 if unknown_occupied and clearance_m else 150)
    finally:
        store.close()
