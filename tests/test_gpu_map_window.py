"""The sliding window -- box transfers and the map shift -- against the world model of tests/window_model.py (proved on the CPU
by tests/test_map_window_host.py): three routes (TSDFMapping.shift_map, shift_map_async, and the ws_shift_* C ABI driven from
here against the contract in include/warpsense_hip.h), the box kernels past one grid pass and past 4 GiB, even sizes, refusals.
Every comparison is np.array_equal."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from window_model import WALKS
import window_model as M
from window_routes import MW, MappingRoute, RES, RawRoute, TAU, _default, _i3, _p, _params, check_device, download, get_params, same_state, state
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu
WS_ERR_INVALID = -1


def make_route(name, size, w=None):
    if name == "raw":
        return RawRoute(w if w is not None else M.World(size, -np.asarray(size), np.asarray(size), _default()))
    return MappingRoute(size, asyn=(name == "async"))


# ------------------------------------------------------------------------------------------------ the walks through every route
@pytest.mark.parametrize("route", ["sync", "async", "raw"])
@pytest.mark.parametrize("size,seed", WALKS)
def test_walk_through_every_route(size, seed, route):
    walk = M.make_walk(size, seed)
    w0 = M.World(size, *M.walk_bounds(size, walk), _default())
    r = make_route(route, size, w0)
    w = M.run_walk(size, walk, seed, r, _default(), world=w0)
    r.finish(w)
    assert np.all(w.pos == 0) and np.count_nonzero(w.store != w.default_raw) > 0


def test_scans_between_shifts_equal_the_oracle_on_every_route():
    """real scans between the shifts: after every step each route == oracle_lib.update_tsdf on an OracleMap built from the model's
    window with the same pos and offset (so the three routes agree bit for bit); the result goes back into the model"""
    import torch
    import warpsense_amd as W
    size = (65, 65, 33)
    walk = [(5, -3, 2), (9, 1, 2), (-20, 10, -8), (-20, 10, -8), (5, -3, 2), (40, 40, 20), (0, 0, 0)]
    worlds = [M.World(size, *M.walk_bounds(size, walk), _default()) for _ in range(3)]
    routes = [make_route(name, size, w) for name, w in zip(("sync", "async", "raw"), worlds)]
    touched = 0
    for k, pos in enumerate(walk):
        # (the synthetic room is centred on the origin: the scan is taken there and moved to the window by whole voxels)
        pts = S.os1_128_scan(sensor_mm=(10.0, 7.0, 3.0), rings=16, azimuths=128, half_extents_mm=(1400.0, 1300.0, 700.0), seed=40 + k)
        pts = pts.astype(np.int64).astype(np.int32) + (np.asarray(pos, dtype=np.int32) * RES)[None, :]
        results = []
        for r, w in zip(routes, worlds):
            if tuple(w.pos) != tuple(pos):
                r.shift(w, pos)
                w.move(pos)
            oa = O.OracleMap(size, TAU, 0, pos=_i3(w.pos), offset=_i3(w.offset()), data=w.ring().copy())
            on = O.OracleMap(size, TAU, 0, pos=_i3(w.pos), offset=_i3(w.offset()))
            O.update_tsdf(oa, on, pts, list(pos), (0, 0, 32768), TAU, MW, RES)
            r.t.update_tsdf(torch.from_numpy(pts).cuda(), list(pos), (0, 0, 32768))
            w.set_ring(oa.data)
            check_device(r.t, w)
            results.append(download(r.t, 0, oa.data.size).data_)
            assert np.array_equal(results[-1], oa.data), (k, pos)
        assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
        touched += int(np.count_nonzero(results[0] != np.uint32(_default())))
    assert touched > 10_000  # the scans are in there
    for r, w in zip(routes, worlds):
        r.finish(w)


# ------------------------------------------------------------------------------------------------ past one grid pass, past 4 GiB
ONE_PASS = 4096 * 256  # lanes of one trip of the box kernels' grid-stride loop


def test_box_kernels_past_one_grid_pass():
    """129^3 (2 146 689 voxels) of arbitrary words, all three offsets rotated: whole-window and just-under / just-over-one-pass box
    transfers, and a shift whose leaving slab needs a second trip of the loop"""
    size, pos = (129, 129, 129), (40, -30, 17)
    rng = np.random.default_rng(129)
    w = M.World(size, np.asarray(pos) - 64, np.asarray(pos) + 64 + np.array([70, 0, 0]), _default())
    w.pos = np.asarray(pos, dtype=np.int64)
    lo, hi = w.window()
    w.write(lo, hi, M.draw_words(rng, 129 ** 3))
    assert np.all(w.offset() != 64) and np.all(w.offset() != 0)
    r = RawRoute(w)
    avg = r.t.avg_map()
    r.check(w)
    assert 129 ** 3 > 2 * ONE_PASS
    assert np.array_equal(avg.extract_box(lo, hi), w.box(lo, hi).reshape(-1))
    words = M.draw_words(rng, 129 ** 3)
    avg.insert_box(lo, hi, words)
    w.write(lo, hi, words)
    r.check(w)
    for ext in [(101, 101, 102), (103, 101, 101)]:  # 1 040 502 and 1 050 703 voxels
        n = int(np.prod(ext))
        assert all(e % 256 for e in ext) and n % 256 and abs(n - ONE_PASS) < 10_000
        a = lo + np.array([7, 11, 20])
        b = a + np.asarray(ext) - 1
        assert M.crosses_all_seams(size, pos, a, b)
        assert np.array_equal(avg.extract_box(a, b), w.box(a, b).reshape(-1))
        words = M.draw_words(rng, n)
        avg.insert_box(a, b, words)
        w.write(a, b, words)
        assert np.array_equal(avg.extract_box(a, b), words)
        r.check(w)
    assert 101 * 101 * 102 < ONE_PASS < 103 * 101 * 101
    new_pos = (pos[0] + 70, pos[1], pos[2])
    r.shift(w, new_pos, check_whole_entering=True)
    w.move(new_pos)
    assert r.slab_voxels == [70 * 129 * 129] and r.slab_voxels[0] > ONE_PASS
    r.check(w)
    r.finish(w)


def test_box_kernels_past_4_gib():
    """the 1025^3 device-only window (4.3 GB per map): world x lives in storage plane (x + 512) % 1025, so with pos x = 1024 the
    window's first plane x = 512 is the LAST storage plane (voxel indices up to 1025^3 - 1, byte offsets beyond 4 GiB) and x = 513
    is the first.  A byte offset that wrapped at 2^32 would land in storage planes 1 .. 3 (world x = 514 .. 516)."""
    import torch
    import warpsense_amd as W
    free, _ = torch.cuda.mem_get_info()
    if free / 2 ** 30 < 16:
        if os.environ.get("WS_ALLOW_BIG_SKIP") == "1":
            pytest.skip("needs ~16 GB on the GPU")
        pytest.fail("needs ~16 GB on the GPU (set WS_ALLOW_BIG_SKIP=1 to skip on this box)")
    size = (1025, 1025, 1025)
    pos = np.array([1024, -5, 3], dtype=np.int64)
    lm = W.LocalMap(*size, TAU, 0, host_voxels=False)
    lm.pos[:] = pos
    lm.offset[:] = M.model_offset(size, pos)
    tm = W.TSDFMapping(_params(size), lm)
    t, L = tm.tsdf(), tm.tsdf()._L
    avg = t.avg_map()
    lo, hi = M.window(size, pos)
    assert lo[0] == 512 and (lo[0] + 512) % 1025 == 1024 and (lo[0] + 1 + 512) % 1025 == 0
    rng = np.random.default_rng(4)
    fill = np.uint32(_default())
    low_a, low_b = (513, lo[1], lo[2]), (516, hi[1], hi[2])  # storage planes 0 .. 3
    low = M.draw_words(rng, 4 * 1025 * 1025)
    avg.insert_box(low_a, low_b, low)
    far_a, far_b = (512, lo[1], lo[2]), (512, hi[1], hi[2])  # the last storage plane, whole: the last voxel of the allocation too
    far = M.draw_words(rng, 1025 * 1025)
    assert 1025 * 1025 > ONE_PASS and 1024 * 1025 * 1025 * 4 > 2 ** 32
    avg.insert_box(far_a, far_b, far)
    assert np.array_equal(avg.extract_box(far_a, far_b), far)
    assert np.array_equal(avg.extract_box(low_a, low_b), low)
    # a small box around the very last voxel (storage 1024, 1024, 1024), across the y and z seams
    y_last, z_last = int(lo[1] + (1024 - (lo[1] + 512)) % 1025), int(lo[2] + (1024 - (lo[2] + 512)) % 1025)
    assert lo[1] < y_last < hi[1] and lo[2] < z_last < hi[2]
    a, b = (512, y_last - 2, z_last - 2), (512, y_last + 2, z_last + 2)
    want = far.reshape(1025, 1025)[y_last - 2 - lo[1]:y_last + 3 - lo[1], z_last - 2 - lo[2]:z_last + 3 - lo[2]]
    assert np.array_equal(avg.extract_box(a, b), want.reshape(-1))
    # the raw shift by 2 voxels: x = 512, 513 leave (the last and the first storage plane), x = 1537, 1538 enter
    new_pos = pos + np.array([2, 0, 0])
    exp = M.expected_slabs(size, pos, new_pos)
    assert len(exp) == 1 and exp[0]["leave"][0][0] == 512 and exp[0]["leave"][1][0] == 513
    ticket = C.c_void_p()
    assert L.ws_shift_begin(t.handle, _p(_i3(new_pos)), int(fill), C.byref(ticket)) == 0, L.ws_last_error()
    try:
        assert L.ws_shift_count(ticket) == 1
        blo, bhi = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
        assert L.ws_shift_entering(ticket, 0, _p(blo), _p(bhi)) == 0
        assert np.array_equal(blo, exp[0]["enter"][0]) and np.array_equal(bhi, exp[0]["enter"][1])
        assert L.ws_shift_wait(ticket) == 0
        data = C.c_void_p()
        assert L.ws_shift_slab(ticket, 0, _p(blo), _p(bhi), C.byref(data)) == 0
        assert np.array_equal(blo, exp[0]["leave"][0]) and np.array_equal(bhi, exp[0]["leave"][1])
        got = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint32)), shape=(2 * 1025 * 1025,)).copy()
    finally:
        assert L.ws_shift_end(ticket) == 0
    assert np.array_equal(got[:1025 * 1025], far)
    assert np.array_equal(got[1025 * 1025:], low[:1025 * 1025])
    for which in (0, 1):
        _, p1, o1 = get_params(t, which)
        assert np.array_equal(p1, new_pos) and np.array_equal(o1, M.model_offset(size, new_pos))
    assert np.all(avg.extract_box(*exp[0]["enter"]) == fill)
    assert np.array_equal(avg.extract_box((514, lo[1], lo[2]), low_b), low[1025 * 1025:])  # and the planes next to them are as they were


# ------------------------------------------------------------------------------------------------ even sizes
def even_world():
    size, pos = (16, 18, 20), (3, -2, 5)
    w = M.World(size, np.asarray(pos) - 3 * np.asarray(size), np.asarray(pos) + 3 * np.asarray(size), _default())
    w.pos = np.asarray(pos, dtype=np.int64)
    lo, hi = w.window()
    w.write(lo, hi, M.draw_words(np.random.default_rng(16), 16 * 18 * 20))
    assert np.all(w.offset() != np.asarray(size) // 2) and np.all(w.offset() != 0)  # rotated
    return size, pos, w


def test_even_sizes_box_transfers():
    """LocalMap forces odd sizes, the C ABI does not.  The window of an even size is pos - size/2 .. pos + size/2 - 1 (every ring cell
    once); a box with more voxels along an axis than the ring has cells is refused and nothing moves."""
    import warpsense_amd as W
    size, pos, w = even_world()
    r = RawRoute(w)
    avg = r.t.avg_map()
    lo, hi = w.window()
    assert np.array_equal(hi - lo + 1, size)
    assert np.array_equal(avg.extract_box(lo, hi), w.box(lo, hi).reshape(-1))
    words = M.draw_words(np.random.default_rng(17), 16 * 18 * 20)
    avg.insert_box(lo, hi, words)
    w.write(lo, hi, words)
    r.check(w)
    before = state(r.t, r.n)
    for axis in (0, 1, 2, None):
        wide = hi.copy()
        if axis is None:
            wide += 1
        else:
            wide[axis] += 1  # pos + size/2: within size/2 of pos, but the ring cell of lo again
        n = int(np.prod(wide - lo + 1))
        with pytest.raises(W.WsError):
            avg.extract_box(lo, wide)
        with pytest.raises(W.WsError):
            avg.insert_box(lo, wide, np.zeros(n, dtype=np.uint32))
        assert same_state(before, state(r.t, r.n))
    r.check(w)


def test_even_sizes_shift():
    """ws_shift_begin on an even-sized map moves the each-cell-once window: slabs and entering boxes as the model computes them (no
    wider than the ring), and the walk invariant over a walk that holds |d| = size on every axis"""
    size, pos, w = even_world()
    r = RawRoute(w)
    walk = [tuple(int(v) for v in np.asarray(p) + np.asarray(pos)) for p in M.make_walk(size, 18, diagonals=2)]
    steps = np.abs(np.diff(np.asarray([pos] + walk), axis=0))
    assert all(np.any(steps[:, k] == size[k]) for k in range(3)) and np.all(steps <= np.asarray(size))
    M.run_walk(size, walk, 18, r, _default(), world=w)
    r.finish(w)
    assert tuple(w.pos) == pos


# ------------------------------------------------------------------------------------------------ refusals and state
def small_world(seed=21):
    size, pos = (21, 17, 13), (4, -5, 3)
    w = M.World(size, np.asarray(pos) - 3 * np.asarray(size), np.asarray(pos) + 3 * np.asarray(size), _default())
    w.pos = np.asarray(pos, dtype=np.int64)
    lo, hi = w.window()
    w.write(lo, hi, M.draw_words(np.random.default_rng(seed), 21 * 17 * 13))
    return size, pos, w


def test_refusals_leave_both_maps_untouched():
    """every refusal is a host-side argument check (WS_ERR_INVALID before any launch): parameters and data of both maps stay as they
    were, and the next valid shift gives the model's window"""
    import torch
    import warpsense_amd as W
    size, pos, w = small_world()
    r = RawRoute(w)
    t, L, avg, new = r.t, r.L, r.t.avg_map(), r.t.new_map()
    before = state(t, r.n)

    def refused(rc_ticket):
        rc, ticket = rc_ticket
        assert rc == WS_ERR_INVALID and not ticket.value
        assert same_state(before, state(t, r.n))

    # a ticket is open
    step = (pos[0] + 2, pos[1], pos[2] - 1)
    rc, open_ticket = r.begin(pos)  # (a zero move: a ticket like any other)
    assert rc == 0
    refused(r.begin(step))
    assert L.ws_shift_reserve(t.handle, 1 << 20) == WS_ERR_INVALID
    assert same_state(before, state(t, r.n))
    assert L.ws_shift_end(open_ticket) == 0
    # larger than the window, per axis and in both directions
    for axis in range(3):
        for sign in (1, -1):
            far = list(pos)
            far[axis] += sign * (size[axis] + 1)
            refused(r.begin(far))
    # new_map not default
    lo, hi = w.window()
    new.insert_box(lo, lo, np.array([12345], dtype=np.uint32))
    before = state(t, r.n)
    refused(r.begin(step))
    new.to_device(W.DeviceMap(_i3(w.size), _i3(w.offset()), np.full(r.n, _default(), dtype=np.uint32), _i3(w.pos)))
    before = state(t, r.n)
    # boxes: outside the window, hi < lo, which out of range
    for a, b in [((lo[0] - 1, lo[1], lo[2]), tuple(hi)), (tuple(lo), (hi[0], hi[1] + 1, hi[2])), ((lo[0], lo[1], hi[2] + 1), (hi[0], hi[1], hi[2] + 1))]:
        n = int(np.prod(np.asarray(b) - np.asarray(a) + 1))
        with pytest.raises(W.WsError):
            avg.extract_box(a, b)
        with pytest.raises(W.WsError):
            avg.insert_box(a, b, np.zeros(n, dtype=np.uint32))
    buf = np.zeros(21 * 17 * 13, dtype=np.uint32)
    a, b = _i3((lo[0] + 3, lo[1], lo[2])), _i3((lo[0] + 2, hi[1], hi[2]))  # hi < lo (through the C ABI: the wrapper sizes its buffer first)
    assert L.ws_map_extract_box(t.handle, 0, _p(a), _p(b), _p(buf)) == WS_ERR_INVALID
    assert L.ws_map_insert_box(t.handle, 0, _p(a), _p(b), _p(buf)) == WS_ERR_INVALID
    for which in (-1, 2):
        assert L.ws_map_extract_box(t.handle, which, _p(_i3(lo)), _p(_i3(lo)), _p(buf)) == WS_ERR_INVALID
        assert L.ws_map_insert_box(t.handle, which, _p(_i3(lo)), _p(_i3(lo)), _p(buf)) == WS_ERR_INVALID
    assert same_state(before, state(t, r.n))
    # a valid shift now: the model's window
    r.shift(w, step)
    w.move(step)
    r.check(w)
    # between scatter and integrate: refused; after the integrate: accepted
    pts = S.os1_128_scan(sensor_mm=(10.0, 7.0, 3.0), rings=8, azimuths=64, half_extents_mm=(400.0, 350.0, 250.0), seed=6)
    pts = pts.astype(np.int64).astype(np.int32) + (np.asarray(step, dtype=np.int32) * RES)[None, :]
    t.scatter(torch.from_numpy(pts).cuda(), list(step), (0, 0, 32768))
    before = state(t, r.n)
    assert np.count_nonzero(before[3] != np.uint32(_default())) > 0  # the scan is in new_map
    refused(r.begin(pos))
    t.integrate()
    w.set_ring(download(t, 0, r.n).data_)
    r.shift(w, pos)
    w.move(pos)
    r.check(w)
    r.finish(w)


def test_zero_move_and_staging():
    """new_pos == pos: a ticket without slabs that ends cleanly and moves nothing.  A walk is bit-identical with the staging
    pre-allocated (ws_shift_reserve, TSDFMapping.reserve_shift) and grown inside the shifts (a small step first, larger ones after)."""
    size, pos, w = small_world(seed=22)
    r = RawRoute(w)
    before = state(r.t, r.n)
    rc, ticket = r.begin(pos)
    assert rc == 0 and ticket.value and r.L.ws_shift_count(ticket) == 0
    a, b = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    data = C.c_void_p()
    assert r.L.ws_shift_entering(ticket, 0, _p(a), _p(b)) == WS_ERR_INVALID
    assert r.L.ws_shift_wait(ticket) == 0
    assert r.L.ws_shift_slab(ticket, 0, _p(a), _p(b), C.byref(data)) == WS_ERR_INVALID
    assert r.L.ws_shift_end(ticket) == 0
    assert same_state(before, state(r.t, r.n))
    walk = [(5, -5, 3), (5, -5, 3), (12, 3, 3), (-9, -14, 16), (4, -5, 3)]  # 1 voxel, nothing, then more per shift than before
    finals = []
    for reserve in (False, True):
        _, _, w2 = small_world(seed=22)
        r2 = RawRoute(w2)
        if reserve:
            assert r2.L.ws_shift_reserve(r2.t.handle, 3 * 21 * 17 * 13) == 0
        M.run_walk(size, walk, 23, r2, _default(), world=w2)
        r2.finish(w2)
        finals.append((download(r2.t, 0, r2.n).data_, r2.store.copy(), list(r2.slab_voxels)))
    assert np.array_equal(finals[0][0], finals[1][0]) and np.array_equal(finals[0][1], finals[1][1])
    assert finals[0][2] == finals[1][2] and max(finals[0][2][1:]) > finals[0][2][0]  # the staging had to grow after the first shift
    # TSDFMapping.reserve_shift in front of an asynchronous walk
    wsize, seed = WALKS[0]
    walk = M.make_walk(wsize, seed)[:12]
    r3 = MappingRoute(wsize, asyn=True, reserve=4)
    w3 = M.run_walk(wsize, walk, seed, r3, _default())
    r3.finish(w3)


def test_new_map_box_round_trips():
    """which = WS_MAP_NEW: box transfers across the seams of new_map, independent entries in both maps"""
    import warpsense_amd as W
    size, pos, w = small_world(seed=31)
    r = RawRoute(w)
    lo, hi = w.window()
    rng = np.random.default_rng(32)
    wn = M.World(size, w.bb_lo, w.bb_hi, _default())  # a model of new_map
    wn.pos = w.pos.copy()
    wn.write(lo, hi, M.draw_words(rng, r.n))
    r.t.new_map().to_device(W.DeviceMap(_i3(size), _i3(w.offset()), wn.ring(), _i3(pos)))
    new, avg = r.t.new_map(), r.t.avg_map()
    seam = 0
    for a, b in M.draw_boxes(size, pos, rng, count=6) + [(lo, hi)]:
        seam += M.crosses_all_seams(size, pos, a, b)
        assert np.array_equal(new.extract_box(a, b), wn.box(a, b).reshape(-1))
        assert np.array_equal(avg.extract_box(a, b), w.box(a, b).reshape(-1))
        words = M.draw_words(rng, np.prod(b - a + 1))
        new.insert_box(a, b, words)
        wn.write(a, b, words)
        assert np.array_equal(download(r.t, 1, r.n).data_, wn.ring())
        assert np.array_equal(download(r.t, 0, r.n).data_, w.ring())
    assert seam >= 2


# ------------------------------------------------------------------------------------------------ partial write-back
WB_BOXES = [((50, -20, -2), (70, 3, 40)),                 # cuts chunks in all three axes (x = 64, y = 0, z = 0 run through it)
            ((60, -70, 10), (90, -40, 12)),               # half outside the window
            ((-1000, -1000, -1000), (1000, 1000, 1000))]  # larger than the window: clipped to it


def _write_back_case(global_map, read_chunks, boxes=WB_BOXES):
    import warpsense_amd as W
    size, pos = (71, 61, 67), (40, -25, 30)
    lm = W.LocalMap(*size, TAU, 0, global_map)
    tm = W.TSDFMapping(_params(size), lm)
    w = M.World(size, np.asarray(pos) - 80, np.asarray(pos) + 80, _default())
    rng = np.random.default_rng(71)
    lo, hi = w.window()
    words = M.draw_words(rng, np.prod(size))
    tm.tsdf().avg_map().insert_box(lo, hi, words)
    w.write(lo, hi, words)
    tm.shift_map(pos)  # a part of the words is in the global map now, the window is rotated
    w.move(pos)
    lo, hi = w.window()
    words = M.draw_words(rng, np.prod(size))
    tm.tsdf().avg_map().insert_box(lo, hi, words)
    w.write(lo, hi, words)
    for a, b in boxes:
        it = M.box_inter(np.asarray(a), np.asarray(b), lo, hi)
        assert it is not None
        assert np.any(it[0] // 64 != it[1] // 64)
        tm.write_back(a, b)
        w.store[w.sl(*it)] = w.world[w.sl(*it)]  # inside the box the window; outside what it held before
        w.check_chunks(read_chunks(lm.map_))
    check_device(tm.tsdf(), w)
    a, b = WB_BOXES[0]
    assert all(a[k] // 64 != b[k] // 64 for k in range(3))
    return tm, w


def test_partial_write_back_in_memory():
    import warpsense_amd as W
    tm, w = _write_back_case(W.GlobalMap(TAU, 0), lambda g: g.chunks)
    tm.write_back()
    lo, hi = w.window()
    w.store[w.sl(lo, hi)] = w.world[w.sl(lo, hi)]
    w.check_chunks(tm.local_map_.map_.chunks)


def test_partial_write_back_h5(tmp_path):
    from warpsense_amd import build
    if build.find_hdf5() is None or build.build_h5() is None:
        pytest.skip("no HDF5 C library on this box")
    import warpsense_amd as W
    path = str(tmp_path / "partial.h5")

    def read_chunks(g):
        # what the FILE holds after write_back (every active chunk was written): closed and opened again
        g.close()
        g2 = W.GlobalMap(TAU, 0, filename=path, open_existing=True)
        out = {key: g2.activate_chunk(*key).copy() for key in sorted(g2._in_file)}
        g2._H.ws_h5_close(g2._file)
        g2._file = None
        return out

    _write_back_case(W.GlobalMap(TAU, 0, filename=path, map_params=_params((71, 61, 67)).map), read_chunks, boxes=WB_BOXES[:1])


# ------------------------------------------------------------------------------------------------ a repeated scan, then the window
def _repeated_scan_setup():
    """the software path of test_gpu_tsdf.py::test_a_scan_that_runs_out_of_chunks_is_aborted_and_repeated: a record pool too small
    for the scan, which the library repeats with a larger one"""
    import warpsense_amd as W
    tau, res, size = 600, 20, (401, 401, 101)
    lm = W.LocalMap(*size, tau, 0)
    tm = W.TSDFMapping(_params(size, res=res, tau=tau), lm)
    t = tm.tsdf()
    t.debug_chunk_policy(1, 9)
    t.set_capacity(4096 * 256)
    far = S.os1_128_scan(sensor_mm=(130.0, -70.0, 40.0), rings=128, azimuths=512, half_extents_mm=(3800.0, 3600.0, 900.0), seed=11)
    oa = O.OracleMap(size, tau, 0)
    O.update_tsdf(oa, oa.copy(), far, (6, -4, 2), (0, 0, 32768), tau, MW, res)
    new_pos = (150, -120, 30)
    w = M.World(size, *M.walk_bounds(size, [new_pos]), int(W.pack_entry(tau, 0)))
    w.set_ring(oa.data)
    return tm, t, far, w, new_pos


def test_shift_right_after_a_repeated_scan():
    """shift_map_async straight after a scan that has to be repeated: the slabs hold the repeated scan's voxels (WS_SETTLE in
    ws_shift_begin)"""
    import torch
    tm, t, far, w, new_pos = _repeated_scan_setup()
    cap0 = t.stats()["record_capacity"]
    tm.update_tsdf(torch.from_numpy(far).cuda(), pos_rm=(6, -4, 2), up_rm=(0, 0, 32768))
    tm.shift_map_async(new_pos)  # nothing in between
    w.move(new_pos)
    tm.wait_shift()
    st = t.stats()
    assert st["status"] == 0 and st["error_flags"] == 0 and st["record_capacity"] > cap0, "the scan must have outgrown its pool"
    assert np.count_nonzero(w.store != w.default_raw) > 100_000  # the scan is in the slabs
    w.check_chunks(tm.local_map_.map_.chunks)
    got = download(t, 0, int(np.prod(w.size)))
    assert np.array_equal(got.pos_, w.pos) and np.array_equal(got.offset_, w.offset()) and np.array_equal(got.data_, w.ring())


def test_extract_box_right_after_a_repeated_scan():
    """the same with ws_map_extract_box (WS_SETTLE there)"""
    import torch
    tm, t, far, w, _ = _repeated_scan_setup()
    cap0 = t.stats()["record_capacity"]
    tm.update_tsdf(torch.from_numpy(far).cuda(), pos_rm=(6, -4, 2), up_rm=(0, 0, 32768))
    lo, hi = w.window()
    box = t.avg_map().extract_box(lo, hi)  # nothing in between
    st = t.stats()
    assert st["status"] == 0 and st["error_flags"] == 0 and st["record_capacity"] > cap0, "the scan must have outgrown its pool"
    assert np.array_equal(box, w.box(lo, hi).reshape(-1))
    assert np.count_nonzero(box != w.default_raw) > 100_000
