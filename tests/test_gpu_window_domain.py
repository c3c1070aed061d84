"""The sliding window and the chunk store far from the origin and past the first size of their tables, against the world model of
tests/window_model.py (held to LocalMap.shift at the same bases by tests/test_window_domain_host.py): the walks of
test_gpu_map_window.py / test_gpu_store.py from bases whose windows touch both ends of int32, raw boxes and a write-back there,
refusals that change nothing, slot tables of more than 8192 words, a box of more chunks than one grid pass, and the ring of eight
tables wrapped without a wait in between.  Every comparison is np.array_equal / torch.equal.

The rule the refusals enforce (include/warpsense_hip.h): a window pos - size/2 .. pos - size/2 + size - 1 lies in int32
on every axis, and so does every window of a shift's plan; else WS_ERR_RANGE before anything is allocated or launched."""
import ctypes as C
import os

import numpy as np
import pytest

from edge_domain_scenes import BOTTOM_KEY, TOP_KEY
from window_model import I32_MAX, I32_MIN, WALKS
import window_model as M
from window_routes import MW, RES, TAU, MappingRoute, RawRoute, _default, _i3, _p, _params, check_device, same_state, state
from window_routes import CW, StoreRoute, chunk_box, same_store, store_state

pytestmark = pytest.mark.gpu

WS_ERR_INVALID, WS_ERR_RANGE = -1, -5


def _sync():
    import torch
    import warpsense_amd as W
    W.Context.default().sync()
    torch.cuda.synchronize()


def _last_error(L):
    return (L.ws_last_error() or b"").decode()


# ------------------------------------------------------------------------------------------------ a. walks from far bases
def make_far_route(route, size, base, w):
    if route == "raw":
        return RawRoute(w)  # (its device map is created from the model's window: pos = base)
    if route.startswith("store"):
        return StoreRoute(size, segment_chunks=2 if route == "store2" else 0, base=base)
    return MappingRoute(size, asyn=(route == "async"), base=base)


def route_chunks(r, route):
    """the chunks a route has filed, by key (the raw route keeps a dense array instead: None)"""
    if route == "raw":
        return None
    return r.chunks() if route.startswith("store") else dict(r.lm.map_.chunks)


_NEAR, _FAR_HOST = {}, {}


def near_walk(size, seed):
    """the walk from the origin through the synchronous host route, once: (final ring download, chunks by key)"""
    if (size, seed) not in _NEAR:
        r = MappingRoute(size, asyn=False)
        w = M.run_walk(size, M.make_walk(size, seed), seed, r, _default(), check_every=False)
        r.finish(w)
        _NEAR[(size, seed)] = (state(r.t, int(np.prod(size)))[2].copy(), {k: v.copy() for k, v in r.lm.map_.chunks.items()})
    return _NEAR[(size, seed)]


def far_host_walk(size, seed, name):
    """the walk from the base `name` through the synchronous host route, once: its chunks by key"""
    if (size, seed, name) not in _FAR_HOST:
        base = M.far_bases(size, seed)[name]
        r = MappingRoute(size, asyn=False, base=base)
        w = M.run_walk(size, M.make_walk(size, seed, base=base), seed, r, _default(), check_every=False, base=base)
        r.finish(w)
        _FAR_HOST[(size, seed, name)] = {k: v.copy() for k, v in r.lm.map_.chunks.items()}
    return _FAR_HOST[(size, seed, name)]


FAR_CASES = [(size, seed, route) for size, seed in WALKS for route in ("sync", "async", "raw", "store", "store2")
             if route != "store2" or size == (71, 61, 67)]


@pytest.mark.parametrize("name", ["aligned+-+", "aligned-+-", "touching"])
@pytest.mark.parametrize("size,seed,route", FAR_CASES)
def test_walk_from_a_far_base(size, seed, route, name):
    base = M.far_bases(size, seed)[name]
    walk = M.make_walk(size, seed, base=base)
    w0 = M.World(size, *M.walk_bounds(size, walk, base), _default(), pos=base)
    assert M.fits_int32(w0.bb_lo, w0.bb_hi)
    r = make_far_route(route, size, base, w0)
    w = M.run_walk(size, walk, seed, r, _default(), world=w0)  # the model after every step
    r.finish(w)
    assert np.array_equal(w.pos, base) and np.count_nonzero(w.store != w.default_raw) > 0
    chunks = route_chunks(r, route)
    if route.startswith("store"):  # key set and bytes of the synchronous host route at the same base
        host = far_host_walk(size, seed, name)
        assert sorted(chunks) == sorted(host) and r.store.keys() == sorted(host)
        for key in host:
            assert np.array_equal(chunks[key], host[key]), key
        if route == "store2":
            assert r.store.capacity() >= r.store.count() > 2 and r.store.capacity() % 2 == 0  # more than one segment
    if name == "touching":
        wins = [M.window(size, p) for p in walk]
        assert any(x[1][0] == I32_MAX for x in wins) and any(x[0][1] == I32_MIN for x in wins)  # windows that hold either voxel
        if chunks is not None:
            assert max(k[0] for k in chunks) == TOP_KEY and min(k[1] for k in chunks) == BOTTOM_KEY
        return
    # aligned: ring offsets and chunk alignment are those of the walk from the origin, so are the bytes
    ring, near = near_walk(size, seed)
    assert np.array_equal(state(r.t, int(np.prod(size)))[2], ring)
    if chunks is not None:
        move = np.asarray(base) // 64
        assert sorted(chunks) == sorted(tuple(int(v) for v in np.asarray(k) + move) for k in near)
        for k, c in near.items():
            assert np.array_equal(chunks[tuple(int(v) for v in np.asarray(k) + move)], c), k


# ------------------------------------------------------------------------------------------------ b. raw boxes at the edge
def edge_pos(size, kind):
    """a window position at the edge of int32: `max` touches INT32_MAX on every axis, `min` INT32_MIN, `mixed` INT32_MAX on x,
    INT32_MIN on y and lies near 2^30 + 37 on z.  An axis whose ring would not be rotated there lies one voxel further in (the
    seam of that axis must run through the window for the first box to cross it)."""
    s = np.asarray(size, dtype=np.int64)
    top, bottom = I32_MAX - (s - 1 - s // 2), I32_MIN + s // 2
    pos = {"max": top, "min": bottom, "mixed": np.array([top[0], bottom[1], 2 ** 30 + 37])}[kind].copy()
    pos = np.where(M.model_offset(s, pos) == 0, pos - np.sign(pos), pos)
    lo, hi = M.window(s, pos)
    assert M.fits_int32(lo, hi) and np.all(M.model_offset(s, pos) != 0)
    touch = {"max": hi == I32_MAX, "min": lo == I32_MIN, "mixed": np.array([hi[0] == I32_MAX, lo[1] == I32_MIN, True])}[kind]
    assert touch.sum() >= 2, (size, kind, pos)  # (at most one axis had to give way)
    return pos


def far_world(size, pos, seed):
    s = np.asarray(size, dtype=np.int64)
    w = M.World(size, pos - 2 * s, pos + 2 * s, _default(), pos=pos)  # (the model's own box may leave int32: it is int64)
    lo, hi = w.window()
    w.write(lo, hi, M.draw_words(np.random.default_rng(seed), np.prod(s)))
    return w


@pytest.mark.parametrize("kind", ["max", "min", "mixed"])
@pytest.mark.parametrize("size", [(71, 61, 67), (16, 18, 20), (70, 66, 130)])
def test_boxes_at_the_edge(size, kind):
    """test_gpu_store.py::test_save_box_and_load_box where the window touches the ends of int32, with extract_box / insert_box
    round trips on the same boxes"""
    import warpsense_amd as W
    fill = np.uint32(_default())
    pos = edge_pos(size, kind)
    w = far_world(size, pos, 5)
    r = RawRoute(w)
    avg = r.t.avg_map()
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    rng = np.random.default_rng(6)
    boxes = M.draw_boxes(size, pos, rng, count=3)
    assert M.crosses_all_seams(size, pos, *boxes[0])
    model = {}  # key -> (64, 64, 64): what the store must hold
    for a, b in boxes:
        assert np.array_equal(avg.extract_box(a, b), w.box(a, b).reshape(-1))
        words = M.draw_words(rng, np.prod(b - a + 1))
        avg.insert_box(a, b, words)
        w.write(a, b, words)
        assert np.array_equal(avg.extract_box(a, b), words)
        store.save_box(r.t, a, b)
        for key in [tuple(int(v) for v in k) for k in W.chunks_of_box(a, b)]:
            c = model.setdefault(key, np.full((64, 64, 64), fill, dtype=np.uint32))
            sl, ia, ib = chunk_box(key, a, b)
            c[sl] = w.box(ia, ib)
        assert store.keys() == sorted(model)
        for key, c in model.items():
            assert np.array_equal(store.chunk(key).reshape(64, 64, 64), c), (key, a, b)  # fill outside, earlier saves kept
        check_device(r.t, w)  # a save leaves the ring alone
    ks = np.asarray(sorted(model))
    if kind != "min":
        assert ks[:, 0].max() <= TOP_KEY and ks[:, 0].max() >= TOP_KEY - 2
    if kind != "max":
        assert ks[:, 1].min() >= BOTTOM_KEY and ks[:, 1].min() <= BOTTOM_KEY + 2
    # load: the whole window.  Present chunks give their voxels, everything else becomes fill; no chunk appears
    n_before = store.count()
    lo, hi = w.window()
    want = np.full(tuple(int(v) for v in w.size), fill, dtype=np.uint32)
    for key, c in model.items():
        sl, ia, ib = chunk_box(key, lo, hi)
        want[tuple(slice(int(ia[k] - lo[k]), int(ib[k] - lo[k]) + 1) for k in range(3))] = c[sl]
    assert np.count_nonzero(want != fill) > 0 and np.count_nonzero(want == fill) > 0
    store.load_box(r.t, lo, hi)
    w.write(lo, hi, want)
    check_device(r.t, w)
    assert store.count() == n_before
    # a load over space the store has never seen, across the seams: fill, and still no chunk
    empty = W.DeviceGlobalMap(TAU, 0)
    words = M.draw_words(rng, np.prod(size))
    avg.insert_box(lo, hi, words)
    w.write(lo, hi, words)
    a, b = boxes[0]
    empty.load_box(r.t, a, b)
    w.write(a, b, np.full(int(np.prod(b - a + 1)), fill, dtype=np.uint32))
    check_device(r.t, w)
    assert empty.count() == 0 and empty.keys() == []
    # the whole window out and in again through the box transfers
    assert np.array_equal(avg.extract_box(lo, hi), w.box(lo, hi).reshape(-1))
    # boxes outside the window (where such a box can be named in int32 at all) or wrapping onto themselves: refused, nothing moves
    before, sbefore = state(r.t, r.n), store_state(store)
    bad = [((lo[0] - 1, lo[1], lo[2]), tuple(hi)), (tuple(lo), (hi[0], hi[1], hi[2] + 1)), (tuple(lo), (hi[0] + 1, hi[1], hi[2])),
           ((lo[0], lo[1] - 1, lo[2]), tuple(hi)), ((lo[0] + 2, lo[1], lo[2]), (lo[0] + 1, hi[1], hi[2]))]
    bad = [(a2, b2) for a2, b2 in bad if M.fits_int32(a2, b2)]
    assert len(bad) >= 3
    buf = np.zeros(int(np.prod(np.asarray(size) + 1)), dtype=np.uint32)
    for a2, b2 in bad:
        for f in (r.L.ws_store_save_box, r.L.ws_store_load_box):
            assert f(store.handle, r.t.handle, 0, _p(_i3(a2)), _p(_i3(b2))) == WS_ERR_INVALID
        assert r.L.ws_map_extract_box(r.t.handle, 0, _p(_i3(a2)), _p(_i3(b2)), _p(buf)) == WS_ERR_INVALID
        assert r.L.ws_map_insert_box(r.t.handle, 0, _p(_i3(a2)), _p(_i3(b2)), _p(buf)) == WS_ERR_INVALID
    assert same_state(before, state(r.t, r.n)) and same_store(sbefore, store_state(store))


def test_write_back_into_a_file_at_the_edge(tmp_path):
    """write_back through the store into an .h5 file with chunk keys 2^25 - 1 and -2^25 in their names, read back from the file"""
    from warpsense_amd import build
    if build.find_hdf5() is None or build.build_h5() is None:
        pytest.skip("no HDF5 C library on this box")
    import warpsense_amd as W
    size = (71, 61, 67)
    pos = edge_pos(size, "mixed")
    path = str(tmp_path / "edge.h5")
    g = W.GlobalMap(TAU, 0, filename=path, map_params=_params(size).map)
    lm = W.LocalMap(*size, TAU, 0, g)
    lm.pos[:] = pos
    lm.offset[:] = M.model_offset(size, pos)
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
    w = far_world(size, pos, 71)
    lo, hi = w.window()
    tm.tsdf().avg_map().insert_box(lo, hi, w.box(lo, hi).reshape(-1))
    tm.write_back()
    w.store[w.sl(lo, hi)] = w.world[w.sl(lo, hi)]
    check_device(tm.tsdf(), w)
    g.close()
    g2 = W.GlobalMap(TAU, 0, filename=path, open_existing=True)
    chunks = {key: g2.activate_chunk(*key).copy() for key in sorted(g2._in_file)}
    g2._H.ws_h5_close(g2._file)
    g2._file = None
    assert sorted(chunks) == store.keys() == [tuple(int(v) for v in k) for k in W.chunks_of_box(lo, hi)]
    assert max(k[0] for k in chunks) == TOP_KEY and min(k[1] for k in chunks) == BOTTOM_KEY and len(chunks) == 4  # x 2, y 1, z 2
    w.check_chunks(chunks)
    for key, c in chunks.items():
        assert np.array_equal(store.chunk(key), c), key


# ------------------------------------------------------------------------------------------------ c. refusals that change nothing
def test_shifts_out_of_int32_are_refused_and_change_nothing():
    """a window that touches INT32_MAX on x and INT32_MIN on y, and new positions one voxel too far: WS_ERR_RANGE in the entry
    point's name from ws_shift_begin, ws_shift_device and (through ws_shift_plan) TSDFMapping.shift_map; both maps, the store and
    its directory are as they were, and the valid shift made afterwards gives the model's bytes"""
    import warpsense_amd as W
    size = (21, 17, 13)
    s = np.asarray(size, dtype=np.int64)
    pos = np.array([I32_MAX - (s[0] - 1 - s[0] // 2), I32_MIN + s[1] // 2, 2 ** 30 + 37], dtype=np.int64)
    lo, hi = M.window(size, pos)
    assert hi[0] == I32_MAX and lo[1] == I32_MIN
    too_far = [pos + d for d in ([1, 0, 0], [0, -1, 0], [1, -1, 0], [1, 0, 5], [-3, -1, 2], [0, -1, -13])]
    valid = pos + np.array([-2, 3, -1])
    seed_key, seed_words = (5, 5, 5), M.draw_words(np.random.default_rng(3), CW)
    for use_store in (False, True):
        w = M.World(size, pos - 3 * s, pos + 3 * s, _default(), pos=pos)
        w.write(lo, hi, M.draw_words(np.random.default_rng(21), np.prod(s)))
        r = RawRoute(w)
        store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
        store.put_chunk(seed_key, seed_words)
        before, sbefore = state(r.t, r.n), (store_state(store), store.count(), store.capacity())
        for new_pos in too_far:
            assert M.fits_int32(new_pos, new_pos) and not M.fits_int32(*M.window(size, new_pos))
            if use_store:
                assert r.L.ws_shift_device(r.t.handle, store.handle, _p(_i3(new_pos))) == WS_ERR_RANGE, _last_error(r.L)
                assert _last_error(r.L).startswith("ws_shift_device")
            else:
                rc, ticket = r.begin(new_pos)
                assert rc == WS_ERR_RANGE and not ticket.value, _last_error(r.L)
                assert _last_error(r.L).startswith("ws_shift_begin")
            assert same_state(before, state(r.t, r.n))
            after = (store_state(store), store.count(), store.capacity())
            assert same_store(sbefore[0], after[0]) and sbefore[1:] == after[1:]
        if use_store:
            assert r.L.ws_shift_device(r.t.handle, store.handle, _p(_i3(valid))) == 0, _last_error(r.L)
            w.move(valid)
            r.check(w)
            chunks = {k: store.chunk(k) for k in store.keys() if k != seed_key}
            w.check_chunks(chunks)
            assert np.array_equal(store.chunk(seed_key), seed_words) and len(chunks) >= 1
        else:
            r.shift(w, valid)
            w.move(valid)
            r.check(w)
            r.finish(w)
    # the synchronous route plans before it moves anything, the asynchronous one begins with ws_shift_begin
    for asyn in (False, True):
        mr = MappingRoute(size, asyn=asyn, base=pos)
        w = M.World(size, pos - 3 * s, pos + 3 * s, _default(), pos=pos)
        words = M.draw_words(np.random.default_rng(22), np.prod(s))
        mr.insert(lo, hi, words)
        w.write(lo, hi, words)
        before = state(mr.t, int(np.prod(s)))
        for new_pos in too_far:
            with pytest.raises(W.WsError, match="status -5"):
                mr.shift(w, new_pos)
            mr.tm.wait_shift()
            assert same_state(before, state(mr.t, int(np.prod(s)))) and not mr.lm.map_.chunks
            mr.check(w)
        mr.shift(w, valid)
        w.move(valid)
        mr.check(w)
        mr.finish(w)


def test_a_window_at_the_top_edge_does_not_hold_int32_min():
    """an even size s at pos = INT32_MAX - s/2 + 1: the window fits, its last voxel is INT32_MAX.  INT32_MIN - pos wraps to s/2 in 32
    bits, which is "within size/2 of pos": the voxel INT32_MIN is refused by all four box calls, and nothing moves"""
    import warpsense_amd as W
    size = (16, 18, 20)
    pos = np.array([I32_MAX - 8 + 1, -2, 5], dtype=np.int64)
    w = far_world(size, pos, 16)
    lo, hi = w.window()
    assert hi[0] == I32_MAX and ((I32_MIN - int(pos[0])) + 2 ** 31) % 2 ** 32 - 2 ** 31 == 8
    r = RawRoute(w)
    store = W.DeviceGlobalMap(TAU, 0)
    store.put_chunk((5, 5, 5), M.draw_words(np.random.default_rng(1), CW))
    before, sbefore = state(r.t, r.n), store_state(store)
    buf = np.full(4, 0xdeadbeef, dtype=np.uint32)
    for a, b in [((I32_MIN, lo[1], lo[2]), (I32_MIN, lo[1], lo[2])), ((I32_MIN, lo[1], lo[2]), (I32_MIN, lo[1] + 1, lo[2] + 1))]:
        a, b = _i3(a), _i3(b)
        assert r.L.ws_map_extract_box(r.t.handle, 0, _p(a), _p(b), _p(buf)) == WS_ERR_INVALID
        assert r.L.ws_map_insert_box(r.t.handle, 0, _p(a), _p(b), _p(buf)) == WS_ERR_INVALID
        assert r.L.ws_store_save_box(store.handle, r.t.handle, 0, _p(a), _p(b)) == WS_ERR_INVALID
        assert r.L.ws_store_load_box(store.handle, r.t.handle, 0, _p(a), _p(b)) == WS_ERR_INVALID
    assert np.all(buf == 0xdeadbeef)
    assert same_state(before, state(r.t, r.n)) and same_store(sbefore, store_state(store)) and store.count() == 1
    # ... while the window's own last voxel is served
    assert np.array_equal(r.t.avg_map().extract_box((I32_MAX, lo[1], lo[2]), (I32_MAX, lo[1], lo[2])), w.box((I32_MAX, lo[1], lo[2]), (I32_MAX, lo[1], lo[2])).reshape(-1))
    # a map whose window does not fit (ws_map_set_params does not ask): WS_ERR_RANGE from the box calls, nothing moves
    out = _i3((I32_MAX - 3, -2, 5))
    assert r.L.ws_map_set_params(r.t.handle, 0, _p(_i3(size)), _p(out), _p(_i3(w.offset()))) == 0
    a = _i3((I32_MAX, lo[1], lo[2]))
    for rc in (r.L.ws_map_extract_box(r.t.handle, 0, _p(a), _p(a), _p(buf)), r.L.ws_map_insert_box(r.t.handle, 0, _p(a), _p(a), _p(buf)),
               r.L.ws_store_save_box(store.handle, r.t.handle, 0, _p(a), _p(a)), r.L.ws_store_load_box(store.handle, r.t.handle, 0, _p(a), _p(a)),
               r.L.ws_shift_device(r.t.handle, store.handle, _p(_i3((I32_MAX - 10, -2, 5))))):
        assert rc == WS_ERR_RANGE, _last_error(r.L)
    assert r.L.ws_map_set_params(r.t.handle, 0, _p(_i3(size)), _p(_i3(pos)), _p(_i3(w.offset()))) == 0
    assert same_state(before, state(r.t, r.n)) and same_store(sbefore, store_state(store))


# ------------------------------------------------------------------------------------------------ d, e. thin windows over many chunks
def thin_window(nc_y, nc_z, cy0, cz0):
    """the smallest window of 3 voxels in x that straddles the chunk border x = 64 (two chunks in x) and overlaps nc_y x nc_z
    chunks in y and z, the first of them (cy0, cz0): one voxel of the first chunk, one of the last, everything in between"""
    size = np.array([3, 64 * (nc_y - 2) + 2, 64 * (nc_z - 2) + 2], dtype=np.int64)
    lo = np.array([63, 64 * cy0 + 63, 64 * cz0 + 63], dtype=np.int64)
    return size, lo + size // 2, lo, lo + size - 1


def need_gpu_memory(gib):
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free / 2 ** 30 < gib:
        if os.environ.get("WS_ALLOW_BIG_SKIP") == "1":
            pytest.skip(f"needs ~{gib} GB on the GPU")
        pytest.fail(f"needs ~{gib} GB on the GPU (set WS_ALLOW_BIG_SKIP=1 to skip on this box)")


class ThinMap:
    """a device-only map whose avg ring is seen through torch (device_ptr()): `world()` is the window in world order"""

    def __init__(self, size, pos, offset):
        import warpsense_amd as W
        from warpsense_amd._abi import _device_tensor
        self.size, self.pos, self.offset = (np.asarray(v, dtype=np.int64) for v in (size, pos, offset))
        self.t = W.TSDFCuda(W.DeviceMap(_i3(size), _i3(offset), None, _i3(pos)), TAU, MW, RES)
        self.ring = _device_tensor(self.t.avg_map().device_ptr(), tuple(int(v) for v in size), "<i4", self.t)
        # world voxel lo + i lies in storage plane (i - size/2 + offset) mod size (get_index)
        self.roll = tuple(int(v) for v in (self.offset - self.size // 2) % self.size)

    def randomize(self, seed):
        import torch
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        _sync()
        self.ring.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, tuple(self.ring.shape), dtype=torch.int32, device="cuda", generator=g))
        _sync()

    def to_ring(self, world):
        import torch
        return torch.roll(world, shifts=self.roll, dims=(0, 1, 2))

    def world(self):
        import torch
        _sync()
        return torch.roll(self.ring, shifts=tuple(-v for v in self.roll), dims=(0, 1, 2))

    def holds(self, world):
        """the ring on the device == `world` (a numpy uint32 or a torch int32 array over the window, world order)"""
        import torch
        if isinstance(world, np.ndarray):
            world = torch.from_numpy(world.view(np.int32)).cuda()
        _sync()
        return torch.equal(self.ring, self.to_ring(world))


def rel(lo, a, b):
    return tuple(slice(int(a[k] - lo[k]), int(b[k] - lo[k]) + 1) for k in range(3))


def test_load_with_a_slot_table_beyond_its_first_size():
    """one load_box whose slot table has 8320 words (8192 is what a table holds from the start: it grows inside the call), with
    present chunks at the first and the last word, either side of word 8192 and at drawn words; then eight small saves and loads
    without a wait, which take the ring of eight tables once round and past the grown one, and a ninth"""
    import warpsense_amd as W
    fill = np.uint32(_default())
    size, pos, lo, hi = thin_window(64, 65, -31, -32)
    keys = [tuple(int(v) for v in k) for k in W.chunks_of_box(lo, hi)]
    n = len(keys)
    assert n == 2 * 64 * 65 == 8320 > 8192 and 2 * 64 * 64 <= 8192 and 2 * 63 * 65 <= 8192  # no smaller y / z chunk count passes 8192
    need_gpu_memory(4)  # two rings of 194 MB, the expected window and its rolled copies
    rng = np.random.default_rng(8192)
    words = [0, 8191, 8192, n - 1] + sorted(int(v) for v in rng.choice(np.arange(1, n - 1), 4, replace=False))
    store = W.DeviceGlobalMap(TAU, 0)
    store.reserve(256)  # (no segment is added below: nothing but the table makes a call wait)
    cmodel = {keys[i]: M.draw_words(rng, CW).reshape(64, 64, 64) for i in words}
    for key, c in cmodel.items():
        store.put_chunk(key, c)
    m = ThinMap(size, pos, M.model_offset(size, pos))
    assert np.all(m.offset != 0) and np.all(m.offset != size // 2)
    m.randomize(1)
    exp = np.full(tuple(int(v) for v in size), fill, dtype=np.uint32)  # the window in world order: built once, on the host
    for key, c in cmodel.items():
        sl, ia, ib = chunk_box(key, lo, hi)
        exp[rel(lo, ia, ib)] = c[sl]
    assert np.count_nonzero(exp != fill) > 1000
    store.load_box(m.t, lo, hi)
    assert m.holds(exp)
    assert store.count() == len(words)
    # eight small calls back to back, each over the chunk border x = 64 and over borders in y and z
    m.randomize(2)
    exp = m.world().cpu().numpy().view(np.uint32).copy()

    def save(a, b):
        store.save_box(m.t, a, b)
        for key in [tuple(int(v) for v in k) for k in W.chunks_of_box(a, b)]:
            c = cmodel.setdefault(key, np.full((64, 64, 64), fill, dtype=np.uint32))
            sl, ia, ib = chunk_box(key, a, b)
            c[sl] = exp[rel(lo, ia, ib)]

    def load(a, b):
        store.load_box(m.t, a, b)
        exp[rel(lo, a, b)] = fill
        for key in [tuple(int(v) for v in k) for k in W.chunks_of_box(a, b)]:
            if key in cmodel:
                sl, ia, ib = chunk_box(key, a, b)
                exp[rel(lo, ia, ib)] = cmodel[key][sl]

    def small_box():
        a = np.array([63, rng.integers(lo[1], hi[1] - 180), rng.integers(lo[2] + 30, hi[2] - 140)], dtype=np.int64)
        return a, a + np.array([2, rng.integers(64, 140), rng.integers(64, 140)])

    tables = 1
    for i in range(4):
        a, b = small_box()
        save(a, b)
        shift = np.array([0, 30, -30])
        load(a + shift, b + shift)  # what was saved, moved by 30 voxels in the ring, and fill around it
        tables += 2
    assert tables == 9  # the ring of eight tables is round once: the grown table has been used again
    assert m.holds(exp)
    for key, c in cmodel.items():
        assert np.array_equal(store.chunk(key).reshape(64, 64, 64), c), key
    a, b = small_box()
    load(a, b)
    assert m.holds(exp) and store.count() == len(cmodel)


def test_save_with_a_slot_table_beyond_its_first_size():
    """one save_box of the whole thin window into an empty store: 8320 chunks of 1 MiB are created (8.7 GB), all flagged new and
    written whole.  Loaded back into a second map whose ring is rotated differently, both windows agree in world order; drawn
    chunks are the window's voxels inside the box and fill outside, the corner chunk the box grazes with one voxel included"""
    import torch
    import warpsense_amd as W
    fill = np.uint32(_default())
    size, pos, lo, hi = thin_window(64, 65, -31, -32)
    keys = [tuple(int(v) for v in k) for k in W.chunks_of_box(lo, hi)]
    n = len(keys)
    assert n == 8320 > 8192
    need_gpu_memory(12)  # 8320 chunks of 1 MiB = 8.7 GB, four rings of 194 MB, rolled copies
    m1 = ThinMap(size, pos, M.model_offset(size, pos))
    m1.randomize(3)
    store = W.DeviceGlobalMap(TAU, 0)
    store.save_box(m1.t, lo, hi)
    assert store.count() == n and store.keys() == keys
    m2 = ThinMap(size, pos, (1, 777, 3001))
    m2.randomize(4)
    store.load_box(m2.t, lo, hi)
    w1 = m1.world()
    assert torch.equal(w1, m2.world()) and not torch.equal(m1.ring, m2.ring)
    assert store.count() == n
    rng = np.random.default_rng(12)
    drawn = [0, 8191, 8192, n - 1] + [int(v) for v in rng.choice(n, 8, replace=False)]
    for i in drawn:
        sl, ia, ib = chunk_box(keys[i], lo, hi)
        want = np.full((64, 64, 64), fill, dtype=np.uint32)
        want[sl] = w1[rel(lo, ia, ib)].cpu().numpy().view(np.uint32)
        if i == 0:
            assert np.count_nonzero(want != fill) <= 1 and sl == (slice(63, 64),) * 3  # grazed: one voxel of the box
        assert np.array_equal(store.chunk(keys[i]).reshape(64, 64, 64), want), keys[i]


def test_load_of_more_chunks_than_one_grid_pass():
    """the load of test_load_with_a_slot_table_beyond_its_first_size at the smallest thin window whose box overlaps more than 65 535
    chunks (2 x 182 x 181 = 65 884): blockIdx.y has to stride.  Present chunks at table words 0, 65 534, 65 535, 65 536 and the
    last.  Load only (a save would create 64 GB of chunks).  The ring is 3 x 11 522 x 11 458 voxels = 1.58 GB; avg and new ring take
    3.2 GB, the expected window and its rolled copies as much again: 12 GB are asked for.  The expected window is built on the
    device (a fill and five slices uploaded)."""
    import torch
    import warpsense_amd as W
    fill = np.uint32(_default())
    size, pos, lo, hi = thin_window(182, 181, -81, -101)
    keys = W.chunks_of_box(lo, hi)
    n = len(keys)
    assert n == 2 * 182 * 181 == 65884 and min(n, 65535) < n and 2 * 181 * 181 <= 65535  # no smaller y / z chunk count passes 65 535
    need_gpu_memory(12)
    rng = np.random.default_rng(65535)
    store = W.DeviceGlobalMap(TAU, 0)
    m = ThinMap(size, pos, M.model_offset(size, pos))
    assert np.all(m.offset != 0) and np.all(m.offset != size // 2)
    m.randomize(5)
    exp = torch.full(tuple(int(v) for v in size), int(fill), dtype=torch.int32, device="cuda")
    for i in [0, 65534, 65535, 65536, n - 1]:
        key = tuple(int(v) for v in keys[i])
        c = M.draw_words(rng, CW).reshape(64, 64, 64)
        store.put_chunk(key, c)
        sl, ia, ib = chunk_box(key, lo, hi)
        exp[rel(lo, ia, ib)] = torch.from_numpy(np.ascontiguousarray(c[sl]).view(np.int32)).cuda()
    assert int((exp != int(fill)).sum()) > 1000
    store.load_box(m.t, lo, hi)
    assert m.holds(exp)
    assert store.count() == 5


# ------------------------------------------------------------------------------------------------ f. the table ring, on purpose
def test_the_table_ring_wraps_without_a_wait():
    """three diagonal ws_shift_device calls out and three back, back to back: 36 launches on 8 tables and nothing in between that
    waits for the device (the store's segments are there beforehand).  Then the model check and the chunk check."""
    size = (21, 17, 13)
    r = StoreRoute(size)
    r.store.reserve(64)
    w = M.World(size, -4 * np.asarray(size), 4 * np.asarray(size), _default())
    lo, hi = w.window()
    words = M.draw_words(np.random.default_rng(36), np.prod(size))
    r.insert(lo, hi, words)
    w.write(lo, hi, words)
    steps = [(9, -8, 6), (18, -16, 12), (27, -24, 18), (18, -16, 12), (9, -8, 6), (0, 0, 0)]
    launches = 0
    L, t = r.t._L, r.t
    for new_pos in steps:
        launches += 2 * len(M.expected_slabs(size, w.pos, new_pos))
        assert L.ws_shift_device(t.handle, r.store.handle, _p(_i3(new_pos))) == 0, _last_error(L)
        w.move(new_pos)
    assert launches == 36 and r.store.capacity() == 256  # (no segment was added on the way)
    r.lm.follow(np.asarray(steps[-1]))
    r.check(w)
    chunks = r.finish(w)
    assert np.count_nonzero(w.store != w.default_raw) > 0 and len(chunks) >= 4
