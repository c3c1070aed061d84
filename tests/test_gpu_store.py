"""The global map in device memory (ws_store_*, ws_shift_device, map_store.hip) against the world model of tests/window_model.py and
against today's host route (TSDFMapping.shift_map with an in-memory GlobalMap).  Every comparison is np.array_equal."""
import os

import numpy as np
import pytest

from window_model import WALKS
import window_model as M
from window_routes import MW, RES, TAU, MappingRoute, RawRoute, _default, _i3, _p, _params, check_device, download, get_params, same_state, state
from window_routes import CW, StoreRoute, chunk_box, same_store, store_state
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu

WS_ERR_INVALID, WS_ERR_CAPACITY = -1, -4


# ------------------------------------------------------------------------------------------------ 1. the walks
_HOST_WALKS = {}


def host_walk(size, seed):
    """the same walk through today's synchronous host route, once per walk: its chunks by key"""
    if (size, seed) not in _HOST_WALKS:
        r = MappingRoute(size, asyn=False)
        w = M.run_walk(size, M.make_walk(size, seed), seed, r, _default(), check_every=False)
        r.finish(w)
        _HOST_WALKS[(size, seed)] = {k: v.copy() for k, v in r.lm.map_.chunks.items()}
    return _HOST_WALKS[(size, seed)]


@pytest.mark.parametrize("segment_chunks", [0, 2])
@pytest.mark.parametrize("size,seed", WALKS)
def test_walk_through_the_store(size, seed, segment_chunks):
    walk = M.make_walk(size, seed)
    r = StoreRoute(size, segment_chunks=segment_chunks)
    w = M.run_walk(size, walk, seed, r, _default())
    chunks = r.finish(w)
    assert np.all(w.pos == 0) and np.count_nonzero(w.store != w.default_raw) > 0
    host = host_walk(size, seed)
    assert sorted(chunks) == sorted(host) and r.store.keys() == sorted(host)
    for key in host:
        assert np.array_equal(chunks[key], host[key]), key
    if segment_chunks == 2:
        assert r.store.capacity() >= r.store.count() > 2 and r.store.capacity() % 2 == 0  # more than one segment
    if size == (71, 61, 67):
        assert min(k[0] for k in chunks) < 0 and max(k[0] for k in chunks) > 0  # negative chunks, chunk borders


# ------------------------------------------------------------------------------------------------ 2. raw boxes
def rotated_world(size, pos, seed):
    w = M.World(size, np.asarray(pos) - 2 * np.asarray(size), np.asarray(pos) + 2 * np.asarray(size), _default())
    w.pos = np.asarray(pos, dtype=np.int64)
    lo, hi = w.window()
    w.write(lo, hi, M.draw_words(np.random.default_rng(seed), np.prod(size)))
    assert np.all(w.offset() != 0)
    return w


@pytest.mark.parametrize("size,pos", [((71, 61, 67), (40, -25, 30)), ((16, 18, 20), (3, -2, 5)), ((70, 66, 130), (-31, 40, -70))])
def test_save_box_and_load_box(size, pos):
    """save_box / load_box on boxes that cross the ring seam in every axis, odd and even sizes: a chunk created by a partial save is
    fill outside the box, a second partial save keeps the first one's voxels, a load over absent chunks gives fill and creates
    nothing, a load over present chunks gives their voxels"""
    import warpsense_amd as W
    fill = np.uint32(_default())
    w = rotated_world(size, pos, 5)
    r = RawRoute(w)
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    rng = np.random.default_rng(6)
    boxes = M.draw_boxes(size, pos, rng, count=3)
    assert M.crosses_all_seams(size, pos, *boxes[0])
    model = {}  # key -> (64, 64, 64): what the store must hold
    for a, b in boxes:
        store.save_box(r.t, a, b)
        for key in [tuple(k) for k in W.chunks_of_box(a, b)]:
            c = model.setdefault(key, np.full((64, 64, 64), fill, dtype=np.uint32))
            sl, ia, ib = chunk_box(key, a, b)
            c[sl] = w.box(ia, ib)
        assert store.keys() == sorted(model)
        for key, c in model.items():
            assert np.array_equal(store.chunk(key).reshape(64, 64, 64), c), (key, a, b)  # fill outside, earlier saves kept
        check_device(r.t, w)  # a save leaves the ring alone
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
    r.t.avg_map().insert_box(lo, hi, words)
    w.write(lo, hi, words)
    a, b = boxes[0]
    empty.load_box(r.t, a, b)
    w.write(a, b, np.full(int(np.prod(b - a + 1)), fill, dtype=np.uint32))
    check_device(r.t, w)
    assert empty.count() == 0 and empty.keys() == []
    # a load into new_map ends "new_map is default": the next shift is refused
    store.load_box(r.t, a, b, which=1)
    assert r.L.ws_shift_device(r.t.handle, store.handle, _p(_i3(np.asarray(pos) + 1))) == WS_ERR_INVALID
    # boxes outside the window or wrapping onto themselves are refused and nothing moves
    before, sbefore = state(r.t, r.n), store_state(store)
    for a2, b2 in [((lo[0] - 1, lo[1], lo[2]), tuple(hi)), (tuple(lo), (hi[0], hi[1], hi[2] + 1)), ((lo[0] + 2, lo[1], lo[2]), (lo[0] + 1, hi[1], hi[2]))]:
        for f in (r.L.ws_store_save_box, r.L.ws_store_load_box):
            assert f(store.handle, r.t.handle, 0, _p(_i3(a2)), _p(_i3(b2))) == WS_ERR_INVALID
    assert r.L.ws_store_save_box(store.handle, r.t.handle, 2, _p(_i3(lo)), _p(_i3(lo))) == WS_ERR_INVALID
    assert same_state(before, state(r.t, r.n)) and same_store(sbefore, store_state(store))


# ------------------------------------------------------------------------------------------------ 3. chunk round trips
def test_chunk_round_trips_and_slot_reuse():
    import warpsense_amd as W
    size, pos = (21, 17, 13), (14, -5, 3)
    w = rotated_world(size, pos, 7)
    r = RawRoute(w)
    fill = np.uint32(_default())
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2)
    rng = np.random.default_rng(8)
    data = {key: M.draw_words(rng, CW) for key in [(0, -1, 0), (0, 0, 0), (-1, -1, 0), (5, 5, 5)]}
    for key, d in data.items():
        assert not store.has_chunk(*key) and store.chunk(key) is None
        store.put_chunk(key, d)
    assert store.keys() == sorted(data) and store.count() == 4 and store.capacity() == 4
    for key, d in data.items():
        assert store.has_chunk(*key) and np.array_equal(store.chunk(key), d)
    assert r.L.ws_store_chunk_dev(store.handle, _p(_i3((0, 0, 0)))) and not r.L.ws_store_chunk_dev(store.handle, _p(_i3((9, 9, 9))))
    # the window over the chunks: a load gives their voxels
    lo, hi = w.window()
    assert lo[1] < 0 <= hi[1] and lo[0] >= 0 and lo[2] < 0  # (0, -1, 0), (0, 0, 0) and absent (0, *, -1)
    store.load_box(r.t, lo, hi)
    want = np.full(tuple(int(v) for v in size), fill, dtype=np.uint32)
    for key in [(0, -1, 0), (0, 0, 0)]:
        sl, ia, ib = chunk_box(key, lo, hi)
        want[tuple(slice(int(ia[k] - lo[k]), int(ib[k] - lo[k]) + 1) for k in range(3))] = data[key].reshape(64, 64, 64)[sl]
    w.write(lo, hi, want)
    check_device(r.t, w)
    assert np.count_nonzero(want == fill) > 0 and np.count_nonzero(want != fill) > 0
    # overwrite, then drop: gone, its space loads as fill, dropping it again is refused
    again = M.draw_words(rng, CW)
    store.put_chunk((0, 0, 0), again)
    assert np.array_equal(store.chunk((0, 0, 0)), again) and store.count() == 4
    store.drop_chunk((0, 0, 0))
    assert not store.has_chunk(0, 0, 0) and store.chunk((0, 0, 0)) is None and store.count() == 3 and (0, 0, 0) not in store.keys()
    with pytest.raises(W.WsError):
        store.drop_chunk((0, 0, 0))
    store.load_box(r.t, lo, hi)
    sl, ia, ib = chunk_box((0, 0, 0), lo, hi)
    w.write(ia, ib, np.full(int(np.prod(ib - ia + 1)), fill, dtype=np.uint32))
    check_device(r.t, w)
    # the freed slot goes to the next chunk a save creates: it holds that chunk's data only (fill outside the box), no segment is added
    words = M.draw_words(rng, np.prod(size))
    r.t.avg_map().insert_box(lo, hi, words)
    w.write(lo, hi, words)
    a, b = (lo[0] + 1, 1, 2), (hi[0] - 1, hi[1] - 1, hi[2] - 1)  # inside chunk (0, 0, 0) only
    assert [tuple(k) for k in W.chunks_of_box(a, b)] == [(0, 0, 0)]
    store.save_box(r.t, a, b)
    assert store.count() == 4 and store.capacity() == 4
    want = np.full((64, 64, 64), fill, dtype=np.uint32)
    sl, ia, ib = chunk_box((0, 0, 0), a, b)
    want[sl] = w.box(ia, ib)
    assert np.array_equal(store.chunk((0, 0, 0)).reshape(64, 64, 64), want)
    for key in [(0, -1, 0), (-1, -1, 0), (5, 5, 5)]:
        assert np.array_equal(store.chunk(key), data[key])  # the neighbours in the pool are as they were
    # reserve, flush_to and load_from
    store.reserve(9)
    assert store.capacity() >= 9 and store.count() == 4
    g = W.GlobalMap(TAU, 0)
    g.activate_chunk(7, 7, 7)[:] = 99
    store.flush_to(g)
    assert sorted(g.chunks) == sorted(store.keys() + [(7, 7, 7)])
    for key in store.keys():
        assert np.array_equal(g.chunks[key], store.chunk(key))
    back = W.DeviceGlobalMap(TAU, 0)
    back.load_from(g, [(7, 7, 7), (5, 5, 5), (1, 2, 3)])
    assert back.keys() == [(5, 5, 5), (7, 7, 7)] and np.all(back.chunk((7, 7, 7)) == 99) and np.array_equal(back.chunk((5, 5, 5)), data[(5, 5, 5)])
    back.close()
    back.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_change_nothing():
    import warpsense_amd as W
    size, pos = (71, 61, 67), (10, -20, 5)
    w = rotated_world(size, pos, 9)
    r = RawRoute(w)
    L, t = r.L, r.t
    diag = tuple(int(v) for v in np.asarray(pos) + np.array([30, -25, 40]))
    # how many chunks the diagonal shift creates: the leaving slabs of its three axes, each chunk once
    need = {tuple(k) for s in M.expected_slabs(size, pos, diag) for k in W.chunks_of_box(*s["leave"])}
    assert len(need) > 8
    seed_key = min(need)
    seed = M.draw_words(np.random.default_rng(10), CW)
    before = state(t, r.n)

    def refused(rc, st, code=WS_ERR_INVALID):
        assert rc == code, (rc, L.ws_last_error())
        assert same_state(before, state(t, r.n)) and same_store(sbefore, store_state(st))

    # max_chunks one below what the shift needs: found before the first launch
    small = W.DeviceGlobalMap(TAU, 0, max_chunks=len(need) - 1, segment_chunks=2)
    sbefore = store_state(small)
    refused(L.ws_shift_device(t.handle, small.handle, _p(_i3(diag))), small, WS_ERR_CAPACITY)
    assert small.count() == 0
    small.put_chunk(seed_key, seed)  # (a chunk the shift needs is there already: the others still do not fit)
    sbefore = store_state(small)
    refused(L.ws_shift_device(t.handle, small.handle, _p(_i3(diag))), small, WS_ERR_CAPACITY)
    small.close()
    # a store the shift fits into exactly, one of its chunks seeded
    store = W.DeviceGlobalMap(TAU, 0, max_chunks=len(need), segment_chunks=2)
    store.put_chunk(seed_key, seed)
    sbefore = store_state(store)
    # an open ws_shift_begin ticket
    rc, ticket = r.begin(pos)
    assert rc == 0
    refused(L.ws_shift_device(t.handle, store.handle, _p(_i3(diag))), store)
    assert L.ws_shift_end(ticket) == 0
    # a step of size + 1, per axis and direction
    for axis in range(3):
        for sign in (1, -1):
            far = list(pos)
            far[axis] += sign * (size[axis] + 1)
            refused(L.ws_shift_device(t.handle, store.handle, _p(_i3(far))), store)
    # a store of another context
    ctx2 = W.Context()
    other = W.DeviceGlobalMap(TAU, 0, ctx=ctx2)
    refused(L.ws_shift_device(t.handle, other.handle, _p(_i3(diag))), store)
    lo, hi = w.window()
    refused(L.ws_store_save_box(other.handle, t.handle, 0, _p(_i3(lo)), _p(_i3(hi))), store)
    refused(L.ws_store_load_box(other.handle, t.handle, 0, _p(_i3(lo)), _p(_i3(hi))), store)
    assert other.count() == 0
    other.close()
    ctx2.close()
    # NULL arguments
    refused(L.ws_shift_device(t.handle, None, _p(_i3(diag))), store)
    refused(L.ws_shift_device(t.handle, store.handle, None), store)
    # new_map not default
    t.new_map().insert_box(lo, lo, np.array([12345], dtype=np.uint32))
    before = state(t, r.n)
    refused(L.ws_shift_device(t.handle, store.handle, _p(_i3(diag))), store)
    t.new_map().to_device(W.DeviceMap(_i3(w.size), _i3(w.offset()), np.full(r.n, _default(), dtype=np.uint32), _i3(w.pos)))
    before = state(t, r.n)
    # new_pos == pos: WS_OK and nothing happens
    refused(L.ws_shift_device(t.handle, store.handle, _p(_i3(pos))), store, 0)
    # and now the shift itself: it fits under max_chunks exactly, the seeded chunk keeps its voxels outside the slabs
    assert L.ws_shift_device(t.handle, store.handle, _p(_i3(diag))) == 0, L.ws_last_error()
    w.move(diag)
    check_device(t, w)
    assert set(store.keys()) == need and store.count() == len(need)
    chunks = {k: store.chunk(k) for k in store.keys()}
    covered = np.zeros((64, 64, 64), dtype=bool)
    for s in M.expected_slabs(size, pos, diag):
        cb = chunk_box(seed_key, *s["leave"])
        if cb is not None:
            covered[cb[0]] = True
    assert covered.any() and not covered.all()
    assert np.array_equal(chunks[seed_key].reshape(64, 64, 64)[~covered], seed.reshape(64, 64, 64)[~covered])
    chunks[seed_key] = np.where(covered, chunks[seed_key].reshape(64, 64, 64), np.uint32(_default())).reshape(-1)
    w.check_chunks(chunks)
    # full: one more chunk is refused with WS_ERR_CAPACITY by put_chunk and save_box alike
    before, sbefore = state(t, r.n), store_state(store)
    free_key = (max(k[0] for k in need) + 3, 0, 0)
    assert L.ws_store_put_chunk(store.handle, _p(_i3(free_key)), _p(seed)) == WS_ERR_CAPACITY
    back = tuple(int(v) for v in np.asarray(diag) + np.array([0, 0, 67]))
    refused(L.ws_shift_device(t.handle, store.handle, _p(_i3(back))), store, WS_ERR_CAPACITY)


# ------------------------------------------------------------------------------------------------ 5. write_back
def _write_back_pair(make_global):
    """the same window written back through the store and through today's route: (store route's global map, host route's)"""
    import warpsense_amd as W
    size, pos = (71, 61, 67), (40, -25, 30)
    out = []
    for use_store in (True, False):
        g = make_global(use_store)
        lm = W.LocalMap(*size, TAU, 0, g)
        store = W.DeviceGlobalMap(TAU, 0, segment_chunks=2) if use_store else None
        tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
        w = M.World(size, np.asarray(pos) - 80, np.asarray(pos) + 80, _default())
        rng = np.random.default_rng(71)
        for step in ((0, 0, 0), pos):
            if any(step):
                (tm.shift_map_device if use_store else tm.shift_map)(step)
                w.move(step)
            lo, hi = w.window()
            words = M.draw_words(rng, np.prod(size))
            tm.tsdf().avg_map().insert_box(lo, hi, words)
            w.write(lo, hi, words)
        if use_store:  # a partial write-back first: inside the box the window, outside what the store held before
            a, b = (50, -20, -2), (70, 3, 40)
            tm.write_back(a, b)
            it = M.box_inter(np.asarray(a), np.asarray(b), *w.window())
            w.store[w.sl(*it)] = w.world[w.sl(*it)]
            w.check_chunks({k: store.chunk(k) for k in store.keys()})
        tm.write_back()
        lo, hi = w.window()
        w.store[w.sl(lo, hi)] = w.world[w.sl(lo, hi)]
        check_device(tm.tsdf(), w)
        out.append((g, w, tm))
    return out


def test_write_back_through_the_store_in_memory():
    import warpsense_amd as W
    (g_store, w, _), (g_host, _, _) = _write_back_pair(lambda use_store: W.GlobalMap(TAU, 0))
    w.check_chunks(g_store.chunks)
    assert sorted(g_store.chunks) == sorted(g_host.chunks) and len(g_host.chunks) >= 8
    for key in g_host.chunks:
        assert np.array_equal(g_store.chunks[key], g_host.chunks[key]), key


def test_write_back_through_the_store_h5(tmp_path):
    from warpsense_amd import build
    if build.find_hdf5() is None or build.build_h5() is None:
        pytest.skip("no HDF5 C library on this box")
    import warpsense_amd as W
    paths = {True: str(tmp_path / "store.h5"), False: str(tmp_path / "host.h5")}
    (g_store, w, _), (g_host, _, _) = _write_back_pair(lambda use_store: W.GlobalMap(TAU, 0, filename=paths[use_store], map_params=_params((71, 61, 67)).map))

    def read_back(g, path):
        g.close()
        g2 = W.GlobalMap(TAU, 0, filename=path, open_existing=True)
        out = {key: g2.activate_chunk(*key).copy() for key in sorted(g2._in_file)}
        g2._H.ws_h5_close(g2._file)
        g2._file = None
        return out

    a, b = read_back(g_store, paths[True]), read_back(g_host, paths[False])
    w.check_chunks(a)
    assert sorted(a) == sorted(b) and len(a) >= 8
    for key in b:
        assert np.array_equal(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------ 6. the hot path
def test_hot_path_agrees_with_the_host_shift():
    """update, shift by (7, -5, 3), update, register_cloud on a 65^3 map: both map downloads, the pose bits and the iteration count
    are those of the same sequence with shift_map"""
    import warpsense_amd as W
    size, step = (65, 65, 65), (7, -5, 3)
    results = []
    for use_store in (True, False):
        lm = W.LocalMap(*size, TAU, 0)
        store = W.DeviceGlobalMap(TAU, 0) if use_store else None
        reg = W.TSDFRegistration(_params(size), lm, device_global_map=store)
        pts = S.os1_128_scan(rings=32, azimuths=256, half_extents_mm=(1400.0, 1300.0, 1200.0), seed=3)
        reg.update_tsdf(pts, pos_rm=(0, 0, 0), up_rm=(0, 0, 32768))
        (reg.shift_map_device if use_store else reg.shift_map)(step)
        pts2 = S.os1_128_scan(sensor_mm=(350.0, -250.0, 150.0), rings=32, azimuths=256, half_extents_mm=(1400.0, 1300.0, 1200.0), seed=4)
        reg.update_tsdf(pts2, pos_rm=step, up_rm=(0, 0, 32768))
        q = S.transform_points_mm(pts2, S.perturbation(30, 20, 0, 1.5))
        T = reg.register_cloud(q, np.eye(4, dtype=np.float32))
        n = int(np.prod(size))
        results.append((download(reg.tsdf(), 0, n), download(reg.tsdf(), 1, n), T.view(np.uint32).copy(), reg.last_iterations,
                        [np.concatenate(get_params(reg.tsdf(), k)) for k in (0, 1)]))
    a, b = results
    assert np.array_equal(a[0].data_, b[0].data_) and np.array_equal(a[1].data_, b[1].data_)
    assert np.array_equal(a[0].pos_, step) and np.array_equal(a[0].pos_, b[0].pos_) and np.array_equal(a[0].offset_, b[0].offset_)
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] and a[3] > 1
    assert all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))
    assert np.count_nonzero(a[0].data_ != np.uint32(_default())) > 10_000


# ------------------------------------------------------------------------------------------------ 7. beyond word 2^30
def test_a_box_beyond_word_2_30():
    """a 1025^3 map (2^30 + 3.2 M voxels, 4.3 GB): with pos x = 1024 the window's first plane x = 512 is the LAST storage plane, whose
    words lie beyond 2^30 (byte offsets beyond 4 GiB).  Save a box there, overwrite the ring, load, compare."""
    import torch
    import warpsense_amd as W
    free, _ = torch.cuda.mem_get_info()
    if free / 2 ** 30 < 16:
        if os.environ.get("WS_ALLOW_BIG_SKIP") == "1":
            pytest.skip("needs ~16 GB on the GPU")
        pytest.fail("needs ~16 GB on the GPU (set WS_ALLOW_BIG_SKIP=1 to skip on this box)")
    size = (1025, 1025, 1025)
    pos = np.array([1024, 300, -200], dtype=np.int64)  # (the y and z seams well inside the window)
    lm = W.LocalMap(*size, TAU, 0, host_voxels=False)
    lm.pos[:] = pos
    lm.offset[:] = M.model_offset(size, pos)
    store = W.DeviceGlobalMap(TAU, 0)
    tm = W.TSDFMapping(_params(size), lm, device_global_map=store)
    avg = tm.tsdf().avg_map()
    lo, hi = M.window(size, pos)
    assert lo[0] == 512 and (lo[0] + 512) % 1025 == 1024 and 1024 * 1025 * 1025 > 2 ** 30
    # the last storage plane around the y and z seams (storage y, z = 1024 | 0), and the first plane next to it (world x = 513)
    y_last, z_last = int(lo[1] + (1024 - (lo[1] + 512)) % 1025), int(lo[2] + (1024 - (lo[2] + 512)) % 1025)
    a, b = np.array([512, y_last - 40, z_last - 70]), np.array([513, y_last + 30, z_last + 50])
    assert np.all(a >= lo) and np.all(b <= hi)
    rng = np.random.default_rng(30)
    n = int(np.prod(b - a + 1))
    words = M.draw_words(rng, n)
    avg.insert_box(a, b, words)
    store.save_box(tm.tsdf(), a, b)
    keys = [tuple(k) for k in W.chunks_of_box(a, b)]
    assert store.keys() == keys and len(keys) == 6
    box = words.reshape(tuple(int(v) for v in b - a + 1))
    for key in keys:
        sl, ia, ib = chunk_box(key, a, b)
        want = np.full((64, 64, 64), np.uint32(_default()), dtype=np.uint32)
        want[sl] = box[tuple(slice(int(ia[k] - a[k]), int(ib[k] - a[k]) + 1) for k in range(3))]
        assert np.array_equal(store.chunk(key).reshape(64, 64, 64), want), key
    avg.insert_box(a, b, M.draw_words(rng, n))  # the ring there is something else now ...
    guard_a, guard_b = np.array([514, a[1], a[2]]), np.array([516, b[1], b[2]])  # ... and where an offset wrapped at 2^32 would land
    guard = M.draw_words(rng, int(np.prod(guard_b - guard_a + 1)))
    avg.insert_box(guard_a, guard_b, guard)
    store.load_box(tm.tsdf(), a, b)
    assert np.array_equal(avg.extract_box(a, b), words)
    assert np.array_equal(avg.extract_box(guard_a, guard_b), guard)
