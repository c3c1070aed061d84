"""The routes by which the tests drive a sliding window against the world model of tests/window_model.py: TSDFMapping, the raw C ABI,
and the device global map; with the state comparisons and the parameter helpers they share."""
import ctypes as C

import numpy as np

import window_model as M


TAU, RES, MW = 1000, 50, 640


def _default():
    import warpsense_amd as W
    return int(W.pack_entry(TAU, 0))


def _i3(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _params(size, res=RES, tau=TAU):
    import warpsense_amd as W
    return W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=MW // 64, size=tuple(s * res / 1000.0 for s in size)))


def get_params(t, which):
    out = [np.zeros(3, dtype=np.int32) for _ in range(3)]
    assert t._L.ws_map_get_params(t.handle, which, *(_p(a) for a in out)) == 0, ("ws_map_get_params", which)
    return out  # size, pos, offset


def download(t, which, n):
    import warpsense_amd as W
    host = W.DeviceMap(np.zeros(3, np.int32), np.zeros(3, np.int32), None, np.zeros(3, np.int32))
    host.data_ = np.empty(n, dtype=np.uint32)
    (t.avg_map() if which == 0 else t.new_map()).to_host(host)
    return host


def state(t, n):
    """everything a refusal must leave alone: the parameters of both maps and both downloads"""
    return [np.concatenate(get_params(t, w)) for w in (0, 1)] + [download(t, w, n).data_ for w in (0, 1)]


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_device(t, w, new_default=True):
    """the invariant on the device: parameters of both maps, the whole avg_map against the model, new_map still default"""
    n = int(np.prod(w.size))
    for which in (0, 1):
        size, pos, off = get_params(t, which)
        assert np.array_equal(size, w.size) and np.array_equal(pos, w.pos), (which, pos, w.pos)
        assert np.array_equal(off, w.offset()), (which, off, w.offset())
    got = download(t, 0, n)
    assert np.array_equal(got.pos_, w.pos) and np.array_equal(got.offset_, w.offset()), (got.pos_, w.pos, got.offset_, w.offset())
    assert np.array_equal(got.data_, w.ring()), (got.data_, w.ring())
    if new_default:
        assert np.all(download(t, 1, n).data_ == np.uint32(_default())), (download(t, 1, n).data_, np.uint32(_default()))


class MappingRoute:
    """TSDFMapping.shift_map / shift_map_async with an in-memory GlobalMap"""

    def __init__(self, size, asyn, reserve=None, base=None):
        import warpsense_amd as W
        self.lm = W.LocalMap(*size, TAU, 0)
        assert tuple(self.lm.size) == tuple(size), (tuple(self.lm.size), tuple(size))
        if base is not None:  # the window starts there: through the parameters, before the device map exists
            self.lm.pos[:] = base
            self.lm.offset[:] = M.model_offset(size, base)
        self.tm = W.TSDFMapping(_params(size), self.lm)
        self.t = self.tm.tsdf()
        self.asyn = asyn
        if reserve is not None:
            self.tm.reserve_shift(reserve)

    def insert(self, lo, hi, words):
        self.t.avg_map().insert_box(lo, hi, words)

    def shift(self, w, new_pos):
        (self.tm.shift_map_async if self.asyn else self.tm.shift_map)(new_pos)

    def check(self, w):
        check_device(self.t, w)
        assert np.array_equal(self.lm.pos, w.pos) and np.array_equal(self.lm.offset, w.offset()), (self.lm.pos, w.pos, self.lm.offset, w.offset())

    def finish(self, w):
        self.tm.wait_shift()
        w.check_chunks(self.lm.map_.chunks)


class RawRoute:
    """ws_shift_* from here, as include/warpsense_hip.h describes a caller: begin; the parts of the entering boxes that the store
    already holds go back in with ws_map_insert_box; wait; every leaving slab is filed; end.  The store is a dense array over the
    model's bounding box (no chunks).  A slab holds `fill` where its voxels entered with an earlier axis of the same shift; those
    are not filed (the store already holds them).  On the way the ticket's own claims are checked against the model."""

    def __init__(self, w, tsdf=None):
        import warpsense_amd as W
        self.size = w.size
        self.n = int(np.prod(w.size))
        self.fill = int(w.default_raw)
        self.t = tsdf or W.TSDFCuda(W.DeviceMap(_i3(w.size), _i3(w.offset()), w.ring(), _i3(w.pos)), TAU, MW, RES)
        if tsdf is None:
            self.t.new_map().to_device(W.DeviceMap(_i3(w.size), _i3(w.offset()), np.full(self.n, self.fill, dtype=np.uint32), _i3(w.pos)))
        self.L = self.t._L
        self.store = np.full(w.world.shape, w.default_raw, dtype=np.uint32)
        self.slab_voxels = []

    def insert(self, lo, hi, words):
        self.t.avg_map().insert_box(lo, hi, words)

    def begin(self, new_pos):
        ticket = C.c_void_p()
        rc = self.L.ws_shift_begin(self.t.handle, _p(_i3(new_pos)), self.fill, C.byref(ticket))
        return rc, ticket

    def shift(self, w, new_pos, check_whole_entering=False):
        L = self.L
        exp = M.expected_slabs(self.size, w.pos, new_pos)
        olo, ohi = w.window()
        rc, ticket = self.begin(new_pos)
        assert rc == 0, L.ws_last_error()
        try:
            assert L.ws_shift_count(ticket) == len(exp), ("ws_shift_count", len(exp))
            lo, hi = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
            flo, fhi = M.window(self.size, new_pos)
            for i, e in enumerate(exp):
                assert L.ws_shift_entering(ticket, i, _p(lo), _p(hi)) == 0, ("ws_shift_entering", i)
                assert np.array_equal(lo, e["enter"][0]) and np.array_equal(hi, e["enter"][1]), (i, lo, hi, e["enter"])
                assert np.all(hi.astype(np.int64) - lo + 1 <= self.size), (lo, hi, self.size)
                it = M.box_inter(*e["enter"], flo, fhi)  # a later axis step may have moved a part of it out again
                if it is not None:
                    if check_whole_entering:
                        assert np.all(self.t.avg_map().extract_box(*it) == np.uint32(self.fill)), (it, self.fill)
                    self.t.avg_map().insert_box(it[0], it[1], self.store[w.sl(*it)].reshape(-1))
            assert L.ws_shift_wait(ticket) == 0, "ws_shift_wait"
            for i, e in enumerate(exp):
                data = C.c_void_p()
                assert L.ws_shift_slab(ticket, i, _p(lo), _p(hi), C.byref(data)) == 0, ("ws_shift_slab", i)
                assert np.array_equal(lo, e["leave"][0]) and np.array_equal(hi, e["leave"][1]), (i, lo, hi, e["leave"])
                ext = tuple(int(v) for v in hi.astype(np.int64) - lo + 1)
                assert all(ext[k] <= self.size[k] for k in range(3)), (ext, self.size)
                got = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint32)), shape=(int(np.prod(ext)),)).reshape(ext).copy()
                want = np.full(ext, np.uint32(self.fill), dtype=np.uint32)
                it = M.box_inter(*e["leave"], olo, ohi)  # the voxels that were in the window when the shift began
                if it is not None:  # (none: an earlier axis stepped by the whole size, the slab is fill only)
                    rel = tuple(slice(int(it[0][k] - lo[k]), int(it[1][k] - lo[k]) + 1) for k in range(3))
                    want[rel] = w.box(*it)
                assert np.array_equal(got, want), (i, lo, hi)
                if it is not None:
                    self.store[w.sl(*it)] = got[rel]
                self.slab_voxels.append(int(np.prod(ext)))
        finally:
            assert L.ws_shift_end(ticket) == 0, "ws_shift_end"

    def check(self, w):
        check_device(self.t, w)

    def finish(self, w):
        assert np.array_equal(self.store, w.store), (self.store, w.store)


CW = 64 ** 3


class StoreRoute:
    """TSDFMapping.shift_map_device with a DeviceGlobalMap"""

    def __init__(self, size, segment_chunks=0, max_chunks=0, base=None):
        import warpsense_amd as W
        self.lm = W.LocalMap(*size, TAU, 0)
        assert tuple(self.lm.size) == tuple(size), (tuple(self.lm.size), tuple(size))
        if base is not None:  # the window starts there: through the parameters, before the device map exists
            self.lm.pos[:] = base
            self.lm.offset[:] = M.model_offset(size, base)
        self.store = W.DeviceGlobalMap(TAU, 0, max_chunks=max_chunks, segment_chunks=segment_chunks)
        self.tm = W.TSDFMapping(_params(size), self.lm, device_global_map=self.store)
        self.t = self.tm.tsdf()

    def insert(self, lo, hi, words):
        self.t.avg_map().insert_box(lo, hi, words)

    def shift(self, w, new_pos):
        self.tm.shift_map_device(new_pos)

    def check(self, w):
        check_device(self.t, w)
        assert np.array_equal(self.lm.pos, w.pos) and np.array_equal(self.lm.offset, w.offset()), (self.lm.pos, w.pos, self.lm.offset, w.offset())

    def chunks(self):
        return {key: self.store.chunk(key) for key in self.store.keys()}

    def finish(self, w):
        chunks = self.chunks()
        w.check_chunks(chunks)
        return chunks


def store_state(store):
    keys = store.keys()
    return keys, [store.chunk(k) for k in keys]


def same_store(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def chunk_box(key, lo, hi):
    """chunk-and-box as (slices of the chunk, world lo, world hi), None if they do not meet"""
    base = np.asarray(key, dtype=np.int64) * 64
    it = M.box_inter(base, base + 63, np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64))
    if it is None:
        return None
    return tuple(slice(int(it[0][k] - base[k]), int(it[1][k] - base[k]) + 1) for k in range(3)), it[0], it[1]
