"""ws_store_view_gain — the view gain of the chunk store against the numpy model of view_gain_model.py on the assembled chunks: a voxel
of the box in an absent chunk is UNKNOWN.  Every comparison is on raw bytes; every scene is checked on the CPU first."""
import ctypes as C

import numpy as np
import pytest

import store_scenes as SM
import view_gain_model as VM
import view_gain_scenes as VS
from query_model import same, window
from view_gain_scenes import RES

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5


@pytest.mark.parametrize("scene", VS.store_scenes(), ids=lambda s: s[0].replace(" ", "_").replace(",", ""))
def test_chunk_scenes_match_the_model(scene):
    name, chunks, lo, hi, o, d, rng = scene
    box = SM.assemble(chunks, lo, hi)
    store = SM.make_store(chunks)
    try:
        for min_value, any_weight in [(0, False), (1000, False), (0, True)]:
            walk = VM.march(box, lo, RES, o, d, rng, min_value, any_weight)
            if min_value == 0 and not any_weight:
                if len(d) >= 63:
                    VS.check_scene(walk, len(d), outside_origins=False)
                assert VS.absent_ray_count(walk, chunks, lo, hi, RES, o, d, rng) >= 1
            want = VM.records(walk)
            got = store.view_gain(RES, o, d, rng, lo=lo, hi=hi, min_value=min_value, any_weight=any_weight, rays=True)
            assert same(got[0], want[0]) and same(got[1], want[1]), (name, min_value, any_weight)
            assert store.last_view_gain["best_unknown_k2"] == int(want[0]["unknown_k2"].max())
            assert same(store.view_gain(RES, o, d, rng, lo=lo, hi=hi, min_value=min_value, any_weight=any_weight), want[0])
    finally:
        store.close()


def test_the_default_box_an_empty_store_and_the_refusals():
    chunks = SM.seam_chunks()
    name, _, _, _, o, d, rng = VS.store_scenes()[0]
    store = SM.make_store(chunks)
    empty = SM.make_store({})
    try:
        lo, hi = SM.bounding_box(chunks)
        want = VM.model(SM.assemble(chunks, lo, hi), lo, RES, o, d, rng)
        got = store.view_gain(RES, o, d, rng, rays=True)  # no box: the bounding box of the present chunks
        assert same(got[0], want[0]) and same(got[1], want[1])
        # an empty store with a box: every voxel of the box is UNKNOWN; without one: every sample is outside
        blo, bhi = (-20, -20, -20), (20, 20, 20)
        want = VM.model(np.zeros((41, 41, 41), dtype=np.uint32), blo, RES, o, d, rng)
        assert same(empty.view_gain(RES, o, d, rng, lo=blo, hi=bhi), want[0]) and want[0]["unknown"].sum() > 100
        none = empty.view_gain(RES, o, d, rng)
        assert np.all(none["unknown"] == 0) and np.all(none["free"] == 0) and np.all(none["live"] == len(d) - 2)
        # resolution 1 mm (step 1): the window admits no such map, the store does
        want = VM.model(SM.assemble(chunks, lo, hi), lo, 1, o // 50, d, 70)
        assert same(store.view_gain(1, o // 50, d, 70, lo=lo, hi=hi), want[0]) and want[0]["free"].sum() + want[0]["unknown"].sum() > 100
        before = store.view_gain(RES, o, d, rng, lo=lo, hi=hi, rays=True)

        def raw(lo_, hi_, rng_, res_, min_value, flags):
            p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
            a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo_, hi_))
            best = C.c_uint64(77)
            oo, dd = np.ascontiguousarray(o, dtype=np.int32), np.ascontiguousarray(d, dtype=np.int32)
            return store._L.ws_store_view_gain(store.handle, p(a), p(b), p(oo), len(oo), p(dd), len(dd), rng_, res_, min_value, flags, C.byref(best)), best.value
        for case, want_rc in [((lo, None, rng, RES, 0, 0), WS_ERR_INVALID), ((hi, lo, rng, RES, 0, 0), WS_ERR_INVALID), ((lo, hi, rng, 0, 0, 0), WS_ERR_INVALID),
                              ((lo, hi, 0, RES, 0, 0), WS_ERR_INVALID), ((lo, hi, rng, RES, 0, 8), WS_ERR_INVALID), ((lo, hi, rng, 1025, 0, 0), WS_ERR_RANGE),
                              ((lo, hi, rng, RES, 40000, 0), WS_ERR_RANGE), ((lo, hi, 8192 * 25, RES, 0, 0), WS_ERR_RANGE)]:
            assert raw(*case) == (want_rc, 77), case
            m, r = C.c_size_t(0), C.c_size_t(0)
            rec, ray = np.zeros(len(o), dtype=VM.RECORD), np.zeros((len(o), len(d)), dtype=VM.RAY)
            pv = lambda v: v.ctypes.data_as(C.c_void_p)
            assert store._L.ws_store_view_gain_download(store.handle, pv(rec), pv(ray), len(o), ray.size, C.byref(m), C.byref(r)) == 0
            assert same(rec, before[0]) and same(ray, before[1]), case
    finally:
        store.close()
        empty.close()


@pytest.mark.parametrize("where", ["+", "-"])
def test_one_millimetre_at_the_edge_of_int32(where):
    """step = max(res / 2, 1) = 1 with |o| + max_range + 2 res == INT32_MAX exactly, across the absent chunks of the row"""
    chunks, lo, hi, o, d, rng = VS.store_edge_scene(where)
    walk = VM.march(SM.assemble(chunks, lo, hi), lo, 1, o, d, rng)
    VS.check_scene(walk, len(d), outside_origins=False)
    assert VS.absent_ray_count(walk, chunks, lo, hi, 1, o, d, rng) >= 10
    want = VM.records(walk)
    store = SM.make_store(chunks)
    try:
        got = store.view_gain(1, o, d, rng, lo=lo, hi=hi, rays=True)
        assert same(got[0], want[0]) and same(got[1], want[1])
        beyond = o.copy()
        beyond[0, 0] += 1 if where == "+" else -1
        with pytest.raises(Exception, match="status -5"):
            store.view_gain(1, beyond, d, rng, lo=lo, hi=hi)
    finally:
        store.close()


def test_sums_beyond_32_bits():
    """a ray's own sum of k^2, the wave's sum, the record and best_unknown_k2 all exceed 2^32"""
    chunks, lo, hi, o, d, rng = VS.big_sum_scene()
    want = VM.model(SM.assemble(chunks, lo, hi), lo, RES, o, d, rng)
    assert int(want[0]["unknown_k2"][0]) >= 2 ** 40
    store = SM.make_store(chunks)
    try:
        got = store.view_gain(RES, o, d, rng, lo=lo, hi=hi, rays=True)
        assert same(got[0], want[0]) and same(got[1], want[1])
        assert store.last_view_gain["best_unknown_k2"] == int(want[0]["unknown_k2"][0])
        three = store.view_gain(RES, np.concatenate([o, o + (50000, 0, 0), o - (3, 1, 2)]), d, rng, lo=lo, hi=hi)
        assert same(three[:1], want[0]) and store.last_view_gain["best_unknown_k2"] == int(three["unknown_k2"].max()) >= 2 ** 40
    finally:
        store.close()


def test_a_saved_window_gives_the_bytes_of_the_window():
    import raycast_model as R
    size = VS.SIZES[0]
    boxes = VS.window_boxes(size)
    lo, hi = window(size, VS.POS)
    ax = [(np.arange(lo[k], hi[k] + 1, dtype=np.int64) - VS.POS[k] + VS.OFFSET[k] + size[k]) % size[k] for k in range(3)]
    data = np.zeros(size, dtype=np.uint32)
    data[np.ix_(ax[0], ax[1], ax[2])] = boxes[0]
    t, _ = R.upload(size, VS.POS, VS.OFFSET, [data.reshape(-1), data.reshape(-1)], res=RES)
    store = SM.make_store({})
    try:
        store.save_box(t, lo, hi)
        o, d = VS.views(size), VS.fan()
        for flags in (dict(), dict(any_weight=True), dict(min_value=1000)):
            a = t.avg_map().view_gain(o, d, 3000, rays=True, **flags)
            b = store.view_gain(RES, o, d, 3000, lo=lo, hi=hi, rays=True, **flags)
            assert same(a[0], b[0]) and same(a[1], b[1]), flags
        assert same(a[0], VM.model(boxes[0], lo, RES, o, d, 3000, min_value=1000)[0])
    finally:
        store.close()
        t.close()
