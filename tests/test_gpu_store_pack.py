"""ws_store_pack / ws_store_unpack — the chunks of a global map in device memory into their packed form and back (the format is stated
in include/warpsense_hip.h) against the numpy model of pack_model.py.  Every comparison is byte for byte: headers, payload, the four
statistics, and the chunks of the store an unpack wrote."""
import ctypes as C

import numpy as np
import pytest

import fuse_scenes as S
import pack_model as PM
import pack_scenes as PS
import two_store_scenes as T
import warpsense_amd as W
from warpsense_amd._abi import _ptr

pytestmark = pytest.mark.gpu

WS_ERR_INVALID, WS_ERR_CAPACITY = -1, -4
FILL = (600, 0)  # PM.FILL as (value, weight)


def make(chunks, **kw):
    return S.make_store(chunks, fill=FILL, **kw)


def same(packed, want):
    headers, payload, stats = want
    assert packed.headers.tobytes() == headers.tobytes(), (packed.headers[:, :8], headers[:, :8])
    assert packed.payload.tobytes() == payload.tobytes() and packed.stats == tuple(stats) and packed.fill == int(PM.FILL)
    return True


@pytest.fixture(scope="module")
def cases():
    """the store of the twelve brick cases (keys negative and at both key ends), the model's stream over it, and its pack"""
    chunks = PM.case_store()
    store = make(chunks)
    return dict(chunks=chunks, store=store, want=PM.pack(chunks, PM.FILL), packed=store.pack())


def test_an_empty_store():
    store = make({})
    p = store.pack()
    assert p.n_chunks == 0 and p.payload_words == 0 and p.stats == (0, 0, 0, 0) and p.ratio == 0.0
    other = make({(1, 1, 1): PM.brick_cases()["random"]})
    other.unpack(p)  # nothing listed: nothing changes
    assert other.keys() == [(1, 1, 1)] and other.chunk((1, 1, 1)).tobytes() == PM.brick_cases()["random"].tobytes()


@pytest.mark.parametrize("name", sorted(PM.brick_cases()))
def test_each_brick_case_alone(name):
    chunks = {PM.CASE_KEYS[name]: PM.brick_cases()[name]}
    store = make(chunks)
    for direct in (False, True):
        assert same(store.pack(direct=direct), PM.pack(chunks, PM.FILL))
    assert store.chunk(PM.CASE_KEYS[name]).tobytes() == chunks[PM.CASE_KEYS[name]].tobytes()  # the store is only read


def test_all_cases_in_one_store_and_twice_the_same_bytes(cases):
    assert same(cases["packed"], cases["want"]) and cases["packed"].n_chunks == 12
    assert all(v > 0 for v in cases["packed"].stats) and 0 < cases["packed"].ratio < 1
    again, direct = cases["store"].pack(), cases["store"].pack(direct=True)
    for p in (again, direct):
        assert same(p, cases["want"])
    cases["packed"].check()
    assert S.read(cases["store"]).keys() == cases["chunks"].keys() and all(S.read(cases["store"])[k].tobytes() == c.tobytes() for k, c in cases["chunks"].items())


def test_a_key_subset_in_descending_order(cases):
    keys = sorted(cases["chunks"], reverse=True)[1::2]
    assert same(cases["store"].pack(keys=keys), PM.pack(cases["chunks"], PM.FILL, keys))
    one = [PM.CASE_KEYS["single_first"]]  # a key end alone
    assert same(cases["store"].pack(keys=one), PM.pack(cases["chunks"], PM.FILL, one))


def test_absent_and_repeated_keys_are_refused_and_the_last_result_stays(cases):
    store, L = cases["store"], cases["store"]._L
    want = PM.pack(cases["chunks"], PM.FILL)
    assert same(store.pack(), want)
    n, words = C.c_size_t(7), C.c_uint64(7)
    for keys in ([(0, 0, 0), (9, 9, 9)], [(0, 0, 0), (5, 5, 5), (0, 0, 0)]):
        k = np.asarray(keys, dtype=np.int32)
        assert L.ws_store_pack(store.handle, _ptr(k), len(k), 0, C.byref(n), C.byref(words), None) == WS_ERR_INVALID
    assert L.ws_store_pack(store.handle, None, 0, 2, C.byref(n), C.byref(words), None) == WS_ERR_INVALID  # an unknown flag bit
    headers, payload = np.zeros_like(want[0]), np.zeros_like(want[1])
    assert L.ws_store_pack_download(store.handle, _ptr(headers), _ptr(payload), len(headers), len(payload), C.byref(n), C.byref(words)) == 0
    assert (n.value, words.value) == (12, len(want[1])) and headers.tobytes() == want[0].tobytes() and payload.tobytes() == want[1].tobytes()


def test_a_download_capacity_too_small_reports_the_sizes(cases):
    store, L = cases["store"], cases["store"]._L
    want = PM.pack(cases["chunks"], PM.FILL)
    store.pack()
    headers, payload = np.zeros_like(want[0]), np.zeros_like(want[1])
    for cap_c, cap_w in ((11, len(payload)), (12, len(payload) - 1), (0, 0)):
        n, words = C.c_size_t(0), C.c_uint64(0)
        assert L.ws_store_pack_download(store.handle, _ptr(headers), _ptr(payload), cap_c, cap_w, C.byref(n), C.byref(words)) == WS_ERR_CAPACITY
        assert (n.value, words.value) == (12, len(payload)) and not headers.any() and not payload.any()
    # the device pointers carry the same counts
    n, words = C.c_size_t(0), C.c_uint64(0)
    assert L.ws_store_pack_headers_dev(store.handle, C.byref(n)) and L.ws_store_pack_payload_dev(store.handle, C.byref(words)) and (n.value, words.value) == (12, len(payload))


def test_an_aged_store_of_two_chunk_segments():
    """five chunks after puts and drops: the slots are neither in key order nor fresh, and span three segments"""
    chunks = {k: PM.case_store()[k] for k in sorted(PM.case_store())[:4]}
    chunks[(2, -2, 2)] = T.observed(77)
    store, record = T.aged_store(chunks, 2, 5, fill=FILL)
    T.check_record(record, 5, 2)
    assert same(store.pack(), PM.pack(chunks, PM.FILL))


def unlike_target():
    """a store with another default, one-chunk segments and a history: three chunks of its own, one under a key of the source"""
    own = {(7, 7, 7): T.observed(91), (0, 0, 1): T.observed(92), (-9, 0, 0): T.observed(93)}
    store, record = T.aged_store(own, 1, 1, fill=(-32768, 3))
    T.check_record(record, 3, 1)
    return own, store


def test_unpack_into_an_unlike_store(cases):
    own, dst = unlike_target()
    keys = [k for k in sorted(cases["chunks"]) if k != (0, -1, 0)]  # all but one
    dst.unpack(cases["store"].pack(keys=keys))
    got = S.read(dst)
    assert sorted(got) == sorted(set(keys) | set(own))
    for k in keys:  # byte-exact though the stores' defaults differ: default bricks get the fill of the pack
        assert got[k].tobytes() == cases["chunks"][k].tobytes(), k
    for k in ((7, 7, 7), (-9, 0, 0)):  # not listed: unchanged
        assert got[k].tobytes() == own[k].tobytes(), k
    assert dst.pack_timing() == (0.0, 0.0, 0.0)  # (the events are off)


def test_unpack_dev_and_clone_give_the_same(cases):
    src = cases["store"]
    _, a = unlike_target()
    _, b = unlike_target()
    a.unpack(src.pack())
    p = src.pack(device=True)
    assert p.on_device and p.payload.is_cuda and p.payload_words == len(cases["want"][1])
    b.unpack(p)
    c = src.clone()
    ra, rb, rc = S.read(a), S.read(b), S.read(c)
    assert sorted(ra) == sorted(rb) and all(ra[k].tobytes() == rb[k].tobytes() for k in ra)
    assert sorted(rc) == sorted(cases["chunks"]) and c.default_raw == src.default_raw and all(rc[k].tobytes() == cases["chunks"][k].tobytes() for k in rc)
    assert same(c.pack(), cases["want"])


def test_a_corrupted_stream_and_a_full_store_change_nothing(cases):
    own, dst = unlike_target()
    before = S.read(dst)
    p = cases["store"].pack()
    for col, delta in ((7, 1), (5, 1), (3, 1), (8, 3)):
        bad = W.PackedMap(p.headers.copy(), p.payload, p.fill)
        bad.headers[4, col] = bad.headers[4, col] + delta if col != 8 else bad.headers[4, col] | delta
        with pytest.raises(W.WsError, match="status -1"):
            dst.unpack(bad)
    with pytest.raises(W.WsError, match="status -1"):
        dst.unpack(W.PackedMap(p.headers, p.payload[:-1], p.fill))
    with pytest.raises(W.WsError, match="status -1"):
        dst.unpack(W.PackedMap(p.headers[::-1], p.payload, p.fill))
    small_own = {(7, 7, 7): T.observed(91), (0, 0, 1): T.observed(92)}
    small = S.make_store(small_own, max_chunks=13, fill=(-32768, 3))  # 2 + 12 - 1 shared = 13 fit; one more does not
    small.unpack(p)
    assert small.count() == 13
    small2 = S.make_store(small_own, max_chunks=12, fill=(-32768, 3))
    with pytest.raises(W.WsError, match="status -4"):
        small2.unpack(p)
    for store, want in ((dst, before), (small2, small_own)):
        got = S.read(store)
        assert sorted(got) == sorted(want) and all(got[k].tobytes() == want[k].tobytes() for k in want)


def same_chunks(store, sc, keys):
    for k in keys:
        assert store.chunk(k).tobytes() == sc["chunks"][k].tobytes(), (k, sc["names"][k])
    return True


@pytest.fixture(scope="module")
def aged130():
    """130 chunks (three waves of the scan) in a store of four-chunk segments whose slots are neither fresh nor in key order: the
    chunks at the odd places go in first, five of them are dropped, then all go in, the absent ones into the freed and the new slots"""
    sc = PS.scene(130)
    store = W.DeviceGlobalMap(FILL[0], FILL[1], segment_chunks=4)
    first = sc["keys"][1::2]
    h, p, _ = PS.stream(sc, first)
    store.unpack(W.PackedMap(h, p, int(PM.FILL)))
    assert store.keys() == first and same_chunks(store, sc, first[::13])
    dropped = first[3::14]
    assert len(dropped) == 5
    for k in dropped:
        store.drop_chunk(k)
    assert store.count() == 60
    want = PS.stream(sc)
    store.unpack(W.PackedMap(want[0], want[1], int(PM.FILL)))
    d = T.Directory(4)  # the same history on the replay of the directory rules
    d.create(first)
    for k in dropped:
        d.drop(k)
    d.create(sc["keys"])
    mixed, reused, spans = T.claims(d, sc["keys"])
    assert mixed and reused == 5 and spans == 33 and store.capacity() == d.capacity() == 132
    yield dict(scene=sc, store=store, want=want)
    store.close()


def test_130_chunks_in_aged_slots(aged130):
    sc, store, want = aged130["scene"], aged130["store"], aged130["want"]
    assert store.count() == 130 and store.keys() == sc["keys"]
    got = S.read(store)
    assert sorted(got) == sc["keys"] and all(got[k].tobytes() == sc["chunks"][k].tobytes() for k in sc["keys"])
    assert same(store.pack(), want) and same(store.pack(direct=True), want)
    rng = np.random.default_rng(70)
    keys = sorted((sc["keys"][i] for i in rng.choice(130, 70, replace=False)), reverse=True)
    assert len(set(keys)) == 70 and same(store.pack(keys=keys), PM.pack(sc["chunks"], PM.FILL, keys))


def test_a_small_result_after_a_large_one(aged130):
    """the buffers of a pack are kept: a later, smaller result must not show what an earlier one left in them"""
    sc, store, L = aged130["scene"], aged130["store"], aged130["store"]._L
    by_name = lambda name: next(k for k in sc["keys"] if sc["names"][k] == name)
    assert same(store.pack(), aged130["want"])
    p = store.pack(keys=[by_name("all_fill")])
    assert same(p, PM.pack(sc["chunks"], PM.FILL, [by_name("all_fill")])) and p.n_chunks == 1 and p.payload_words == 0 and p.stats == (512, 0, 0, 160)
    words = C.c_uint64(7)
    assert not L.ws_store_pack_payload_dev(store.handle, C.byref(words)) and words.value == 0
    n = C.c_size_t(7)
    assert L.ws_store_pack_headers_dev(store.handle, C.byref(n)) and n.value == 1
    one = [by_name("random")]
    assert same(store.pack(keys=one), PM.pack(sc["chunks"], PM.FILL, one)) and same(store.pack(keys=one, direct=True), PM.pack(sc["chunks"], PM.FILL, one))


def test_1030_chunks_through_unpack_and_pack():
    """more chunks than one round of the scan (1024), about 1 GiB of store: the model's stream in, the same bytes out; then the
    payload stays on the device, into a second store and back into the store it came from"""
    import time
    t0 = time.perf_counter()
    sc = PS.scene(1030)
    want = PS.stream(sc)
    store, second = make({}, segment_chunks=0), make({}, segment_chunks=0)
    try:
        store.unpack(W.PackedMap(want[0], want[1], int(PM.FILL)))
        assert store.count() == 1030 and store.keys() == sc["keys"]
        assert same(store.pack(), want)
        rng = np.random.default_rng(1030)
        ends = [0, 1, 63, 64, 1023, 1024, 1029]
        places = ends + sorted(int(i) for i in rng.choice([i for i in range(1030) if i not in ends], 24, replace=False))
        assert len(set(places)) == 31 and same_chunks(store, sc, [sc["keys"][i] for i in places])
        p = store.pack(device=True)
        assert p.on_device and p.payload_words == len(want[1]) and p.headers.tobytes() == want[0].tobytes()
        second.unpack(p)
        assert second.count() == 1030 and same(second.pack(), want)
        store.unpack(store.pack(device=True))
        assert store.count() == 1030 and same(store.pack(), want)
    finally:
        store.close(), second.close()
    print("1030 chunks: %.2f s, %.1f MB of payload" % (time.perf_counter() - t0, 4e-6 * len(want[1])))


def test_pack_timing_reports_three_passes_then_the_unpack(cases):
    store = cases["store"]
    store.pack_timing(1)
    store.pack()
    ms = store.pack_timing()
    assert all(0 < v < 1000 for v in ms), ms
    dst = make({})
    dst.pack_timing(1)
    dst.unpack(store.pack())
    ms = dst.pack_timing(0)
    assert 0 < ms[0] < 1000 and ms[1:] == (0.0, 0.0), ms
    store.pack_timing(0)


def test_end_to_end_window_scan_shift_file(tmp_path):
    """a small odd window takes one synthetic scan and is shifted on the device: chunks with surface, free space and unseen space;
    pack, file, a fresh store: surface() and mesh() of both stores are byte-equal"""
    import store_scenes as SM
    from window_routes import _params
    from warpsense_amd import synthetic as SY
    size, res, tau = (67, 61, 35), SM.RES, SM.TAU
    store = W.DeviceGlobalMap(tau, 0, segment_chunks=4)
    tm = W.TSDFMapping(_params(size), W.LocalMap(*size, tau, 0), device_global_map=store)
    room = dict(rings=32, azimuths=256, half_extents_mm=(1700.0, 1300.0, 900.0))
    tm.update_tsdf(np.rint(SY.os1_128_scan(sensor_mm=(0.0, 0.0, 0.0), seed=30, **room)).astype(np.int32), pos_rm=np.zeros(3, dtype=np.int32), up_rm=(0, 0, 32768))
    tm.shift_map_device((9, -5, 2))
    path = str(tmp_path / "run.wspk")
    packed = tm.save_global_packed(path)
    print("end to end:", packed.n_chunks, "chunks", packed.stats, "ratio %.4f" % packed.ratio)
    # (after ONE scan the weights of free space still vary with the distance: no brick is uniform yet; unseen space is default)
    assert packed.n_chunks >= 2 and packed.stats[0] > 0 and packed.stats[2] > 0 and packed.ratio < 0.9
    fresh = W.DeviceGlobalMap(-5, 1, segment_chunks=1)
    loaded = fresh.load_packed(path)
    assert (loaded.resolution, loaded.tau) == (res, tau) and fresh.keys() == store.keys()
    a, b = store.surface(tau, res), fresh.surface(tau, res)
    assert len(a) > 100 and a.tobytes() == b.tobytes()
    (va, fa), (vb, fb) = store.mesh(res), fresh.mesh(res)
    assert len(fa) > 100 and va.tobytes() == vb.tobytes() and fa.tobytes() == fb.tobytes()
    model = PM.pack(S.read(store), np.uint32(store.default_raw))
    assert packed.headers.tobytes() == model[0].tobytes() and packed.payload.tobytes() == model[1].tobytes()
    store.close(), fresh.close()
