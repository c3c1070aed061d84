"""ws_map_view_gain — the view gain of a device map (the rules are stated in include/warpsense_hip.h) against the numpy model of
view_gain_model.py, applied to the world-order box of the window's entries.  Every comparison is on the raw bytes of the view records
and the ray records.  Every scene is checked on the CPU before the device is asked (view_gain_scenes.check_scene; the same conditions
run in test_view_gain_host.py without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import query_domain_scenes as QD
import raycast_model as R
import view_gain_model as VM
import view_gain_scenes as VS
from query_model import same, window
from view_gain_scenes import MW, RES, TAU

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5


def make_window(boxes, pos, offset, res=RES):
    """a TSDFCuda whose two maps hold `boxes` (world order, first voxel window(size, pos)[0]) in a ring rotated by `offset`"""
    size = boxes[0].shape
    lo, hi = window(size, pos)
    ax = [(np.arange(lo[k], hi[k] + 1, dtype=np.int64) - pos[k] + offset[k] + size[k]) % size[k] for k in range(3)]
    raws = []
    for b in boxes:
        data = np.zeros(size, dtype=np.uint32)
        data[np.ix_(ax[0], ax[1], ax[2])] = b
        raws.append(data.reshape(-1))
    t, _ = R.upload(size, pos, offset, raws, tau=TAU, mw=MW, res=res)
    assert np.array_equal(t.avg_map().extract_box(lo, hi).reshape(size), boxes[0])  # the ring holds the box
    return t, lo, hi


def p(v):
    return None if v is None else v.ctypes.data_as(C.c_void_p)


def raw_call(t, which, lo, hi, o, d, rng, min_value, flags, best=True, m=None, n=None):
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    o, d = (None if v is None else np.ascontiguousarray(v, dtype=np.int32).reshape(-1, 3) for v in (o, d))
    out = C.c_uint64(77)
    rc = t._L.ws_map_view_gain(t.handle, which, p(a), p(b), p(o), len(o) if m is None else m, p(d), len(d) if n is None else n, rng, min_value, flags,
                               C.byref(out) if best else None)
    return rc, out.value


def download(t, rays=True):
    m, r = C.c_size_t(0), C.c_size_t(0)
    assert t._L.ws_map_view_gain_download(t.handle, None, None, 0, 0, C.byref(m), C.byref(r)) == 0
    rec, ray = np.zeros(m.value, dtype=VM.RECORD), np.zeros(r.value, dtype=VM.RAY)
    assert t._L.ws_map_view_gain_download(t.handle, p(rec), p(ray) if rays and r.value else None, m.value, r.value, C.byref(m), C.byref(r)) == 0
    return rec, ray


# ------------------------------------------------------------------------------------------------ 1. random windows
@pytest.mark.parametrize("size", VS.SIZES, ids=lambda s: "x".join(map(str, s)))
def test_random_windows_match_the_model(size):
    boxes = VS.window_boxes(size)
    t, lo, hi = make_window(boxes, VS.POS, VS.OFFSET)
    o, d = VS.views(size), VS.fan()
    try:
        for which in (0, 1):
            w = t.avg_map() if which == 0 else t.new_map()
            for rng in VS.RANGES:
                for min_value in VS.MIN_VALUES:
                    for flags in VS.FLAG_SETS:
                        any_weight = flags == VS.ANY_WEIGHT
                        walk = VM.march(boxes[which], lo, RES, o, d, rng, min_value, any_weight)
                        if rng == 3000:
                            for n in (63, 64, 65, 1034):
                                VS.check_scene(walk, n)
                        for m in VS.M_VALUES:
                            for n in VS.N_VALUES:
                                want = VM.records(walk, m, n)
                                got = w.view_gain(o[:m], d[:n], rng, min_value=min_value, any_weight=any_weight, rays=flags == VS.RAYS)
                                case = (size, which, rng, min_value, flags, m, n)
                                if flags == VS.RAYS:
                                    assert same(got[0], want[0]) and same(got[1], want[1]), case
                                else:
                                    assert same(got, want[0]), case
                                assert w.last_view_gain["best_unknown_k2"] == int(want[0]["unknown_k2"].max()), case
        # the device tensors alias the same bytes
        rec, ray = t.avg_map().view_gain(o[:3], d[:65], 3000, rays=True, device=True)
        want = VM.model(boxes[0], lo, RES, o[:3], d[:65], 3000)
        assert same(rec.cpu().numpy().view(np.uint8).reshape(-1).view(VM.RECORD), want[0])
        assert same(ray.cpu().numpy().view(np.uint8).reshape(-1).view(VM.RAY).reshape(3, 65), want[1])
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 2. the rotated ring
def test_after_real_shifts_of_the_window_with_an_explicit_box_and_the_null_box():
    """the ring rotated by the map's own shifts (the sequence of test_rotated_rings_after_the_shift_sequence); the scene goes in
    through ws_map_insert_box afterwards"""
    import warpsense_amd as W
    size = (21, 19, 23)
    lm = W.LocalMap(*size, TAU, 0)
    params = W.Params(W.MapParams(resolution=RES, max_distance=TAU / 1000.0, max_weight=10, size=tuple(s * RES / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    for new_pos in [(3, 0, 0), (3, -4, 2), (10, -4, 2), (10, 5, -3), (-2, 5, -3)]:
        tm.shift_map(new_pos)
    pos = (-2, 5, -3)
    box = VS.window_boxes(size)[0]
    lo, hi = window(size, pos)
    avg = tm.tsdf().avg_map()
    avg.insert_box(lo, hi, box.reshape(-1))
    off = np.zeros(3, np.int32)
    tm.tsdf()._L.ws_map_get_params(tm.tsdf().handle, 0, None, None, p(off))
    assert all(0 < int(v) < s for v, s in zip(off, size)), off  # all offsets non-zero: the seam lies inside the window
    o, d = VS.views(size, pos=pos), VS.fan()
    walk = VM.march(box, lo, RES, o, d, 3000)
    VS.check_scene(walk, 1034)
    got = avg.view_gain(o, d, 3000, rays=True)
    want = VM.records(walk)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert same(tm.view_gain(positions_m=o.astype(np.float64) / 1000.0, fan=d, max_range_m=3.0), want[0])
    blo, bhi = lo + (2, 3, 1), hi - (4, 1, 5)  # an explicit box smaller than the window: the rest counts for nothing
    sub = box[2:size[0] - 4, 3:size[1] - 1, 1:size[2] - 5]
    walk = VM.march(sub, blo, RES, o, d, 3000)
    VS.check_scene(walk, 1034)
    got = avg.view_gain(o, d, 3000, lo=blo, hi=bhi, rays=True)
    want = VM.records(walk)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert same(avg.view_gain(o, d, 3000, lo=lo, hi=hi), VM.model(box, lo, RES, o, d, 3000)[0])


# ------------------------------------------------------------------------------------------------ 3. resolutions and far origins
@pytest.mark.parametrize("res", [2, 51, 64])
@pytest.mark.parametrize("sign", [1, -1])
def test_other_resolutions_with_origins_at_the_edge_of_int32(res, sign):
    """|o| + max_range + 2 res == INT32_MAX exactly on x, the window around it (2 mm is the smallest resolution a window admits; the
    store test runs 1 mm)"""
    pos, box, lo, o, d, rng = VS.edge_scene(res, sign)
    t, _ = R.upload(QD.SIZE, pos, QD.OFF, QD.entries(), res=res)
    try:
        walk = VM.march(box, lo, res, o, d, rng)
        VS.check_scene(walk, len(d), outside_origins=False)
        got = t.avg_map().view_gain(o, d, rng, rays=True)
        want = VM.records(walk)
        assert same(got[0], want[0]) and same(got[1], want[1])
        beyond = o[0].copy()
        beyond[0] += sign
        before = download(t)
        assert raw_call(t, 0, None, None, beyond[None], d, rng, 0, 0)[0] == WS_ERR_RANGE
        after = download(t)
        assert same(before[0], after[0]) and same(before[1], after[1])
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 4. refusals, repeats, other queries
@pytest.fixture(scope="module")
def small_window():
    size = VS.SIZES[0]
    boxes = VS.window_boxes(size)
    t, lo, hi = make_window(boxes, VS.POS, VS.OFFSET)
    yield t, lo, hi, boxes, VS.views(size), VS.fan()
    t.close()


def test_every_refusal_leaves_the_last_result(small_window):
    t, lo, hi, boxes, o, d = small_window
    assert raw_call(t, 0, None, None, o[:3], d[:65], 3000, 0, VS.RAYS)[0] == 0
    before = download(t)
    assert len(before[0]) == 3 and len(before[1]) == 3 * 65
    big_m, big_n = np.zeros((65536, 3), np.int32), np.ones((2 ** 19 + 1, 3), np.int32)
    cases = [
        ("max_range 0", raw_call(t, 0, None, None, o, d, 0, 0, 0), WS_ERR_INVALID),
        ("max_range < 0", raw_call(t, 0, None, None, o, d, -5, 0, 0), WS_ERR_INVALID),
        ("unknown flag", raw_call(t, 0, None, None, o, d, 3000, 0, 4), WS_ERR_INVALID),
        ("bad which", raw_call(t, 2, None, None, o, d, 3000, 0, 0), WS_ERR_INVALID),
        ("m == 0 and a result asked for", raw_call(t, 0, None, None, o, d, 3000, 0, 0, m=0), WS_ERR_INVALID),
        ("one NULL box pointer", raw_call(t, 0, lo, None, o, d, 3000, 0, 0), WS_ERR_INVALID),
        ("box outside the window", raw_call(t, 0, lo - 1, hi, o, d, 3000, 0, 0), WS_ERR_INVALID),
        ("hi < lo", raw_call(t, 0, hi, lo, o, d, 3000, 0, 0), WS_ERR_INVALID),
        ("NULL origins", raw_call(t, 0, None, None, None, d, 3000, 0, 0, m=3), WS_ERR_INVALID),
        ("NULL directions", raw_call(t, 0, None, None, o, None, 3000, 0, 0, n=3), WS_ERR_INVALID),
        ("min_value < 0", raw_call(t, 0, None, None, o, d, 3000, -1, 0), WS_ERR_RANGE),
        ("min_value > 32767", raw_call(t, 0, None, None, o, d, 3000, 32768, 0), WS_ERR_RANGE),
        ("K > 8191", raw_call(t, 0, None, None, o, d, 8192 * (RES // 2), 0, 0), WS_ERR_RANGE),
        ("n > 2^19", raw_call(t, 0, None, None, o, big_n, 3000, 0, 0), WS_ERR_RANGE),
        ("m > 65535", raw_call(t, 0, None, None, big_m, d, 3000, 0, 0), WS_ERR_RANGE),
        ("m n > 2^27 with rays", raw_call(t, 0, None, None, big_m[:1025], big_n[:2 ** 17], 3000, 0, VS.RAYS), WS_ERR_RANGE),
        ("origin does not fit", raw_call(t, 0, None, None, [[2 ** 31 - 1 - 3000 - 2 * RES + 1, 0, 0]], d, 3000, 0, 0), WS_ERR_RANGE),
    ]
    for name, (rc, best), want in cases:
        assert rc == want and best == 77, (name, rc, best)
        after = download(t)
        assert same(before[0], after[0]) and same(before[1], after[1]), name
    # no view or no ray otherwise: WS_OK, nothing written
    assert raw_call(t, 0, None, None, o, d, 3000, 0, 0, n=0) == (0, 77)
    assert raw_call(t, 0, None, None, o, d, 3000, 0, 0, m=0, best=False)[0] == 0
    after = download(t)
    assert same(before[0], after[0]) and same(before[1], after[1])
    # K = 8191 is admitted; asking for rays that the last call did not write is refused
    assert raw_call(t, 0, None, None, o[:1], d[:2], 8191 * (RES // 2), 0, 0)[0] == 0
    m, r = C.c_size_t(0), C.c_size_t(0)
    ray = np.zeros(2, dtype=VM.RAY)
    assert t._L.ws_map_view_gain_download(t.handle, None, p(ray), 0, 2, C.byref(m), C.byref(r)) == WS_ERR_INVALID


def test_two_calls_give_the_same_bytes_and_no_query_disturbs_another(small_window):
    t, lo, hi, boxes, o, d = small_window
    avg = t.avg_map()
    first = avg.view_gain(o, d, 3000, rays=True)
    again = avg.view_gain(o, d, 3000, rays=True)
    assert same(first[0], again[0]) and same(first[1], again[1])
    origin = o[0]
    fr, rc = avg.frontier(), avg.raycast(origin, d, 3000)[0]
    held = download(t)
    assert same(held[0], first[0]) and same(held[1].reshape(first[1].shape), first[1])  # frontier and ray cast left the result alone
    f_dev, cnt = avg.frontier(device=True), C.c_size_t(0)
    avg.raycast(origin, d, 3000)
    avg.view_gain(o[:3], d[:64], 20)
    assert same(f_dev.cpu().numpy().view(np.uint8).reshape(-1), fr.view(np.uint8).reshape(-1))  # and the view gain left theirs alone
    got = np.zeros(len(d), dtype=R.RAY)
    assert t._L.ws_map_raycast_download(t.handle, p(got), None, len(d), C.byref(cnt)) == 0 and same(got, rc)
    timing = avg.view_gain_timing(1)
    avg.view_gain(o, d, 3000)
    timing = avg.view_gain_timing(0)
    assert len(timing) == 3 and all(v >= 0 for v in timing) and timing[1] > 0


# ------------------------------------------------------------------------------------------------ 5. mapping level
def test_next_best_view_after_one_scan_of_the_synthetic_room():
    """the scene of test_view_gain_host.test_on_the_oracles_map_the_next_best_view_sees_more_than_staying_put, where the order is shown
    on the oracle's map of the same scan"""
    import warpsense_amd as W
    size = VS.ROOM_SIZE
    lm = W.LocalMap(*size, TAU, 0)
    params = W.Params(W.MapParams(resolution=RES, max_distance=TAU / 1000.0, max_weight=10, size=tuple(s * RES / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    pose = np.eye(4)
    tm.update_tsdf(VS.room_scan(), pose=pose)
    fan = VS.room_fan()
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    tm.tsdf().avg_map().to_host(host)
    lo, hi = lm.window()
    box = host.data_.reshape(size)[np.ix_(*[(np.arange(lo[k], hi[k] + 1) - lm.pos[k] + lm.offset[k] + lm.size[k]) % lm.size[k] for k in range(3)])]
    a, cand, goals, records, order = VS.next_view_model(box, lo)
    at_a = tm.view_gain(poses=pose[None], fan=fan, max_range_m=VS.ROOM_RANGE_MM / 1000.0)
    assert same(at_a, a)
    nbv = tm.next_best_view(seed_mm=[VS.ROOM_SEED_MM], clearance_m=VS.ROOM_CLEARANCE_M, fan=fan, max_range_m=VS.ROOM_RANGE_MM / 1000.0, min_size=VS.ROOM_MIN_SIZE)
    assert len(cand) >= 2 and np.array_equal(nbv["candidates"], cand) and np.array_equal(nbv["goal"][cand], goals)
    assert same(nbv["records"], records) and np.array_equal(nbv["order"], order) and nbv["winner"] == int(cand[order[0]])
    assert tuple(nbv["path"][0][["x", "y", "z"]].tolist()) == tuple(int(v) for v in goals[order[0]]) and nbv["header"]["status"] == 0
    assert tuple(nbv["path"][-1][["x", "y", "z"]].tolist()) == tuple(int(v) // RES for v in VS.ROOM_SEED_MM) and nbv["path"][-1]["cost"] == 0
    winner = int(nbv["records"]["unknown_k2"][nbv["order"][0]])
    print("A", int(at_a["unknown_k2"][0]), "winner", winner, "candidates", len(cand))
    assert winner > int(at_a["unknown_k2"][0])  # going there shows more unknown volume than staying put
