"""ws_map_frontier — the frontier of a device map and its clusters (the rules are stated in include/warpsense_hip.h) against the numpy
model of frontier_model.py, applied to the world-order box of the window's entries (ws_map_extract_box).  Every comparison is on the
raw bytes of records, labels and cluster table.  Every scene is checked on the CPU before the device is asked."""
import ctypes as C

import numpy as np
import pytest

import frontier_model as FM
from frontier_scenes import (MW, RES, TAU, check_scene, random_box, room_box, ROOM_CLUSTERS, ROOM_RECORDS, corner_blobs, tunnel_box, u_box)
from query_model import same, window

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
ANY, CLUSTERS = 1, 2


def make_window(box, pos=(0, 0, 0), offset=None, new_box=None):
    """a TSDFCuda whose avg_map window holds `box` (world order, first voxel window(size, pos)[0]) in a ring rotated by `offset`"""
    import warpsense_amd as W
    size = box.shape
    offset = tuple(s // 2 for s in size) if offset is None else offset
    lo, hi = window(size, pos)
    ax = [(np.arange(lo[k], hi[k] + 1, dtype=np.int64) - pos[k] + offset[k] + size[k]) % size[k] for k in range(3)]

    def ring(b):
        data = np.zeros(size, dtype=np.uint32)
        data[np.ix_(ax[0], ax[1], ax[2])] = b
        return np.ascontiguousarray(data.reshape(-1))
    t = W.TSDFCuda(W.DeviceMap(size, offset, ring(box), pos), TAU, MW, RES)
    if new_box is not None:
        t.new_map().to_device(W.DeviceMap(size, offset, ring(new_box), pos))
    assert np.array_equal(t.avg_map().extract_box(lo, hi).reshape(size), box)  # the ring holds the box
    return t, lo, hi


def same3(got, want):
    return all(same(g, w) for g, w in zip(got, want)) and len(got) == len(want) == 3


def raw_call(t, which, lo, hi, min_value, flags):
    n, k = C.c_size_t(77), C.c_size_t(77)
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    rc = t._L.ws_map_frontier(t.handle, which, p(a), p(b), min_value, flags, C.byref(n), C.byref(k))
    return rc, n.value, k.value


def download(t, cap_records=None, cap_clusters=None, labels=True, table=True):
    n, k = C.c_size_t(0), C.c_size_t(0)
    assert t._L.ws_map_frontier_download(t.handle, None, None, None, 0, 0, C.byref(n), C.byref(k)) == 0
    cr, ck = n.value if cap_records is None else cap_records, k.value if cap_clusters is None else cap_clusters
    rec, lab, tab = np.zeros(cr, dtype=FM.RECORD), np.zeros(cr, dtype=np.uint32), np.zeros(ck, dtype=FM.CLUSTER)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    rc = t._L.ws_map_frontier_download(t.handle, p(rec), p(lab) if labels else None, p(tab) if table else None, cr, ck, C.byref(n), C.byref(k))
    return rc, (rec, lab, tab), n.value, k.value


# ------------------------------------------------------------------------------------------------ 1. random entries
ROTATED = dict(pos=(3, -2, 5), offset=(7, 4, 9))  # every axis of the ring wraps inside the window


@pytest.fixture(scope="module")
def random_window():
    box, new_box = random_box((20, 19, 21), seed=1), random_box((20, 19, 21), seed=2)
    t, lo, hi = make_window(box, new_box=new_box, **ROTATED)
    yield t, lo, hi, (box, new_box)
    t.close()


@pytest.mark.parametrize("any_weight", [False, True])
@pytest.mark.parametrize("min_value", [0, 1, TAU])
def test_random_entries_match_the_model(random_window, min_value, any_weight):
    t, lo, hi, boxes = random_window
    for which in (0, 1):
        want = FM.frontier(boxes[which], lo, min_value, any_weight)
        check_scene(*want)
        w = t.avg_map() if which == 0 else t.new_map()
        got = w.frontier(min_value=min_value, any_weight=any_weight, clusters=True)
        print(which, min_value, any_weight, len(want[0]), len(want[2]))
        assert same3(got, want), (which, min_value, any_weight)
        assert same(w.frontier(min_value=min_value, any_weight=any_weight), want[0])
        assert same3(w.frontier(lo=lo, hi=hi, min_value=min_value, any_weight=any_weight, clusters=True), want)


def test_after_real_shifts_of_the_window():
    """the ring rotated by the map's own shifts; the scene goes in through ws_map_insert_box afterwards"""
    import warpsense_amd as W
    size = (21, 19, 23)
    lm = W.LocalMap(*size, TAU, 0)
    params = W.Params(W.MapParams(resolution=RES, max_distance=TAU / 1000.0, max_weight=10, size=tuple(s * RES / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    for new_pos in [(3, 0, 0), (3, -4, 2), (10, -4, 2), (10, 5, -3), (-2, 5, -3)]:
        tm.shift_map(new_pos)
    box = random_box(size, seed=3)
    lo, hi = window(size, (-2, 5, -3))
    avg = tm.tsdf().avg_map()
    avg.insert_box(lo, hi, box.reshape(-1))
    assert np.array_equal(avg.extract_box(lo, hi).reshape(size), box)
    off = np.zeros(3, np.int32)
    tm.tsdf()._L.ws_map_get_params(tm.tsdf().handle, 0, None, None, off.ctypes.data_as(C.c_void_p))
    assert all(int(o) != 0 for o in off), off
    want = FM.frontier(box, lo)
    check_scene(*want)
    assert same3(tm.frontier(clusters=True), want) and same(tm.frontier(), want[0])


# ------------------------------------------------------------------------------------------------ 2. the hollow room
def test_hollow_room_with_holes_in_its_walls():
    box = room_box()
    t, lo, hi = make_window(box, pos=(-4, 6, 1), offset=(3, 17, 8))
    try:
        want = FM.frontier(box, lo, TAU)
        check_scene(*want)
        assert len(want[0]) == ROOM_RECORDS and len(want[2]) == ROOM_CLUSTERS  # one cluster per hole, its area in voxels
        assert sorted(want[2]["count"].tolist()) == sorted([64, 49, 48, 25, 9, 16, 9])
        got = t.avg_map().frontier(min_value=TAU, clusters=True)
        assert same3(got, want)
        assert raw_call(t, 0, None, None, TAU, CLUSTERS) == (0, ROOM_RECORDS, ROOM_CLUSTERS)
        assert raw_call(t, 0, None, None, TAU, 0) == (0, ROOM_RECORDS, 0)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 3. component shapes
@pytest.mark.parametrize("gap", [0, 1])
def test_blobs_at_a_corner_and_one_voxel_apart(gap):
    box = corner_blobs(gap)
    t, lo, hi = make_window(box, pos=(1, 2, 3), offset=(2, 11, 5))
    try:
        want = FM.frontier(box, lo)
        assert len(want[2]) == 1 + gap and len(want[0]) >= 50
        assert same3(t.avg_map().frontier(clusters=True), want)
    finally:
        t.close()


def test_a_long_zigzag_tunnel_is_one_cluster():
    box, length = tunnel_box()
    t, lo, hi = make_window(box, pos=(0, 0, 0), offset=(13, 29, 7))
    try:
        want = FM.frontier(box, lo)
        assert length >= 3000 and len(want[0]) == length and len(want[2]) == 1 and want[2]["count"][0] == length
        # the record order is far from the path order: the path's second plane starts at the far end of the records of the first
        got = t.avg_map().frontier(clusters=True)
        assert same3(got, want)
        assert np.all(got[1] == 0)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 4. boxes
def test_boxes(random_window):
    t, lo, hi, boxes = random_window
    box = boxes[0]
    whole = FM.frontier(box, lo)
    one = tuple(int(whole[0][n][len(whole[0]) // 2]) for n in "xyz")
    cases = {"whole window": (tuple(lo), tuple(hi)), "one voxel": (one, one),
             "unaligned cut": ((lo[0] + 2, lo[1] + 3, lo[2] + 1), (hi[0] - 4, hi[1] - 1, hi[2] - 2)),
             "one column": ((lo[0], hi[1], lo[2]), (lo[0], hi[1], hi[2])), "one plane": ((lo[0], lo[1], lo[2] + 9), (hi[0], hi[1], lo[2] + 9))}
    for name, (a, b) in cases.items():
        sub = box[tuple(slice(int(a[k] - lo[k]), int(b[k] - lo[k]) + 1) for k in range(3))]
        for flags in ((0, False), (TAU, True)):
            want = FM.frontier(sub, a, *flags)
            got = t.avg_map().frontier(lo=a, hi=b, min_value=flags[0], any_weight=flags[1], clusters=True)
            assert same3(got, want), (name, flags)
        if name == "one voxel":
            assert len(FM.records(sub, a)) == 0  # its neighbours are outside the box
        if name == "unaligned cut":
            inside = whole[0][np.all([(whole[0][n] >= a[k]) & (whole[0][n] <= b[k]) for k, n in enumerate("xyz")], axis=0)]
            assert len(FM.records(sub, a)) < len(inside)  # not the restriction of the window's result
    with pytest.raises(Exception):
        t.avg_map().frontier(lo=(int(lo[0]) - 1, 0, 0), hi=(int(lo[0]), 0, 0))  # outside the window


def test_a_box_face_cuts_a_cluster_in_two():
    box, cut_lo = u_box()
    t, lo, hi = make_window(box, pos=(0, 0, 0), offset=(4, 5, 6))
    try:
        whole = FM.frontier(box, lo)
        assert len(whole[2]) == 1
        a, b = (int(lo[0]), cut_lo, int(lo[2])), tuple(int(v) for v in hi)
        sub = box[:, cut_lo - int(lo[1]):, :]
        want = FM.frontier(sub, a)
        assert len(want[2]) == 2 and want[2]["count"].sum() < whole[2]["count"][0]
        assert same3(t.avg_map().frontier(clusters=True), whole)
        assert same3(t.avg_map().frontier(lo=a, hi=b, clusters=True), want)  # the box's table, not the window's
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 5. results and buffers
def test_zero_records_small_large_small_and_identical_calls(random_window):
    t, lo, hi, boxes = random_window
    L, n = t._L, C.c_size_t(5)
    empty, _, _ = make_window(np.zeros((5, 6, 7), dtype=np.uint32))
    try:
        assert raw_call(empty, 0, None, None, 0, CLUSTERS) == (0, 0, 0)
        for f in (L.ws_map_frontier_records_dev, L.ws_map_frontier_labels_dev, L.ws_map_frontier_clusters_dev):
            n.value = 5
            assert f(empty.handle, C.byref(n)) is None and n.value == 0
        rec, lab, tab = empty.avg_map().frontier(clusters=True)
        assert rec.shape == (0,) and rec.dtype == FM.RECORD and lab.shape == (0,) and tab.shape == (0,) and tab.dtype == FM.CLUSTER
        rc, _, got_n, got_k = download(empty)
        assert (rc, got_n, got_k) == (0, 0, 0)
    finally:
        empty.close()
    fresh, flo, fhi = make_window(boxes[0], **ROTATED)  # a map whose buffers have never grown
    try:
        small_box = ((flo[0], flo[1], flo[2]), (flo[0] + 3, flo[1] + 3, flo[2] + 3))
        small = FM.frontier(boxes[0][:4, :4, :4], small_box[0])
        large = FM.frontier(boxes[0], flo)
        assert 0 < len(small[0]) < len(large[0])
        avg = fresh.avg_map()
        assert same3(avg.frontier(*small_box, clusters=True), small)
        assert same3(avg.frontier(clusters=True), large)
        assert same3(avg.frontier(*small_box, clusters=True), small)  # the old result is gone
        rc, got, got_n, got_k = download(fresh)
        assert rc == 0 and (got_n, got_k) == (len(small[0]), len(small[2])) and same3(got, small)
        first, second = avg.frontier(clusters=True), avg.frontier(clusters=True)
        assert same3(first, second) and same3(first, large)
    finally:
        fresh.close()


def test_other_queries_leave_the_result_and_download_prefixes(random_window):
    t, lo, hi, boxes = random_window
    want = FM.frontier(boxes[0], lo, 1)
    avg = t.avg_map()
    assert same3(avg.frontier(min_value=1, clusters=True), want)
    avg.surface(marker=True), avg.mesh(), avg.distance(max_dist_vox=3), avg.sample(np.zeros((4, 3), np.int32))
    rc, got, n, k = download(t)
    assert rc == 0 and (n, k) == (len(want[0]), len(want[2])) and same3(got, want)
    # prefixes: fewer records and rows than there are, and more
    rc, got, n, k = download(t, cap_records=10, cap_clusters=2)
    assert rc == 0 and (n, k) == (len(want[0]), len(want[2])) and same3(got, tuple(w[:c] for w, c in zip(want, (10, 10, 2))))
    rc, got, n, k = download(t, cap_records=len(want[0]) + 9, cap_clusters=len(want[2]) + 9)
    assert rc == 0 and same3(tuple(g[:len(w)] for g, w in zip(got, want)), want)
    assert not got[0][len(want[0]):].view(np.uint8).any() and not got[2][len(want[2]):].view(np.uint8).any()  # nothing beyond the totals
    # device tensors alias the same bytes
    drec, dlab, dtab = avg.frontier(min_value=1, clusters=True, device=True)
    assert drec.is_cuda and tuple(drec.shape) == (len(want[0]), 4) and tuple(dtab.shape) == (len(want[2]), 16)
    assert np.array_equal(drec.cpu().numpy().view(np.uint8).reshape(-1), want[0].view(np.uint8))
    assert np.array_equal(dlab.cpu().numpy().view(np.uint8).reshape(-1), want[1].view(np.uint8))
    assert np.array_equal(dtab.cpu().numpy().view(np.uint8).reshape(-1), want[2].view(np.uint8))
    # a call without clusters: its labels and rows cannot be asked for
    assert same(avg.frontier(min_value=1), want[0])
    rc, _, n, k = download(t)
    assert rc == WS_ERR_INVALID and (n, k) == (len(want[0]), 0)
    rc, got, n, k = download(t, labels=False, table=False)
    assert rc == 0 and same(got[0], want[0])
    n = C.c_size_t(5)
    assert t._L.ws_map_frontier_labels_dev(t.handle, C.byref(n)) is None and n.value == 0
    assert t._L.ws_map_frontier_clusters_dev(t.handle, C.byref(n)) is None and n.value == 0
    assert t._L.ws_map_frontier_records_dev(t.handle, C.byref(n)) is not None and n.value == len(want[0])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_previous_result(random_window):
    t, lo, hi, boxes = random_window
    want = FM.frontier(boxes[0], lo)
    assert same3(t.avg_map().frontier(clusters=True), want)
    a, b = tuple(int(v) for v in lo), tuple(int(v) for v in hi)
    refused = {
        "unknown flag bits": ((0, a, b, 0, 4), WS_ERR_INVALID), "bad which": ((2, a, b, 0, 0), WS_ERR_INVALID), "negative which": ((-1, a, b, 0, 0), WS_ERR_INVALID),
        "only lo": ((0, a, None, 0, 0), WS_ERR_INVALID), "only hi": ((0, None, b, 0, 0), WS_ERR_INVALID),
        "hi < lo": ((0, b, a, 0, 0), WS_ERR_INVALID), "outside the window": ((0, (a[0] - 1, a[1], a[2]), b, 0, 0), WS_ERR_INVALID),
        "min_value < 0": ((0, a, b, -1, 0), WS_ERR_RANGE), "min_value > 32767": ((0, a, b, 32768, CLUSTERS), WS_ERR_RANGE),
    }
    for name, (args, code) in refused.items():
        rc, n, k = raw_call(t, *args)
        assert rc == code and (n, k) == (77, 77), (name, rc, n, k)
        rc, got, n, k = download(t)
        assert rc == 0 and same3(got, want), name
    assert raw_call(t, 0, a, b, 32767, ANY | CLUSTERS)[0] == 0
    assert t._L.ws_map_frontier(None, 0, None, None, 0, 0, None, None) == WS_ERR_INVALID
    assert t._L.ws_map_frontier_download(t.handle, None, None, None, 0, 0, None, None) == WS_ERR_INVALID
    assert raw_call(t, 0, None, None, 0, 0)[0] == 0 and t._L.ws_map_frontier(t.handle, 0, None, None, 0, 0, None, None) == 0  # the counts may be NULL


def test_timing_reports_four_stages(random_window):
    t, lo, hi, boxes = random_window
    avg = t.avg_map()
    avg.frontier_timing(1)
    avg.frontier(clusters=True)
    ms = avg.frontier_timing(0)
    assert len(ms) == 4 and all(v > 0 for v in ms), ms
    avg.frontier(clusters=True)
    assert avg.frontier_timing() == (0.0, 0.0, 0.0, 0.0)
