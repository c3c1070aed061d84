"""ws_store_frontier — the frontier of the global map in device memory (the rules are stated in include/warpsense_hip.h) against the
numpy model of frontier_model.py, applied to a dense array assembled from host copies of the chunks (store_scenes.assemble) in which
every voxel of an absent chunk is UNKNOWN.  Every comparison is on the raw bytes of records, labels and cluster table."""
import ctypes as C

import numpy as np
import pytest

import frontier_model as FM
import store_scenes as SM
from query_model import same, window

pytestmark = pytest.mark.gpu
TAU, RES, MW, CS, CW = 1000, 50, 640, 64, 64 ** 3
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
CLUSTERS = 2
FREE, WALL = FM.pack(TAU, 1), FM.pack(-TAU // 2, 3)


def same3(got, want):
    return len(got) == len(want) == 3 and all(same(g, w) for g, w in zip(got, want))


def model(chunks, lo, hi, min_value=0, any_weight=False):
    present = SM.assemble({k: np.ones(CW, dtype=np.uint32) for k in chunks}, lo, hi) != 0
    return FM.frontier(SM.assemble(chunks, lo, hi), lo, min_value, any_weight, present)


# ------------------------------------------------------------------------------------------------ the seam store
def seam_chunks():
    """seven chunks around the origin, (0, 0, -1) absent; everything unknown but: a free block around the common corner, which
    crosses a chunk face on every axis and stands against the absent chunk; three small blobs, one across a face of every axis; a
    walled free plate in the outer face x = -64 of the bounding box; and some entries of negative weight"""
    w = np.zeros((2 * CS,) * 3, dtype=np.uint32)  # index = world + 64
    w[58:70, 58:70, 58:70] = FREE
    w[63:65, 94:96, 94:96] = FREE   # across x = -1 | 0
    w[20:22, 63:65, 100:102] = FREE  # across y = -1 | 0
    w[100:102, 20:22, 63:65] = FREE  # across z = -1 | 0, in the chunks (0, -1, -1) and (0, -1, 0)
    w[0:2, 73:86, 73:86] = WALL
    w[0, 74:85, 74:85] = FREE
    w[30:33, 30:33, 30:33] = FM.pack(TAU, -1)  # free under ANY_WEIGHT only
    chunks = SM.split(w)
    del chunks[SM.ABSENT]
    return chunks


BOUNDS = ((-CS,) * 3, (CS - 1,) * 3)
GROWN = ((-CS - 1,) * 3, (CS,) * 3)


@pytest.fixture(scope="module")
def seam():
    chunks = seam_chunks()
    store = SM.make_store(chunks)  # segments of two chunks
    yield store, chunks
    store.close()


def test_clusters_cross_chunk_faces_and_the_absent_chunk_is_frontier(seam):
    store, chunks = seam
    want = model(chunks, *BOUNDS)
    rec, labels, table = want
    assert len(rec) >= 200 and len(table) == 4 and int(np.bitwise_or.reduce(rec["mask"])) == 0b111111 and table["count"].max() >= 50
    big = rec[labels == labels[np.argmax((rec["x"] == -6) & (rec["y"] == -6) & (rec["z"] == -6))]]
    for n in "xyz":  # the block's cluster has members on both sides of the face between key -1 and key 0 of every axis
        assert big[n].min() < 0 <= big[n].max()
    # a free face against the absent chunk (x >= 0, y >= 0, z < 0): the block's voxels at z = 0 above it see UNKNOWN at -z
    face = rec[(rec["x"] == 2) & (rec["y"] == 2) & (rec["z"] == 0)]
    assert len(face) == 1 and face["mask"][0] == 0b010000
    assert not np.any((rec["x"] >= 0) & (rec["y"] >= 0) & (rec["z"] < 0))  # a voxel of an absent chunk is never free
    for any_weight in (False, True):
        for min_value in (0, TAU, TAU + 1):
            want = model(chunks, *BOUNDS, min_value, any_weight)
            assert same3(store.frontier(min_value=min_value, any_weight=any_weight, clusters=True), want), (min_value, any_weight)
            assert same3(store.frontier(*BOUNDS, min_value=min_value, any_weight=any_weight, clusters=True), want)
            assert same(store.frontier(min_value=min_value, any_weight=any_weight), want[0])
    assert len(model(chunks, *BOUNDS, 0, True)[2]) == 5 and len(model(chunks, *BOUNDS, TAU + 1)[0]) == 0


def test_default_box_against_the_box_grown_by_one(seam):
    store, chunks = seam
    inner, outer = model(chunks, *BOUNDS), model(chunks, *GROWN)
    plate = lambda r: r[(r["x"] == -CS)]
    assert len(plate(inner[0])) == 0 and len(plate(outer[0])) == 121 and np.all(plate(outer[0])["mask"] == 0b000001)
    assert len(outer[2]) == len(inner[2]) + 1
    assert same3(store.frontier(clusters=True), inner)
    assert same3(store.frontier(*GROWN, clusters=True), outer)
    cut = ((-40, -29, -50), (37, 45, 20))  # cuts all seven chunks (and the absent one) with unaligned faces
    assert same3(store.frontier(*cut, clusters=True), model(chunks, *cut))
    assert same3(store.frontier((1, 1, -60), (60, 60, -2), clusters=True), model(chunks, (1, 1, -60), (60, 60, -2)))  # in the absent chunk
    far = ((-2 ** 31,) * 3, (2 ** 31 - 1,) * 3)  # any box in int32: every face of the mapped volume is inside it
    assert same3(store.frontier(*far, clusters=True), outer)


def test_same_bytes_as_the_window(seam):
    import warpsense_amd as W
    store, chunks = seam
    lm = W.LocalMap(127, 127, 127, TAU, 0)
    t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
    try:
        lo, hi = window(lm.size, lm.pos)
        assert tuple(lo) == (-63,) * 3 and tuple(hi) == (63,) * 3 and (store.default_raw >> 16) == 0  # fill_entry has weight 0
        store.load_box(t, lo, hi)
        for a, b in [(tuple(lo), tuple(hi)), ((-40, -29, -50), (37, 45, 20)), ((-63, -5, -7), (63, 4, 9))]:
            for any_weight in (False, True):
                got_window = t.avg_map().frontier(lo=a, hi=b, any_weight=any_weight, clusters=True)
                got_store = store.frontier(lo=a, hi=b, any_weight=any_weight, clusters=True)
                assert len(got_store[0]) > 100 and same3(got_store, got_window) and same3(got_store, model(chunks, a, b, 0, any_weight)), (a, b, any_weight)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ far-apart chunks
FAR_KEYS = [(-20000, 15000, -16000), (0, 0, 0), (20000, -15000, 16000)]


def test_three_chunks_a_million_voxels_apart():
    chunks = {}
    for i, key in enumerate(FAR_KEYS):
        c = np.zeros((CS,) * 3, dtype=np.uint32)
        c[20 + i:30, 25:31, 28:36 + i] = FREE
        c[0:3, 40:45, 63] = FREE  # in two faces of the chunk: x = 0 is a face of the bounding box for the first chunk only
        chunks[key] = c.reshape(-1)
    lo, hi = SM.bounding_box(chunks)
    assert int((hi - lo).min()) > 1_000_000
    parts, n, k = [], 0, 0
    for key in sorted(chunks):  # ascending cx: the chunks follow each other in the records; their neighbours are absent chunks
        base = np.asarray(key, dtype=np.int64) * CS
        a, b = np.maximum(base - 1, lo), np.minimum(base + CS, hi)
        rec, labels, table = model({key: chunks[key]}, a, b)
        table["first"] += n
        parts.append((rec, labels + np.uint32(k), table))
        n, k = n + len(rec), k + len(table)
    want = tuple(np.concatenate([p[j] for p in parts]) for j in range(3))
    assert len(want[0]) > 600 and len(want[2]) == 6
    store = SM.make_store(chunks, segment_chunks=0)
    try:
        # What the header's cost rule allows on a first call: 32 KB of masks and totals and 56 bytes of tables per listed chunk, 24 bytes
        # per record (record, parent, label) and 64 per cluster with an eighth of slack -- under 200 KB for three chunks and a thousand
        # records -- in twelve device allocations (mask, two totals, the count, records, tables, parents, labels, two head totals, the
        # head count, clusters), each of which the allocator may round up to 2 MB.  A pass over the box would need 10^15 bytes.
        import torch
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        got = store.frontier(clusters=True)
        taken = free_before - torch.cuda.mem_get_info()[0]
        print("device memory taken by the first call:", taken)
        assert taken <= (12 * 2 + 1) << 20, taken
        assert same3(got, want)
        assert int(np.diff(got[0]["x"].astype(np.int64)).max()) > 1_000_000
        assert same3(store.frontier(lo=lo, hi=hi, clusters=True), want)
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ empty store, refusals, buffers
def raw_call(store, lo, hi, min_value, flags):
    n, k = C.c_size_t(77), C.c_size_t(77)
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    return store._L.ws_store_frontier(store.handle, p(a), p(b), min_value, flags, C.byref(n), C.byref(k)), n.value, k.value


def test_a_store_with_zero_chunks():
    import warpsense_amd as W
    empty = W.DeviceGlobalMap(TAU, 0)
    try:
        assert raw_call(empty, None, None, 0, CLUSTERS) == (0, 0, 0) and raw_call(empty, (-5, -5, -5), (5, 5, 5), 0, 0) == (0, 0, 0)
        n = C.c_size_t(9)
        for f in (empty._L.ws_store_frontier_records_dev, empty._L.ws_store_frontier_labels_dev, empty._L.ws_store_frontier_clusters_dev):
            n.value = 9
            assert f(empty.handle, C.byref(n)) is None and n.value == 0
        rec, labels, table = empty.frontier(clusters=True)
        assert rec.shape == (0,) and rec.dtype == FM.RECORD and labels.shape == (0,) and table.shape == (0,) and table.dtype == FM.CLUSTER
    finally:
        empty.close()


def test_refusals_leave_the_previous_result_and_timing(seam):
    store, chunks = seam
    want = model(chunks, *BOUNDS)
    assert same3(store.frontier(clusters=True), want)
    a, b = BOUNDS
    for name, (args, code) in {"unknown flag bits": ((a, b, 0, 8), WS_ERR_INVALID), "only lo": ((a, None, 0, 0), WS_ERR_INVALID),
                               "only hi": ((None, b, 0, 0), WS_ERR_INVALID), "hi < lo": ((b, a, 0, 0), WS_ERR_INVALID),
                               "min_value < 0": ((a, b, -1, 0), WS_ERR_RANGE), "min_value > 32767": ((a, b, 32768, 0), WS_ERR_RANGE)}.items():
        assert raw_call(store, *args) == (code, 77, 77), name
        n, k = C.c_size_t(0), C.c_size_t(0)
        rec, lab, tab = np.zeros(len(want[0]), FM.RECORD), np.zeros(len(want[0]), np.uint32), np.zeros(len(want[2]), FM.CLUSTER)
        p = lambda v: v.ctypes.data_as(C.c_void_p)
        assert store._L.ws_store_frontier_download(store.handle, p(rec), p(lab), p(tab), len(rec), len(tab), C.byref(n), C.byref(k)) == 0
        assert (n.value, k.value) == (len(rec), len(tab)) and same3((rec, lab, tab), want), name
    store.surface(TAU, RES), store.mesh(RES), store.distance(lo=(-8, -8, -8), hi=(8, 8, 8), max_dist_vox=3)  # other queries in between
    drec, dlab, dtab = (v.cpu().numpy() for v in store.frontier(clusters=True, device=True))
    assert same(np.ascontiguousarray(drec).view(FM.RECORD).reshape(-1), want[0]) and same(dlab.view(np.uint32), want[1])
    assert same(np.ascontiguousarray(dtab).view(FM.CLUSTER).reshape(-1), want[2])
    assert same(store.frontier(), want[0])
    assert store._L.ws_store_frontier_download(store.handle, None, p(lab), None, 4, 0, C.byref(n), C.byref(k)) == WS_ERR_INVALID
    store.frontier_timing(1)
    store.frontier(clusters=True)
    ms = store.frontier_timing(0)
    assert len(ms) == 4 and all(v > 0 for v in ms), ms
