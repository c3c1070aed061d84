"""The resolution and position domain of the queries, as include/warpsense_hip.h states it: resolutions 2 .. 1024 mm for a map (from
1 mm for the store), a ray origin with |o| + max_range + 2 res <= INT32_MAX, a mesh box with (|c| + 1) res <= INT32_MAX, windows and
chunks anywhere in int32 voxel space.  The four map queries (surface, mesh, ray cast, distance) and the two store queries
(ws_store_mesh, ws_store_raycast) against the numpy models of their own test files, on raw bytes, at the resolutions where the step
and half rules, the fractions and the 2^30 weights change (2, 3, 51, 1024; 1 for the store) and at positions near +-2 * 10^9 mm and
10^9 voxels; and every far result against the near result of the same entries moved by whole voxels, which a mistake shared by
model and kernel would not survive.  tests/test_query_domain_host.py holds the models to hand-worked cases, the sphere and the
translation property without a GPU, and checks that every fixture here clears its thresholds in the model alone.

The inputs (rows, maps, ray sets, chunk sets) live here, so that the host checks and these tests use the same ones."""
import ctypes as C

import numpy as np
import pytest

import distance_model as D
import mesh_model as M
from query_domain_scenes import CS, FAR_ROWS, I32, MW, NEAR, N_RANDOM, OFF, ROWS, SIZE, SPECIAL, STORE_CASES, TAU, counts, edge_case, entries, inner_box, moved, moved_surface, moved_vert, rays, store_base, store_boxes, store_chunks, store_id, store_keys, store_model, store_rays, wrap_targets
import query_model as QM
import raycast_model as R
import store_raycast_scenes as SR
import store_scenes as SM
import surface_model as G

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5


def row_id(row):
    return f"res{row[0]}-x{row[1][0]}"


def mesh_edge_case(res, sign):
    """a window whose last voxel on x lies one voxel beyond the largest the mesh's range rule admits: (pos, lo, hi of the largest box)"""
    c_max = I32 // res - 1
    assert (c_max + 1) * res <= I32 < (c_max + 2) * res
    pos = (sign * (c_max + 1 - SIZE[0] // 2), 4, -3)
    lo, hi = QM.window(SIZE, pos)
    assert max(abs(int(lo[0])), abs(int(hi[0]))) == c_max + 1
    a, b = lo.copy(), hi.copy()
    if sign > 0:
        b[0] -= 1
    else:
        a[0] += 1
    return pos, a, b


# ------------------------------------------------------------------------------------------------ helpers on the device
def upload(res, pos):
    return R.upload(SIZE, pos, OFF, entries(), res=res)


def raw_map_cast(t, o, d, rng, flags=0):
    o, d = np.ascontiguousarray(o, dtype=np.int32), np.ascontiguousarray(d, dtype=np.int32)
    return t._L.ws_map_raycast(t.handle, 0, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), len(d), rng, flags, None)


def last_map_records(t, n):
    rec, got = np.zeros(n, dtype=R.RAY), C.c_size_t(0)
    assert t._L.ws_map_raycast_download(t.handle, rec.ctypes.data_as(C.c_void_p), None, n, C.byref(got)) == 0 and got.value == n
    return rec


def mesh_totals(t):
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    assert t._L.ws_map_mesh_download(t.handle, None, None, 0, 0, C.byref(gv), C.byref(gf)) == 0
    return gv.value, gf.value


# ------------------------------------------------------------------------------------------------ 1. the window queries, row by row
def test_a_map_needs_two_millimetres():
    import warpsense_amd as W
    view = W.DeviceMap(SIZE, OFF, entries()[0], NEAR)
    with pytest.raises(W.WsError):
        W.TSDFCuda(view, TAU, MW, 1)
    W.TSDFCuda(view, TAU, MW, 2).close()


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_raycast_matches_the_model(row):
    import torch
    res, pos = row
    t, views = upload(res, pos)
    o, d, rng = rays(res, pos)
    avg = t.avg_map()
    for any_weight in (False, True):
        want = R.model_of(views[0], res, o, d, rng, any_weight)
        n_hit, n_grad = counts(want)
        print(row_id(row), any_weight, "hits", n_hit, "gradients", n_grad)
        assert n_hit > 500 and n_grad > 300
        assert R.same(avg.raycast(o, d.astype(np.int32), rng, any_weight=any_weight, gradient=True), want), any_weight
        assert avg.last_hits == n_hit
    # as targets, from the host and from the device (the random directions: origin + direction fits int32 at every row)
    dr = d[:N_RANDOM]
    want = R.model_of(views[0], res, o, o + dr, rng, False, True)
    assert R.same(want, R.model_of(views[0], res, o, dr, rng)) and counts(want)[0] > 500
    tgt = (o + dr).astype(np.int32)
    assert R.same(avg.raycast(o, tgt, rng, gradient=True, targets=True), want)
    assert R.same(avg.raycast(o, torch.from_numpy(tgt).cuda(), rng, gradient=True, targets=True), want)
    assert R.same(avg.raycast(o, torch.from_numpy(dr.astype(np.int32)).cuda(), rng, gradient=True), want)
    t.close()


@pytest.mark.parametrize("sign", (1, -1))
@pytest.mark.parametrize("res", sorted({r for r, _ in FAR_ROWS}))
def test_raycast_at_the_edge_of_the_origin_range(res, sign):
    pos, o, rng = edge_case(res, sign)
    assert abs(int(o[0])) + rng + 2 * res == I32
    t, views = upload(res, pos)
    avg = t.avg_map()
    d = np.concatenate([np.random.default_rng(res).integers(-32768, 32769, (N_RANDOM, 3)), SPECIAL])
    for any_weight in (False, True):
        want = R.model_of(views[0], res, o, d, rng, any_weight)
        n_hit, n_grad = counts(want)
        print(res, sign, any_weight, "hits", n_hit, "gradients", n_grad)
        assert n_hit > 500 and n_grad > 300
        assert R.same(avg.raycast(o, d.astype(np.int32), rng, any_weight=any_weight, gradient=True), want), any_weight
        assert avg.last_hits == n_hit
    # one unit beyond the edge: refused, nothing launched, the last result stays readable
    beyond = o.copy()
    beyond[0] += sign
    assert raw_map_cast(t, beyond, d, rng) == WS_ERR_RANGE and raw_map_cast(t, o, d, rng + 1) == WS_ERR_RANGE
    assert QM.same(last_map_records(t, len(d)), want[0])
    if sign < 0:
        # targets whose difference from the origin needs more than 32 bits
        tgt = wrap_targets(o, rng, res)
        want = R.model_of(views[0], res, o, tgt, rng, True, True)
        hit = want[0]["range_mm"] >= 0
        print(res, "wrapping targets: hits per group", [int(hit[k:k + 64].sum()) for k in (0, 64, 128)])
        assert hit[:64].sum() > 16 and not hit[64:].any()
        short = R.model_of(views[0], res, o, tgt - 2 ** 32 * (np.arange(192) >= 128)[:, None] * np.array([1, 0, 0]), rng, True, True)
        assert (short[0]["range_mm"][128:] >= 0).sum() > 16  # what a 32-bit subtraction would make of the third group: hits
        assert R.same(avg.raycast(o, tgt.astype(np.int32), rng, any_weight=True, gradient=True, targets=True), want)
    t.close()


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_mesh_matches_the_model(row):
    res, pos = row
    t, views = upload(res, pos)
    for name, (a, b) in (("window", (None, None)), ("inner", inner_box(pos))):
        for any_weight in (False, True):
            want = M.model(views[0], res, a, b, any_weight)
            print(row_id(row), name, any_weight, "vertices", len(want[0]), "faces", len(want[1]))
            assert len(want[0]) > 100 and len(want[1]) > 100
            assert M.same(t.avg_map().mesh(lo=a, hi=b, any_weight=any_weight), want), (name, any_weight)
    t.close()


@pytest.mark.parametrize("res,sign", [(1024, 1), (1024, -1), (2, 1), (2, -1)])
def test_mesh_of_the_largest_box_the_range_rule_admits(res, sign):
    pos, a, b = mesh_edge_case(res, sign)
    t, views = upload(res, pos)
    avg = t.avg_map()
    for any_weight in (False, True):
        want = M.model(views[0], res, a, b, any_weight)
        print(res, sign, any_weight, "vertices", len(want[0]), "faces", len(want[1]), "largest |x_mm|", int(np.abs(want[0]["x_mm"].astype(np.int64)).max()))
        assert len(want[0]) > 100 and len(want[1]) > 100
        assert M.same(avg.mesh(lo=a, hi=b, any_weight=any_weight), want), any_weight
    assert np.abs(want[0]["x_mm"].astype(np.int64)).max() > I32 - 3 * res  # vertices within three voxels of the end of int32
    # one voxel further, and the whole window: refused, nothing launched, the last result stays
    before = mesh_totals(t)
    lo, hi = QM.window(SIZE, pos)
    nv, nf = C.c_size_t(7), C.c_size_t(7)
    p = lambda v: np.ascontiguousarray(v, dtype=np.int32).ctypes.data_as(C.c_void_p)
    assert t._L.ws_map_mesh(t.handle, 0, p(lo), p(hi), 0, C.byref(nv), C.byref(nf)) == WS_ERR_RANGE
    assert t._L.ws_map_mesh(t.handle, 0, None, None, 0, C.byref(nv), C.byref(nf)) == WS_ERR_RANGE
    assert mesh_totals(t) == before == (len(want[0]), len(want[1]))
    t.close()


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_surface_matches_the_model(row):
    res, pos = row
    t, views = upload(res, pos)
    for name, (a, b) in (("window", (None, None)), ("inner", inner_box(pos))):
        want_rec, want_mk = G.model(views[0], TAU, res, a, b)
        rec, mk = t.avg_map().surface(lo=a, hi=b, marker=True)
        print(row_id(row), name, "records", len(want_rec))
        assert len(want_rec) > 100 and QM.same(rec, want_rec) and QM.same(mk, want_mk), name
    if pos[0] >= 2 ** 24:
        x = want_rec["x"].astype(np.int64)
        assert np.any(np.float32(x).astype(np.int64) != x)  # the marker's (float)x rounds
    t.close()


@pytest.mark.parametrize("row", FAR_ROWS, ids=row_id)
def test_distance_matches_the_model(row):
    res, pos = row
    t, views = upload(res, pos)
    for name, (a, b) in (("window", (None, None)), ("inner", inner_box(pos))):
        for kw in ({}, dict(unknown_occupied=True), dict(columns=True)):
            want, n_sites = D.model(views[1], 5, a, b, **kw)
            d2 = want & np.uint32(0xFFFFFF)
            print(row_id(row), name, kw, "sites", n_sites, "between", int(np.count_nonzero((d2 > 0) & (d2 < 25))))
            assert n_sites >= 3 and np.count_nonzero((d2 > 0) & (d2 < 25)) > 20
            assert D.same(t.new_map().distance(lo=a, hi=b, max_dist_vox=5, **kw), want) and t.new_map().last_sites == n_sites, (name, kw)
    t.close()


@pytest.mark.parametrize("row", FAR_ROWS, ids=row_id)
def test_the_far_window_gives_the_near_result_moved(row):
    """the same entries at NEAR and at the row's position, the origin and the targets moved by whole voxels: ranges, gradients, faces,
    weights, distance records and raw entries identical, points moved by s res, surface voxels by s"""
    res, pos = row
    s = np.asarray(pos, dtype=np.int64) - NEAR
    near, _ = upload(res, NEAR)
    far, _ = upload(res, pos)
    (o0, d, rng), (o1, _, _) = rays(res, NEAR), rays(res, pos)
    assert np.array_equal(o1 - o0, s * res)
    for any_weight in (False, True):
        a = near.avg_map().raycast(o0, d.astype(np.int32), rng, any_weight=any_weight, gradient=True)
        b = far.avg_map().raycast(o1, d.astype(np.int32), rng, any_weight=any_weight, gradient=True)
        assert counts(a)[0] > 500 and R.same(b, (moved(a[0], s * res), a[1])), any_weight
        va, fa = near.avg_map().mesh(any_weight=any_weight)
        vb, fb = far.avg_map().mesh(any_weight=any_weight)
        assert len(fa) > 100 and M.same((vb, fb), (moved_vert(va, s * res), fa)), any_weight
    dr = d[:N_RANDOM]
    a = near.avg_map().raycast(o0, (o0 + dr).astype(np.int32), rng, gradient=True, targets=True)
    b = far.avg_map().raycast(o1, (o1 + dr).astype(np.int32), rng, gradient=True, targets=True)
    assert R.same(b, (moved(a[0], s * res), a[1]))
    ra, rb = near.avg_map().surface(), far.avg_map().surface()
    assert len(ra) > 100 and QM.same(rb, moved_surface(ra, s))
    for kw in ({}, dict(unknown_occupied=True), dict(columns=True)):
        assert D.same(far.new_map().distance(max_dist_vox=5, **kw), near.new_map().distance(max_dist_vox=5, **kw)), kw
    near.close()
    far.close()


# ------------------------------------------------------------------------------------------------ 2. the store queries
def test_the_store_admits_one_millimetre_and_refuses_zero():
    store = SM.make_store(store_chunks(1, "near"))
    try:
        o, d, rng = store_rays(1, "near")["in"]
        d = np.ascontiguousarray(d[:64], dtype=np.int32)
        assert SR.raw_cast(store, o, d, len(d), rng, res=0)[0] == WS_ERR_INVALID and SM.raw_mesh(store, None, None, 0)[0] == WS_ERR_INVALID
        assert SR.raw_cast(store, o, d, len(d), rng, res=1)[0] == 0 and SM.raw_mesh(store, None, None, 1)[0] == 0
        assert SR.raw_cast(store, o, d, len(d), rng, res=1025)[0] == WS_ERR_RANGE
    finally:
        store.close()


@pytest.mark.parametrize("case", STORE_CASES, ids=store_id)
def test_store_raycast_matches_the_model(case):
    res, where = case
    store = SM.make_store(store_chunks(res, where))
    try:
        sets = store_rays(res, where)
        boxes = store_boxes(res, where)
        # (each model walks every sample: the random rays run on both boxes under both weight rules, the long rays across the absent
        # chunks under one rule per box)
        for box, name, any_weight in ((None, "in", False), (None, "in", True), (None, "gap", False), (boxes[1], "in", False), (boxes[1], "in", True),
                                      (boxes[1], "gap", True)):
            lo, hi = (None, None) if box is None else box
            o, d, rng = sets[name]
            want = store_model(res, where, name, box, any_weight)
            n_hit, n_grad = counts(want)
            print(store_id(case), "box" if box else "all", name, any_weight, "hits", n_hit, "gradients", n_grad, "of", len(d))
            if name == "in":
                assert n_hit > 500 and n_grad > 300
            elif box is None:
                assert n_hit > 50  # behind 13 absent chunks
            got = store.raycast(res, o, d.astype(np.int32), rng, lo=lo, hi=hi, any_weight=any_weight, gradient=True)
            assert R.same(got, want), (box is None, name, any_weight)
            assert store.last_hits == n_hit
        o, d, rng = sets["in"]
        tgt = np.clip(o + d[:N_RANDOM], -I32, I32)  # (the origin of a far block lies within 2^15 of the end of int32)
        want = R.model(SR.Chunks(store_chunks(res, where), base=store_base(res, where)), res, o, tgt, rng, False, True)
        assert counts(want)[0] > 500
        assert R.same(store.raycast(res, o, tgt.astype(np.int32), rng, gradient=True, targets=True), want)
    finally:
        store.close()


@pytest.mark.parametrize("case", STORE_CASES, ids=store_id)
def test_store_mesh_matches_the_model(case):
    res, where = case
    chunks = store_chunks(res, where)
    K, x_lone = store_keys(res, where)
    store = SM.make_store(chunks)
    try:
        block = {k: v for k, v in chunks.items() if k[0] != x_lone}
        lone = {k: v for k, v in chunks.items() if k[0] == x_lone}
        for any_weight in (False, True):
            # the bounding box: the block and the isolated chunk, their cells following each other in ascending x
            parts = [SM.model_store(c, res, any_weight=any_weight) for c in ((block, lone) if x_lone > K[0] else (lone, block))]
            want = (np.concatenate([parts[0][0], parts[1][0]]), np.concatenate([parts[0][1], parts[1][1] + np.uint32(len(parts[0][0]))]))
            print(store_id(case), any_weight, "vertices", len(want[0]), "faces", len(want[1]))
            assert len(want[0]) > 100 and len(want[1]) > 100
            assert M.same(store.mesh(res, any_weight=any_weight), want), any_weight
            a, b = store_boxes(res, where)[1]
            want = SM.model_store(block, res, a, b, any_weight)
            assert len(want[0]) > 100 and len(want[1]) > 100
            assert M.same(store.mesh(res, lo=a, hi=b, any_weight=any_weight), want), ("box", any_weight)
    finally:
        store.close()


@pytest.mark.parametrize("case", [c for c in STORE_CASES if c[0] >= 2], ids=store_id)
def test_store_and_window_return_the_same_bytes(case):
    """the block loaded into a window of that resolution at the same place (ws_store_load_box): the store's queries on the window's
    box and the window's queries give the same bytes"""
    import warpsense_amd as W
    res, where = case
    K = np.asarray(store_keys(res, where)[0], dtype=np.int64) * CS
    store = SM.make_store(store_chunks(res, where))
    try:
        lm = W.LocalMap(129, 129, 129, TAU, 0)
        view = lm.device_map()
        view.pos_[:] = K + CS
        t = W.TSDFCuda(view, TAU, MW, res)
        lo, hi = QM.window(view.size_, view.pos_)
        assert tuple(lo) == tuple(K) and tuple(hi) == tuple(K + 2 * CS) and (store.default_raw >> 16) == 0
        store.load_box(t, lo, hi)
        o, d, rng = store_rays(res, where)["in"]
        for any_weight in (False, True):
            got_window = t.avg_map().raycast(o, d.astype(np.int32), rng, any_weight=any_weight, gradient=True)
            got_store = store.raycast(res, o, d.astype(np.int32), rng, lo=lo, hi=hi, any_weight=any_weight, gradient=True)
            assert counts(got_store)[0] > 500 and R.same(got_store, got_window), any_weight
            for a, b in ((K, K + 2 * CS - 1), store_boxes(res, where)[1]):
                got_window, got_store = t.avg_map().mesh(lo=a, hi=b, any_weight=any_weight), store.mesh(res, lo=a, hi=b, any_weight=any_weight)
                assert len(got_store[0]) > 100 and len(got_store[1]) > 100 and M.same(got_store, got_window), (any_weight, tuple(a))
        t.close()
    finally:
        store.close()
