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

import test_gpu_distance as D
import test_gpu_mesh as M
import test_gpu_raycast as R
import test_gpu_store_mesh as SM
import test_gpu_store_raycast as SR
import test_gpu_surface as G
import test_store_raycast_host as H

pytestmark = pytest.mark.gpu
TAU, MW = G.TAU, 640
I32 = 2 ** 31 - 1
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
CS = 64

# ------------------------------------------------------------------------------------------------ the window grid
SIZE = (21, 17, 13)        # the smallest of G.SIZES
OFF = (5, 11, 9)           # the ring's seam lies inside the window on every axis
NEAR = (0, 0, 3)
ROWS = [(2, NEAR), (3, NEAR), (51, NEAR), (1024, NEAR),
        (50, (40_000_000, -20_000_000, 3)),        # voxel x beyond 2^24 (marker rounding), mm near 2 * 10^9
        (1024, (-2_000_000, 1_000_000, 3)),        # negative far, the largest resolution
        (2, (1_000_000_000, -500_000_000, 3))]     # the ring sum b - pos + offset + size at 10^9
FAR_ROWS = ROWS[4:]


def row_id(row):
    return f"res{row[0]}-x{row[1][0]}"


BIG = 2 ** 30 - 1
SPECIAL = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0], [BIG, BIG, -BIG], [-BIG, 3, BIG], [BIG, -BIG, 7], [2 ** 30, 1, 1],
                    [0, 0, 0], [-2 ** 31, 0, 0]], dtype=np.int64)  # the list of test_rotated_rings_after_the_shift_sequence
N_RANDOM = 2048


_ENTRIES = []


def entries():
    """storage-order entries of the two maps, drawn once: the mesh's draw (ray cast, mesh, surface) and the distance field's draw"""
    if not _ENTRIES:
        _ENTRIES.extend([M.draw_entries(SIZE, seed=5), D.draw_entries(SIZE, seed=5)])
    return _ENTRIES


def ring(pos, which=0):
    return R.Ring(entries()[which], SIZE, pos, OFF)


def rays(res, pos):
    """origin at the window's centre, 2048 random directions and the special ones; max_range"""
    lo, _ = G.window(SIZE, pos)
    o, d = R.random_rays(SIZE, seed=sum(SIZE), lo=lo, n=N_RANDOM, res=res)
    return o, np.concatenate([d, SPECIAL]), 60 * res


def counts(want):
    return H.hits_of(want[0]), int(np.count_nonzero(np.any(want[1] != 0, axis=1)))


def inner_box(pos):
    lo, hi = G.window(SIZE, pos)
    return lo + (1, 2, 1), hi - (2, 1, 1)


def edge_case(res, sign, axis=0):
    """an origin with |o| + max_range + 2 res == INT32_MAX exactly on `axis`, in the centre voxel of a window: (pos, origin, range)"""
    rng = 60 * res
    pos, o = [7, -5, 3], [7 * res + 1, -5 * res + 2, 3 * res + 3]
    o[axis] = sign * (I32 - rng - 2 * res)
    pos[axis] = o[axis] // res
    return tuple(pos), np.asarray(o, dtype=np.int64), rng


def wrap_targets(o, rng, res):
    """targets from an origin at the negative edge of x: 64 with d_x = 2^30 - 1 (live), 64 with 2^30 (dead), 64 whose true d_x of about
    2^32 wraps, in 32 bits, to a short ray towards -x (dead; live and mostly hitting if the subtraction were 32-bit)"""
    g = np.random.default_rng(3)
    m = rng + 2 * res
    out = []
    for dx, spread in ((2 ** 30 - 1, 2 ** 29), (2 ** 30, 2 ** 29), (2 ** 32 - (m + 1000), m + 1000)):
        d = np.concatenate([np.full((64, 1), dx, dtype=np.int64), g.integers(-spread, spread + 1, (64, 2))], axis=1)
        out.append(o + d)
    tgt = np.concatenate(out)
    assert np.all(np.abs(tgt) <= I32)
    return tgt


def mesh_edge_case(res, sign):
    """a window whose last voxel on x lies one voxel beyond the largest the mesh's range rule admits: (pos, lo, hi of the largest box)"""
    c_max = I32 // res - 1
    assert (c_max + 1) * res <= I32 < (c_max + 2) * res
    pos = (sign * (c_max + 1 - SIZE[0] // 2), 4, -3)
    lo, hi = G.window(SIZE, pos)
    assert max(abs(int(lo[0])), abs(int(hi[0]))) == c_max + 1
    a, b = lo.copy(), hi.copy()
    if sign > 0:
        b[0] -= 1
    else:
        a[0] += 1
    return pos, a, b


# ------------------------------------------------------------------------------------------------ the store grid
STORE_RES = (1, 3, 51, 1024)  # ws_store_raycast and ws_store_mesh admit map_resolution >= 1: half = 0, step = 1
GAP = 13                      # absent chunks between the block and the isolated chunk, along x


def store_keys(res, where):
    """(key origin K of the 2 x 2 x 2 block K .. K + 1, x key of the isolated chunk).  "near": the block straddles the world origin.
    "+" / "-": the isolated chunk is the outermost chunk whose every voxel the mesh's range rule admits, within one chunk of
    +-INT32_MAX mm; the block lies 13 absent chunks nearer to the origin"""
    if where == "near":
        return (-1, -1, -1), 1 + GAP
    k_out = (I32 // res - 1 - (CS - 1)) // CS  # 64 k + 63 <= INT32_MAX / res - 1
    assert (CS * k_out + CS) * res <= I32 < (CS * (k_out + 2)) * res
    if where == "+":
        return (k_out - GAP - 2, 3, -2), k_out
    k_neg = (I32 // res - 1) // CS  # the chunk -k holds the voxels -64 k .. -64 k + 63: (64 k + 1) res <= INT32_MAX
    return (-k_neg + GAP + 1, 3, -2), -k_neg


_STORE = {}


def store_chunks(res, where):
    """seven chunks of the block (the one at K + (1, 1, 0) absent) and the isolated chunk, drawn entries"""
    if "world" not in _STORE:
        _STORE["world"] = M.draw_entries((2 * CS,) * 3, seed=128).reshape((2 * CS,) * 3)
        _STORE["lone"] = M.draw_entries((CS,) * 3, seed=77)
    K, x_lone = store_keys(res, where)
    w = _STORE["world"]
    out = {}
    for c in SM.SEAM_KEYS:
        if c == SM.ABSENT:
            continue
        out[tuple(K[k] + c[k] + 1 for k in range(3))] = np.ascontiguousarray(w[tuple(slice(CS * (v + 1), CS * (v + 2)) for v in c)]).reshape(-1)
    out[(x_lone, K[1], K[2])] = _STORE["lone"]
    return out


def store_base(res, where):
    return store_keys(res, where)[0]


def store_boxes(res, where):
    """None (the default box) and a sub-box that cuts through the chunks of the block"""
    K = np.asarray(store_keys(res, where)[0], dtype=np.int64) * CS
    return [None, (K + (24, 35, 14), K + (101, 109, 84))]


def store_rays(res, where):
    """(origin, dirs, range) of the ray sets: "in" -- from the block's common corner, 2048 random directions and the special ones,
    60 res; "gap" -- from the absent stretch two chunks off the block towards the isolated chunk, across the absent chunks between,
    with the largest range the origin admits on the far side"""
    K, x_lone = store_keys(res, where)
    Kv = np.asarray(K, dtype=np.int64) * CS
    g = np.random.default_rng(19)
    o_in = (Kv + CS) * res + np.array([res // 3, -(res // 2), res // 5])
    d_in = np.concatenate([g.integers(-32768, 32769, (N_RANDOM, 3)), SPECIAL])
    towards = 1 if x_lone > K[0] else -1
    x_from = (K[0] + 3) * CS + 5 if towards > 0 else (K[0] - 1) * CS - 5  # a voxel in the absent chunk next but one to the block
    o_gap = np.array([x_from * res + 1, (Kv[1] + 20) * res + 2, (Kv[2] + 30) * res], dtype=np.int64)
    lone_lo = np.array([x_lone * CS, Kv[1], Kv[2]], dtype=np.int64)
    tgt = (lone_lo + g.integers(2, CS - 2, (256, 3))) * res
    tgt[:, 0] = (lone_lo[0] + (2 if towards > 0 else CS - 3)) * res  # the face of the isolated chunk that looks at the block
    d_gap = np.concatenate([tgt - o_gap, -(tgt - o_gap)[:16], np.array([[towards, 0, 0], [towards * 4096, 1, -1]])])
    reach = (GAP + 1) * CS * res
    if where != "near":
        reach = I32 - 2 * res - int(np.abs(o_gap).max())  # |o| + max_range + 2 res == INT32_MAX exactly
        assert reach > (GAP - 2) * CS * res
    return {"in": (o_in, d_in, 60 * res), "gap": (o_gap, d_gap, int(reach))}


def store_model(res, where, name, box=None, any_weight=False):
    o, d, rng = store_rays(res, where)[name]
    lo, hi = (None, None) if box is None else box
    return R.model(H.Chunks(store_chunks(res, where), lo, hi, base=store_base(res, where)), res, o, d, rng, any_weight)


STORE_CASES = [(res, where) for res in STORE_RES for where in ("near", "+", "-")]


def store_id(case):
    return f"res{case[0]}{case[1]}"


# ------------------------------------------------------------------------------------------------ helpers on the device
def upload(res, pos):
    return R.upload(SIZE, pos, OFF, entries(), res=res)


def moved(rec, s_mm):
    """ray records moved by s_mm where they hit"""
    out = rec.copy()
    hit = rec["range_mm"] >= 0
    for k, name in enumerate(("x_mm", "y_mm", "z_mm")):
        out[name][hit] = rec[name][hit] + int(s_mm[k])
    return out


def moved_vert(vert, s_mm):
    out = vert.copy()
    for k, name in enumerate(("x_mm", "y_mm", "z_mm")):
        out[name] = vert[name] + int(s_mm[k])
    return out


def moved_surface(rec, s):
    out = rec.copy()
    for k, name in enumerate("xyz"):
        out[name] = rec[name] + int(s[k])
    return out


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
    assert G.same(last_map_records(t, len(d)), want[0])
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
    lo, hi = G.window(SIZE, pos)
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
        assert len(want_rec) > 100 and G.same(rec, want_rec) and G.same(mk, want_mk), name
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
    assert len(ra) > 100 and G.same(rb, moved_surface(ra, s))
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
        want = R.model(H.Chunks(store_chunks(res, where), base=store_base(res, where)), res, o, tgt, rng, False, True)
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
        lo, hi = G.window(view.size_, view.pos_)
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
