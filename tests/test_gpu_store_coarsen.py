"""ws_store_coarsen — a global map in device memory at half the resolution of another (the rule is stated in include/warpsense_hip.h)
against the numpy model of coarsen_model.py.  Every comparison is bit for bit: the key set, every chunk and the four statistics."""
import ctypes as C

import numpy as np
import pytest

import coarsen_model as CM
import fuse_scenes as S
from fuse_scenes import FILL, RES, TAU

pytestmark = pytest.mark.gpu

WS_OK, WS_ERR_INVALID, WS_ERR_CAPACITY = 0, -1, -4


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_coarsen(dst, src, keys=None, n_keys=None, min_observed=8, flags=0, stats=True):
    """(status, stats) of the C entry point itself"""
    out = np.full(4, 77, dtype=np.uint64)
    k = None if keys is None else np.ascontiguousarray(np.asarray(keys, dtype=np.int32).reshape(-1, 3))
    n = (0 if k is None else len(k)) if n_keys is None else n_keys
    L = (dst or src)._L
    rc = L.ws_store_coarsen(dst.handle if dst else None, src.handle if src else None, _p(k), n, int(min_observed), int(flags), _p(out) if stats else None)
    return rc, out


def check(dst_chunks, src_chunks, keys=None, min_observed=8):
    """coarsen on the device and compare with the model; returns (DST's chunks, stats)"""
    want, want_stats = CM.coarsen(dst_chunks, src_chunks, keys, min_observed, FILL)
    dst, src = S.make_store(dst_chunks), S.make_store(src_chunks)
    st = src.coarsen(dst, keys, min_observed)
    got = S.read(dst)
    print("stats", st, "model", want_stats)
    assert st.as_tuple() == tuple(want_stats), (st, want_stats)
    assert CM.same(got, want)
    assert CM.same(S.read(src), src_chunks)  # SRC is only read
    return got, st


def observed(seed):
    """a chunk of random entries, every weight > 0"""
    rng = np.random.default_rng(seed)
    return CM.pack(rng.integers(-TAU, TAU + 1, CM.CW), rng.integers(1, 700, CM.CW))


def test_one_chunk_is_one_octant_of_its_parent():
    src = {(0, 0, 0): S.draw(1, True)}
    for m in (1, 8):
        got, st = check({}, src, None, m)
        data = got[(0, 0, 0)].reshape(64, 64, 64)
        inside = np.zeros((64, 64, 64), dtype=bool)
        inside[:32, :32, :32] = True
        assert sorted(got) == [(0, 0, 0)] and np.all(data[~inside] == FILL) and st.created == 1 and 1000 < st.valued <= 32 ** 3
        assert np.count_nonzero(data[inside] != FILL) == st.valued


@pytest.mark.parametrize("min_observed", [1, 4, 8])
def test_all_eight_children(min_observed):
    """weights 0 and negative, values +-32767 and -32768"""
    src = {}
    for c in range(8):
        chunk = S.draw(20 + c, False).copy()
        chunk[c::97] = CM.pack(-32768, 3)
        chunk[(c + 5)::89] = CM.pack(-32768, 32767)
        src[(c >> 2, (c >> 1) & 1, c & 1)] = chunk
    got, st = check({}, src, None, min_observed)
    assert sorted(got) == [(0, 0, 0)] and st.valued > 1000 and (min_observed == 1 or st.short > 1000) and np.any(CM.unpack(got[(0, 0, 0)])[0] < -TAU)


def test_negative_and_mixed_keys():
    src = {(-1, -1, -1): observed(31), (-3, 2, -2): observed(32), (1, 0, 0): observed(33), (2, 0, 0): observed(34),
           (10, 10, 11): observed(35), (11, 10, 11): observed(36)}  # parent (5, 5, 5) has its cz = 1 children only
    got, st = check({}, src)
    assert sorted(got) == sorted([(-1, -1, -1), (-2, 1, -1), (0, 0, 0), (1, 0, 0), (5, 5, 5)]) and st.created == 5 and st.valued == 6 * 32 ** 3
    for key, octant in [((-1, -1, -1), (1, 1, 1)), ((-2, 1, -1), (1, 0, 0)), ((0, 0, 0), (1, 0, 0)), ((1, 0, 0), (0, 0, 0))]:
        data = got[key].reshape(64, 64, 64)
        inside = np.zeros((64, 64, 64), dtype=bool)
        inside[tuple(slice(32 * o, 32 * o + 32) for o in octant)] = True
        assert np.all(data[~inside] == FILL) and np.all(data[inside] != FILL), key
    half = got[(5, 5, 5)].reshape(64, 64, 64)
    assert np.all(half[:, :, :32] == FILL) and np.all(half[:, 32:, :] == FILL) and np.all(half[:, :32, 32:] != FILL)


def test_listed_keys():
    """only listed parents change; a listed parent without children is not created, an existing one becomes fill; an existing chunk
    is overwritten in all its words; duplicates are accepted"""
    src = {(0, 0, 0): observed(41), (1, 1, 1): observed(42), (2, 0, 0): observed(43), (4, 4, 4): observed(44)}
    dst = {(0, 0, 0): S.draw(45, False), (1, 0, 0): S.draw(46, False), (7, 7, 7): S.draw(47, False), (-1, 0, 0): S.draw(48, False)}
    keys = [(7, 7, 7), (0, 0, 0), (9, 9, 9), (0, 0, 0), (2, 2, 2), (7, 7, 7)]
    got, st = check(dst, src, keys)
    assert sorted(got) == sorted(list(dst) + [(2, 2, 2)]) and st.as_tuple() == (3, 1, 3 * 32 ** 3, 0)
    assert np.all(got[(7, 7, 7)] == FILL) and np.all(got[(0, 0, 0)].reshape(64, 64, 64)[:32, 32:, :] == FILL)  # nothing of the old chunks is left
    assert np.array_equal(got[(1, 0, 0)], dst[(1, 0, 0)]) and np.array_equal(got[(-1, 0, 0)], dst[(-1, 0, 0)])  # (1, 0, 0) has a child but is not listed
    # an empty list is a call that does nothing
    store, other = S.make_store(dst), S.make_store(src)
    rc, stats = raw_coarsen(store, other, np.zeros((0, 3), dtype=np.int32))
    assert rc == WS_OK and np.all(stats == 0) and CM.same(S.read(store), dst)


def lookup(chunks, voxels, fill):
    """the raw entries of world voxels (n, 3) in a dictionary of chunks"""
    v = np.asarray(voxels, dtype=np.int64)
    out = np.full(len(v), fill, dtype=np.uint32)
    key, loc = np.floor_divide(v, 64), np.mod(v, 64)
    for i, k in enumerate(map(tuple, key.tolist())):
        if k in chunks:
            out[i] = chunks[k][loc[i, 0] * 4096 + loc[i, 1] * 64 + loc[i, 2]]
    return out


def test_the_entry_is_the_sample_at_the_coarse_centre():
    """resolution 64, min_observed 8: at the centre (2 V + 1) r of a coarse voxel every trilinear fraction is r / 2, so where the
    sample's cell is valid its d_mm and weight are the coarse entry's value and weight, and where it is not the entry is fill"""
    chunks = S.sphere_and_floor()
    base, dst = S.make_store(chunks), S.make_store({})
    base.coarsen(dst)
    got = S.read(dst)
    block = lambda x, y, z: np.stack(np.meshgrid(np.arange(*x), np.arange(*y), np.arange(*z), indexing="ij"), axis=-1).reshape(-1, 3)
    V = np.concatenate([block((8, 24), (-8, 8), (0, 8)), block((-8, 8), (-8, 8), (-24, -16))])  # across the sphere's surface, across the floor
    assert len(V) == 4096
    rec = base.sample(RES, ((2 * V + 1) * RES).astype(np.int32), TAU)[0]
    valid = rec["cls"] != 0
    entry = lookup(got, V, FILL)
    value, weight = CM.unpack(entry)
    print("valid cells", int(valid.sum()), "of", len(V))
    assert valid.sum() > 500 and (~valid).sum() > 500
    assert np.array_equal(rec["d_mm"][valid], value[valid]) and np.array_equal(rec["weight"][valid], weight[valid]) and np.all(weight[valid] > 0)
    assert np.all(entry[~valid] == FILL)


_PYRAMID = {}


def pyramid_case():
    if not _PYRAMID:
        base = dict(S.sphere_and_floor())
        base[(5, -3, 2)] = observed(61)
        _PYRAMID.update(base=base, levels=CM.pyramid(base, 3, 8, FILL))
    return _PYRAMID


def read_levels(p):
    return [S.read(p.store(l)) for l in range(p.levels + 1)]


def test_pyramid_is_the_model_applied_three_times():
    import warpsense_amd as W
    import store_scenes as SM
    g = pyramid_case()
    p = W.MapPyramid(S.make_store(g["base"]), 3, RES, segment_chunks=2)
    stats = p.rebuild()
    assert [p.resolution(l) for l in range(4)] == [RES, 2 * RES, 4 * RES, 8 * RES] and p.store(0) is p.base
    for l, (got, want) in enumerate(zip(read_levels(p), g["levels"])):
        assert CM.same(got, want), l
    assert [s.chunks for s in stats] == [len(g["levels"][l]) for l in (1, 2, 3)] and stats[0].valued > 1000
    # the mesh of level 1 at twice the resolution is the mesh model's on the model's level-1 chunks
    vert, face = p.store(1).mesh(p.resolution(1))
    mv, mf = SM.model_store(g["levels"][1], 2 * RES)
    assert vert.tobytes() == mv.tobytes() and face.tobytes() == mf.tobytes() and len(vert) > 100
    p.close()


def test_refresh_of_a_box_equals_a_rebuild():
    import warpsense_amd as W
    g = pyramid_case()
    p = W.MapPyramid(S.make_store(g["base"]), 3, RES, segment_chunks=2)
    p.rebuild()
    changed = dict(g["base"])
    changed[(-1, 0, -1)] = observed(62)
    p.base.put_chunk((-1, 0, -1), changed[(-1, 0, -1)])
    before = read_levels(p)
    stats = p.refresh((-64, 0, -64), (-1, 63, -1))
    assert [s.chunks for s in stats] == [1, 1, 1] and [s.created for s in stats] == [0, 0, 0]
    full = W.MapPyramid(S.make_store(changed), 3, RES, segment_chunks=2)
    full.rebuild()
    after = read_levels(p)
    for l, (got, want, model) in enumerate(zip(after, read_levels(full), CM.pyramid(changed, 3, 8, FILL))):
        assert CM.same(got, want) and CM.same(got, model), l
    assert not CM.same(after[1], before[1]) and sum(not np.array_equal(after[1][k], before[1][k]) for k in before[1]) == 1
    p.close(), full.close()


def test_refusals_change_nothing():
    import warpsense_amd as W
    src_chunks = {(0, 0, 0): observed(71), (2, 0, 0): observed(72), (4, 0, 0): observed(73)}
    dst_chunks = {(0, 0, 0): S.draw(74, False), (9, 9, 9): S.draw(75, False)}
    dst, src = S.make_store(dst_chunks, max_chunks=3), S.make_store(src_chunks)  # the call needs (1, 0, 0) and (2, 0, 0): four chunks
    foreign = W.DeviceGlobalMap(TAU, 0, ctx=W.Context(0))
    observed_fill = S.make_store(dst_chunks, fill=(TAU, 1))
    keys = np.array([[0, 0, 0]], dtype=np.int32)
    cases = [dict(dst=None, src=src), dict(dst=dst, src=None), dict(dst=dst, src=dst), dict(dst=dst, src=foreign), dict(dst=dst, src=src, min_observed=0),
             dict(dst=dst, src=src, min_observed=9), dict(dst=dst, src=src, min_observed=-1), dict(dst=dst, src=src, flags=1), dict(dst=dst, src=src, flags=0x80000000),
             dict(dst=dst, src=src, keys=None, n_keys=1), dict(dst=observed_fill, src=src)]
    for kw in cases:
        rc, stats = raw_coarsen(**kw)
        assert rc == WS_ERR_INVALID and np.all(stats == 77), kw
        assert dst._L.ws_last_error().decode().startswith("ws_store_coarsen:")
    # capacity one chunk short
    rc, stats = raw_coarsen(dst, src)
    assert rc == WS_ERR_CAPACITY and np.all(stats == 77)
    assert dst.keys() == sorted(dst_chunks) and CM.same(S.read(dst), dst_chunks) and CM.same(S.read(src), src_chunks)
    assert CM.same(S.read(observed_fill), dst_chunks)
    # one more chunk allowed: the same stores coarsen
    roomy = S.make_store(dst_chunks, max_chunks=4)
    assert src.coarsen(roomy).as_tuple() == tuple(CM.coarsen(dst_chunks, src_chunks, None, 8, FILL)[1]) and roomy.count() == 4
    # with listed keys that exist the short store is enough
    assert raw_coarsen(dst, src, keys)[0] == WS_OK and dst.count() == 2
    foreign.close()


def window_case():
    import raycast_model as R
    size = (33, 33, 33)
    rng = np.random.default_rng(12)
    # the window [-16, 16]^3 around the origin; with offset = size / 2 storage order is world order
    box = CM.pack(rng.integers(-TAU, TAU, size), rng.integers(1, 50, size))
    t, _ = R.upload(size, (0, 0, 0), tuple(s // 2 for s in size), [box, box], tau=TAU, mw=S.MW, res=RES)
    return t, box


def test_ordering_without_a_host_wait():
    """save_box -> coarsen(stats=False) -> mesh of DST, all enqueued without a wait, gives the bytes of the synchronised sequence"""
    t, box = window_case()
    meshes = []
    for wait in (False, True):
        src, dst = S.make_store({}), S.make_store({})
        src.save_box(t, (-16, -16, -16), (16, 16, 16))
        if wait:
            src.ctx.sync()
        assert src.coarsen(dst, min_observed=1, stats=wait) is None or wait
        if wait:
            dst.ctx.sync()
        vert, face = dst.mesh(2 * RES)
        meshes.append((vert.tobytes(), face.tobytes(), S.read(dst)))
    assert meshes[0][0] == meshes[1][0] and meshes[0][1] == meshes[1][1] and len(meshes[0][0]) > 0 and CM.same(meshes[0][2], meshes[1][2])
    src_chunks = {}
    for key in [(i, j, k) for i in (-1, 0) for j in (-1, 0) for k in (-1, 0)]:
        c = np.full((64, 64, 64), FILL, dtype=np.uint32)
        c[tuple(slice(48, 64) if k < 0 else slice(0, 17) for k in key)] = box[tuple(slice(0, 16) if k < 0 else slice(16, 33) for k in key)]
        src_chunks[key] = c.reshape(-1)
    assert CM.same(meshes[0][2], CM.coarsen({}, src_chunks, None, 1, FILL)[0])


def test_two_runs_give_equal_bytes_and_timing():
    g = pyramid_case()
    runs = []
    for _ in range(2):
        dst, src = S.make_store({}), S.make_store(g["base"])
        dst.coarsen_timing(1)
        st = src.coarsen(dst, None, 4)
        ms = dst.coarsen_timing()
        assert len(ms) == 2 and ms[1] > 0
        runs.append((S.read(dst), st.as_tuple()))
    assert CM.same(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] == tuple(CM.coarsen({}, g["base"], None, 4, FILL)[1])


def test_global_pyramid_and_global_mesh_level():
    """TSDFMapping.global_pyramid after real use: the window goes into the store, the levels are the model's of the store's chunks; after a
    shift and another scan the refreshed pyramid equals a rebuilt one; global_mesh(level=1) is the mesh of level 1, level=0 the bytes of
    the plain call"""
    import warpsense_amd as W
    import store_scenes as SM
    from window_routes import _params
    size = (65, 65, 65)
    store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size), W.LocalMap(*size, SM.TAU, 0), device_global_map=store)
    fill = int(W.pack_entry(SM.TAU, 0))
    tm.update_tsdf(SM.walk_scan(0), pos_rm=SM.WALK[0], up_rm=(0, 0, 32768))
    p = tm.global_pyramid(2, min_observed=4, segment_chunks=2)
    want = CM.pyramid(S.read(store), 2, 4, fill)
    assert CM.same(S.read(p.store(1)), want[1]) and CM.same(S.read(p.store(2)), want[2]) and len(want[1]) > 0
    plain = tm.global_mesh()
    tm.shift_map_device(SM.WALK[1])
    tm.update_tsdf(SM.walk_scan(1), pos_rm=SM.WALK[1], up_rm=(0, 0, 32768))
    assert tm.global_pyramid(2, min_observed=4) is p
    want = CM.pyramid(S.read(store), 2, 4, fill)
    assert CM.same(S.read(p.store(1)), want[1]) and CM.same(S.read(p.store(2)), want[2])
    vert, face = tm.global_mesh(level=1)
    mv, mf = SM.model_store(want[1], 2 * SM.RES)
    assert vert.tobytes() == mv.tobytes() and face.tobytes() == mf.tobytes()
    again = tm.global_mesh(level=0)
    direct = store.mesh(SM.RES)
    assert again[0].tobytes() == direct[0].tobytes() and again[1].tobytes() == direct[1].tobytes() and len(plain[0]) > 0
    p.close(), store.close()
