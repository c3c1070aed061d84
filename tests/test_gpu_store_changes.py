"""ws_store_changes — where one global map in device memory differs from another under a rigid pose (the rule is stated in
include/warpsense_hip.h) against the numpy model of changes_model.py.  Every comparison is bit for bit: records, labels, cluster
table and the six statistics."""
import ctypes as C

import numpy as np
import pytest

import changes_model as M
import frontier_model as FM
import fuse_model as F
import fuse_scenes as S
from changes_scenes import BAND, EDGES, FREE, draw, pose_maps, scene
from fuse_scenes import FILL, RES, TAU

pytestmark = pytest.mark.gpu

WS_OK, WS_ERR_INVALID, WS_ERR_RANGE = 0, -1, -5
ALL = M.APPEARED | M.VANISHED | M.CLUSTERS


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def got_of(res):
    return res.records, res.labels, res.clusters, res.stats.as_tuple()


def check(cur_chunks, ref_chunks, pose, res=RES, band=BAND, free_value=FREE, mw=1, lo=None, hi=None, flags=ALL, stores=None):
    """changes on the device against the model; returns the model's tuple"""
    want = M.changes(cur_chunks, ref_chunks, pose, res, band, free_value, mw, lo, hi, flags)
    cur, ref = stores or (S.make_store(cur_chunks), S.make_store(ref_chunks))
    kinds = {3: "both", 1: "appeared", 2: "vanished"}[flags & 3]
    got = cur.changes(ref, pose, resolution=res, band=band, free_value=free_value, min_weight=mw, lo=lo, hi=hi, kinds=kinds, clusters=bool(flags & M.CLUSTERS))
    assert got.stats.as_tuple() == tuple(int(v) for v in want[3]), (got.stats, want[3])
    assert M.same(got_of(got), want)
    if stores is None:
        assert F.same((S.read(cur), ()), (cur_chunks, ())) and F.same((S.read(ref), ()), (ref_chunks, ()))  # both are only read
    return want


def test_one_chunk_with_every_pair_of_classes():
    """the identity pose: every value edge against every value edge, every weight against every weight around min_weight 2"""
    n = len(EDGES)
    w = np.array([-5, 0, 1, 2, 32767])
    cur, ref = draw(1), draw(2)
    ev, nv = np.repeat(EDGES, n), np.tile(EDGES, n)
    cur[:n * n], ref[:n * n] = F.pack(ev, 5), F.pack(nv, 5)
    cur[4096:4096 + 25], ref[4096:4096 + 25] = F.pack(0, np.repeat(w, 5)), F.pack(FREE, np.tile(w, 5))
    for mw in (1, 2):
        want = check({(0, 0, 0): cur}, {(0, 0, 0): ref}, F.identity_pose(), mw=mw)
        direct, dstats = M.direct({(0, 0, 0): cur}, {(0, 0, 0): ref}, BAND, FREE, mw)
        assert want[0].tobytes() == direct.tobytes() and want[3].tolist() == [1] + dstats
        assert want[3][2] > 1000 and want[3][3] > 1000 and want[3][4] > 1000 and len(want[2]) > 1


def test_a_store_against_its_byte_copy():
    chunks = {(0, 0, 0): draw(3), (-1, 2, 0): draw(4)}
    want = check(chunks, dict(chunks), F.identity_pose((77, -5, 1000)), mw=2)
    assert len(want[0]) == 0 and want[3].tolist() == [2, sum(int((F.unpack(c)[1] >= 2).sum()) for c in chunks.values()), 0, 0, 0, 0]


def corner_case():
    """2 x 2 x 2 chunks with keys -1 and 0: everything observed free on both sides but the voxels at local 0 and 63 on every axis,
    which are occupied in one of the maps; (0, 0, -1) is in CUR only, (-1, -1, 0) in REF only"""
    free, cur, ref = np.full((64, 64, 64), F.pack(TAU, 9), dtype=np.uint32), {}, {}
    for i, key in enumerate((a, b, c) for a in (-1, 0) for b in (-1, 0) for c in (-1, 0)):
        one, two = free.copy(), free.copy()
        for j, l in enumerate((x, y, z) for x in (0, 63) for y in (0, 63) for z in (0, 63)):
            (one if (i + j) & 1 else two)[l] = F.pack(-3 + j, 4 + i)
        cur[key], ref[key] = one.reshape(-1), two.reshape(-1)
    del ref[(0, 0, -1)], cur[(-1, -1, 0)]
    return cur, ref


def test_2x2x2_chunks_with_negative_keys_and_missing_chunks():
    cur, ref = corner_case()
    want = check(cur, ref, F.identity_pose())
    assert want[3].tolist() == [7, 6 * F.CW, 6 * 4, 6 * 4, F.CW, want[3][5]] and len(want[0]) == 48
    # the eight voxels around the common corner are one cluster of both kinds where their chunks are compared
    assert int(want[2]["count"].max()) >= 6 and set(want[0]["kind"].tolist()) == {1, 2}


def test_boxes():
    cur, ref = {(0, 0, 0): draw(11), (1, 0, 0): draw(12), (0, -1, 0): draw(13)}, {(0, 0, 0): draw(14), (1, 0, 0): draw(15), (0, -1, 0): draw(16)}
    stores = S.make_store(cur), S.make_store(ref)
    cut = check(cur, ref, F.identity_pose(), lo=(40, -9, 3), hi=(70, 20, 60), stores=stores)
    assert cut[3][0] == 3 and len(cut[0]) > 100 and cut[0]["x"].min() == 40 and cut[0]["x"].max() == 70 and cut[0]["y"].min() == -9 and cut[0]["z"].max() == 60
    one = check(cur, ref, F.identity_pose(), lo=(64, 0, 0), hi=(64, 63, 63), stores=stores)
    assert one[3][0] == 1 and set(one[0]["x"].tolist()) == {64}
    whole = check(cur, ref, F.identity_pose(), stores=stores)
    assert whole[3][0] == 3 and whole[3][1] > cut[3][1] > one[3][1] > 0
    nothing = check(cur, ref, F.identity_pose(), lo=(200, 200, 200), hi=(300, 300, 300), stores=stores)
    assert len(nothing[0]) == 0 and nothing[3].tolist() == [0] * 6 and nothing[1].shape == (0,) and nothing[2].shape == (0,)


def test_translation_that_is_no_multiple_of_the_resolution():
    import warpsense_amd as W
    cur, ref = pose_maps()
    want = check(cur, ref, W.fuse_pose(S.rot(t=(RES + 13, -2 * RES - 40, 7))), mw=2)
    assert want[3][1] > 100000 and want[3][4] > 10000 and len(want[0]) > 1000


def test_quarter_turn_about_z_is_a_lattice_permutation():
    import warpsense_amd as W
    cur, ref = {(0, 0, 0): draw(32)}, {(0, 0, 0): draw(33)}
    c = 32 * RES + RES // 2  # the centre of voxel 32
    T = S.rot(90)
    T[:3, 3] = np.array([c, c, c]) - T[:3, :3] @ np.array([c, c, c])
    pose = W.fuse_pose(T, (c, c, c))
    assert set(np.abs(pose[:9].astype(np.int64)).tolist()) == {0, F.Q30}
    want = check(cur, ref, pose)
    # every sample is one REF voxel: the plain comparison with the permuted chunk, where the image lies in the chunk
    v = M.LOCAL
    u = (v - 32) @ (pose[:9].reshape(3, 3).astype(np.int64) // F.Q30).T + 32
    inside = np.all((u >= 0) & (u < 64), axis=1)
    turned = np.where(inside, ref[(0, 0, 0)][np.clip(u[:, 0], 0, 63) * 4096 + np.clip(u[:, 1], 0, 63) * 64 + np.clip(u[:, 2], 0, 63)], F.pack(0, 0)).astype(np.uint32)
    direct, dstats = M.direct(cur, {(0, 0, 0): turned}, BAND, FREE)
    assert want[0].tobytes() == direct.tobytes() and want[3].tolist() == [1] + dstats and len(direct) > 1000


@pytest.mark.parametrize("res", [7, 64])
def test_general_rotation_with_a_fractional_translation(res):
    import warpsense_amd as W
    cur, ref = pose_maps()
    pose = W.fuse_pose(S.rot(4, -2, 3, (13 * res / 64, -7.4, 4.2)), (32 * res, 64 * res, 32 * res))
    want = check(cur, ref, pose, res=res)
    assert want[3][1] > 50000 and len(want[0]) > 500 and want[3][4] > 10000


def test_the_reach_and_a_dead_sample():
    """resolution 1024, pivot 0: the chunk with key 255 ends 512 mm inside 2^24 mm, the chunk with key 256 begins outside"""
    cur = {(255, 0, 0): draw(41), (256, 0, 0): draw(42)}
    ref = {(255, 0, 0): draw(43), (256, 0, 0): draw(44)}
    want = check(cur, ref, F.identity_pose(), res=1024)
    near = M.changes({(255, 0, 0): cur[(255, 0, 0)]}, ref, F.identity_pose(), 1024, BAND, FREE, flags=ALL)
    assert want[3].tolist() == [2] + near[3].tolist()[1:] and want[0].tobytes() == near[0].tobytes() and len(want[0]) > 1000 and want[0]["x"].max() < 256 * 64
    dead = F.identity_pose()
    dead[12] = 2 ** 30 - 255 * 64 * 1024  # q_x >= 2^30 for every voxel of the near chunk
    want = check(cur, ref, dead, res=1024)
    assert len(want[0]) == 0 and want[3].tolist() == [2, 0, 0, 0, int((F.unpack(cur[(255, 0, 0)])[1] >= 1).sum()), 0]


def test_scene_with_a_box_added_and_a_pillar_removed():
    s = scene()
    want = check(s["cur"], s["ref"], F.identity_pose())
    rec, labels, table, stats = want
    assert len(table) == 2 and stats[2] == 8 ** 3 and stats[3] == 3 * 3 * 41
    for k, (name, kind) in enumerate((("pillar", 2), ("box", 1))):  # numbered by first member: the pillar has the smaller x
        assert table["count"][k] == (stats[3] if kind == 2 else stats[2]) and set(rec["kind"][labels == k].tolist()) == {kind}
        assert table["lo"][k].tolist() == list(s[name][0]) and table["hi"][k].tolist() == list(s[name][1])
    assert set(rec["ref_value"][rec["kind"] == 2].tolist()) == {0} and set(rec["ref_value"][rec["kind"] == 1].tolist()) == {TAU}


def test_kind_selection_and_repeatability():
    s = scene()
    stores = S.make_store(s["cur"]), S.make_store(s["ref"])
    full = check(s["cur"], s["ref"], F.identity_pose(), stores=stores)
    for flag in (M.APPEARED, M.VANISHED):
        part = check(s["cur"], s["ref"], F.identity_pose(), flags=flag | M.CLUSTERS, stores=stores)
        assert part[0].tobytes() == full[0][full[0]["kind"] == flag].tobytes() and part[3].tolist() == full[3].tolist() and len(part[2]) == 1
    runs = [got_of(stores[0].changes(stores[1], resolution=RES, band=BAND, free_value=FREE, clusters=True)) for _ in range(2)]
    assert M.same(runs[0], runs[1]) and M.same(runs[0], full)
    assert M.same(got_of(S.make_store(s["cur"]).changes(S.make_store(s["ref"]), resolution=RES, band=BAND, free_value=FREE, clusters=True)), full)


def raw_call(cur, ref, pose, res=RES, lo=None, hi=None, band=BAND, free_value=FREE, mw=1, flags=3, stats=True):
    n, k, st = C.c_size_t(77), C.c_size_t(77), np.full(6, 77, dtype=np.uint64)
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    pose = None if pose is None else np.ascontiguousarray(pose, dtype=np.int32)
    L = (cur or ref)._L
    rc = L.ws_store_changes(cur.handle if cur else None, ref.handle if ref else None, _p(pose), res, _p(a), _p(b), band, free_value, mw, flags, C.byref(n), C.byref(k),
                            _p(st) if stats else None)
    return rc, n.value, k.value, st.tolist()


def download(store, want):
    n, k = C.c_size_t(0), C.c_size_t(0)
    rec, lab, tab = np.zeros(len(want[0]), M.RECORD), np.zeros(len(want[0]), np.uint32), np.zeros(len(want[2]), FM.CLUSTER)
    assert store._L.ws_store_changes_download(store.handle, _p(rec), _p(lab), _p(tab), len(rec), len(tab), C.byref(n), C.byref(k)) == WS_OK
    return (n.value, k.value) == (len(rec), len(tab)) and rec.tobytes() == want[0].tobytes() and lab.tobytes() == want[1].tobytes() and tab.tobytes() == want[2].tobytes()


def test_refusals_leave_the_last_result_and_the_frontier_is_apart():
    import warpsense_amd as W
    s = scene()
    cur, ref = S.make_store(s["cur"]), S.make_store(s["ref"])
    want = check(s["cur"], s["ref"], F.identity_pose(), stores=(cur, ref))
    ident = F.identity_pose()
    bad_rot = ident.copy()
    bad_rot[4] = F.Q30 + 1
    other = W.Context(0)
    foreign = W.DeviceGlobalMap(TAU, 0, ctx=other)
    a, b = (-64,) * 3, (63,) * 3
    invalid = [dict(cur=None), dict(ref=None), dict(pose=None), dict(stats=False), dict(ref=cur), dict(ref=foreign), dict(pose=bad_rot), dict(lo=a), dict(hi=b),
               dict(lo=b, hi=a), dict(flags=8 | 3), dict(flags=4), dict(flags=0)]
    # (the two WS_ERR_RANGE refusals for 2^19 chunks or more, of REF and of CUR in the box, need half a terabyte of chunks: they are
    # covered only by reading store_lookup_plan and the listed.size() check of ws_store_changes in api_store_pair.hip)
    ranged = [dict(res=0), dict(res=1025), dict(band=0), dict(free_value=BAND - 1), dict(free_value=32768), dict(mw=0), dict(mw=32768)]
    for code, cases in ((WS_ERR_INVALID, invalid), (WS_ERR_RANGE, ranged)):
        for kw in cases:
            args = dict(cur=cur, ref=ref, pose=ident)
            args.update(kw)
            assert raw_call(**args) == (code, 77, 77, [77] * 6), kw
            assert download(cur, want), kw
    foreign.close()
    # a frontier call in between: both results stay what they were
    grown = dict(lo=(-65,) * 3, hi=(64,) * 3, clusters=True)  # one voxel more than the bounding box: its observed-free faces are frontier
    front = cur.frontier(**grown)
    assert len(front[0]) > 0 and download(cur, want)
    again = cur.changes(ref, resolution=RES, band=BAND, free_value=FREE, kinds="appeared")
    assert len(again.records) == want[3][2]
    n = C.c_size_t(0)
    assert cur._L.ws_store_frontier_records_dev(cur.handle, C.byref(n)) is not None and n.value == len(front[0])  # the frontier's result is still there
    rec, lab, tab = np.zeros(len(front[0]), FM.RECORD), np.zeros(len(front[0]), np.uint32), np.zeros(len(front[2]), FM.CLUSTER)
    k = C.c_size_t(0)
    assert cur._L.ws_store_frontier_download(cur.handle, _p(rec), _p(lab), _p(tab), len(rec), len(tab), C.byref(n), C.byref(k)) == WS_OK
    assert all(x.tobytes() == y.tobytes() for x, y in zip(front, (rec, lab, tab)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(front, cur.frontier(**grown)))
    cur.changes_timing(1)
    cur.changes(ref, resolution=RES, band=BAND, free_value=FREE, clusters=True)
    ms = cur.changes_timing(0)
    assert len(ms) == 4 and all(v > 0 for v in ms), ms


def test_an_empty_store_on_either_side():
    import warpsense_amd as W
    chunks = {(0, 0, 0): draw(51)}
    empty, full = W.DeviceGlobalMap(TAU, 0), S.make_store(chunks)
    assert raw_call(empty, full, F.identity_pose(), flags=7) == (WS_OK, 0, 0, [0] * 6)
    n = C.c_size_t(9)
    assert empty._L.ws_store_changes_records_dev(empty.handle, C.byref(n)) is None and n.value == 0
    want = check(chunks, {}, F.identity_pose(), stores=(full, empty))
    assert len(want[0]) == 0 and want[3].tolist() == [1, 0, 0, 0, int((F.unpack(chunks[(0, 0, 0)])[1] >= 1).sum()), 0]


def test_map_changes_after_a_scan_a_shift_and_another_scan():
    """the mapping layer: the store of the run after a scan, a device shift and a second scan against a copy of the store after the
    first scan; the records are the model's, so nothing has VANISHED where the model sees nothing"""
    import warpsense_amd as W
    import store_scenes as SM
    from window_routes import _params
    from warpsense_amd import synthetic as SY
    size, res = (65, 65, 65), SM.RES
    store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params(size), W.LocalMap(*size, SM.TAU, 0), device_global_map=store)
    room = dict(rings=32, azimuths=256, half_extents_mm=(1700.0, 1300.0, 900.0))
    tm.update_tsdf(np.rint(SY.os1_128_scan(sensor_mm=(0.0, 0.0, 0.0), seed=30, **room)).astype(np.int32), pos_rm=np.zeros(3, dtype=np.int32), up_rm=(0, 0, 32768))
    tm.global_surface_cloud()  # the window goes into the store
    before = S.read(store)
    ref = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    for key, data in before.items():
        ref.put_chunk(key, data)
    tm.shift_map_device((6, -3, 2))
    sensor = (6.0 * res, -3.0 * res, 2.0 * res)
    tm.update_tsdf(np.rint(SY.os1_128_scan(sensor_mm=sensor, seed=31, **room)).astype(np.int32), pos_rm=np.array([6, -3, 2], dtype=np.int32), up_rm=(0, 0, 32768))
    got = tm.map_changes(ref, clusters=True)
    want = M.changes(S.read(store), before, F.identity_pose(), res, res, SM.TAU, flags=ALL)
    print("map_changes:", got.stats, "records", len(got.records))
    assert M.same(got_of(got), want) and got.stats.known_both > 1000
    assert int((got.records["kind"] == 2).sum()) == int((want[0]["kind"] == 2).sum())
    store.close(), ref.close()
