"""ws_store_fuse — one global map in device memory fused into another under a rigid pose (the rule is stated in
include/warpsense_hip.h) against the numpy model of fuse_model.py.  Every comparison is bit for bit: the key set, every chunk and
the six statistics."""
import ctypes as C

import numpy as np
import pytest

import fuse_model as F
import fuse_scenes as S
from fuse_scenes import FILL, MW, RES, TAU

pytestmark = pytest.mark.gpu

WS_OK, WS_ERR_INVALID, WS_ERR_CAPACITY, WS_ERR_RANGE = 0, -1, -4, -5


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_fuse(dst, src, pose, res=RES, mw=MW, flags=0):
    """(status, stats) of the C entry point itself"""
    stats = np.full(6, 77, dtype=np.uint64)
    pose = None if pose is None else np.ascontiguousarray(pose, dtype=np.int32)
    rc = dst._L.ws_store_fuse(dst.handle if dst else None, src.handle if src else None, _p(pose), int(res), int(mw), int(flags), _p(stats))
    return rc, stats


def check(dst_chunks, src_chunks, pose, res=RES, mw=MW, want=None):
    """fuse on the device and compare with the model; returns (chunks, stats, model's pair)"""
    want = want or F.fuse(dst_chunks, src_chunks, pose, res, mw, FILL)
    dst, src = S.make_store(dst_chunks), S.make_store(src_chunks)
    st = dst.fuse(src, pose, mw, resolution=res)
    got = S.read(dst)
    assert st.as_tuple() == tuple(int(v) for v in want[1]), (st, want[1])
    assert F.same((got, st.as_tuple()), want)
    assert F.same((S.read(src), ()), (src_chunks, ()))  # SRC is only read
    return got, st, want


def test_identity_and_the_oracle_route():
    """1. 3 src and 3 dst chunks, two shared; weights 0, negative (dst), ew + nw beyond max_weight, values at +-32767"""
    dst, src = S.identity_case()
    got, st, _ = check(dst, src, F.identity_pose())
    for key, data in S.oracle_route(dst, src, MW, FILL).items():
        assert got[key].tobytes() == data.tobytes(), key
    assert st.created == 1 and st.averaged > 100000 and st.set > 100000
    # negative weights in SRC as well, against the model alone: the oracle would copy such an entry over an unobserved voxel (nw != 0),
    # the rule (valid iff weight > 0) leaves the voxel untouched
    negative = {k: S.draw(10 + i, False) for i, k in enumerate(sorted(src))}
    assert any(np.any(F.unpack(v)[1] < 0) for v in negative.values())
    check(dst, negative, F.identity_pose())


def test_whole_voxel_translation_across_chunk_borders():
    """2. a translation by whole voxels, negative keys on both sides: the samples cross chunk borders on every axis"""
    import warpsense_amd as W
    src = {(-1, -1, -1): S.draw(21, True), (-2, -1, -1): S.draw(22, True), (-1, 0, -2): S.draw(23, True)}
    dst = {(-3, -1, 1): S.draw(24, False), (-2, -1, 1): S.draw(25, False), (-3, -1, 2): S.draw(26, False)}
    pose = W.fuse_pose(S.rot(t=(-64 * RES - 3 * RES, 5 * RES, 130 * RES)))
    got, st, _ = check(dst, src, pose)
    assert st.averaged > 1000 and st.created >= 3 and min(k[0] for k in got) < -2


@pytest.mark.parametrize("angles", [(90, 0, 0), (0, 0, 180)])
def test_lattice_rotation_is_a_permutation(angles):
    """3. 90 degrees about z and 180 degrees about x around a lattice pivot: every sample is one src voxel, so the result is the
    oracle's integrate of the permuted src chunk"""
    import warpsense_amd as W
    src, dst = {(0, 0, 0): S.draw(31, True)}, {(0, 0, 0): S.draw(32, False)}
    c = 32 * RES + RES // 2  # the centre of voxel 32
    T = S.rot(*angles)
    T[:3, 3] = np.array([c, c, c]) - T[:3, :3] @ np.array([c, c, c])
    pose = W.fuse_pose(T, (c, c, c))
    assert set(np.abs(pose[:9].astype(np.int64)).tolist()) == {0, F.Q30} and pose[9:].tolist() == [c] * 6
    got, st, _ = check(dst, src, pose)
    v = np.stack(np.meshgrid(*(np.arange(64),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    u = (v - 32) @ (pose[:9].reshape(3, 3).astype(np.int64) // F.Q30).T + 32
    inside = np.all((u >= 0) & (u < 64), axis=1)
    new = np.where(inside, src[(0, 0, 0)][np.clip(u[:, 0], 0, 63) * 4096 + np.clip(u[:, 1], 0, 63) * 64 + np.clip(u[:, 2], 0, 63)], F.pack(0, 0)).astype(np.uint32)
    want = S.oracle_route(dst, {(0, 0, 0): new}, MW, FILL)
    assert got[(0, 0, 0)].tobytes() == want[(0, 0, 0)].tobytes() and st.averaged + st.set > 150000


_GENERAL = {}


def general_case():
    if not _GENERAL:
        import warpsense_amd as W
        src, dst = S.sphere_and_floor(), S.sphere_and_floor(shift=(0.4, -0.3, 0.2), weight=35)
        del dst[(0, 0, 0)]
        pose = W.fuse_pose(S.rot(17, 3, 0, (13, -7, 4)))
        _GENERAL.update(src=src, dst=dst, pose=pose, want=F.fuse(dst, src, pose, RES, MW, FILL))
    return _GENERAL


def test_general_pose_on_sphere_and_floor():
    """4. 17 degrees yaw, 3 degrees pitch, (13, -7, 4) mm on a sphere-and-floor TSDF in 2 x 2 x 2 chunks: the created chunks are
    exactly the model's"""
    g = general_case()
    got, st, want = check(g["dst"], g["src"], g["pose"], want=g["want"])
    assert st.created >= 1 and st.averaged > 10000 and st.set > 1000 and set(got) - set(g["dst"]) == set(want[0]) - set(g["dst"])


def test_single_voxels_at_the_ends_of_the_loops():
    """5. one qualifying voxel at local (63, 63, 63) of a dst chunk and one at (0, 0, 0) of its diagonal neighbour"""
    a, b = np.full(F.CW, FILL, dtype=np.uint32), np.full(F.CW, FILL, dtype=np.uint32)
    a[-1], b[0] = F.pack(-123, 7), F.pack(321, 9)
    got, st, _ = check({(0, 0, 0): S.draw(51, False)}, {(0, 0, 0): a, (1, 1, 1): b}, F.identity_pose())
    assert st.averaged + st.set == 2 and st.created == 1 and got[(1, 1, 1)][0] == F.pack(321, 9) and np.all(got[(1, 1, 1)][1:] == FILL)


def test_far_from_the_origin_and_the_reach():
    """6. pivots near +-2^29 mm: a src chunk inside 2^24 mm of the pivot is fused, one across the limit in part, one outside not at all"""
    k = (1 << 29) // (64 * RES)  # 2^17: the chunk whose first voxel centre is at 2^29 + 32 mm
    pivot = (k * 64 * RES - 1000, -(k * 64 * RES) + 1000, 0)
    n = (1 << 24) // (64 * RES)  # chunks per reach
    src = {(k + n - 2, -k, 0): S.draw(61, True), (k + n - 1, -k, 0): S.draw(62, True), (k + n, -k, 0): S.draw(63, True),
           (k, -k - n + 1, 0): S.draw(64, True), (k, -k - n - 1, 0): S.draw(65, True)}
    dst = {(k + n - 1, -k, 0): S.draw(66, False)}
    got, _, _ = check(dst, src, F.identity_pose(pivot))
    assert (k + n - 2, -k, 0) in got and (k + n, -k, 0) not in got and (k, -k - n - 1, 0) not in got
    part = got[(k + n - 1, -k, 0)].reshape(64, 64, 64)
    assert not np.array_equal(part[0], dst[(k + n - 1, -k, 0)].reshape(64, 64, 64)[0]) and np.array_equal(part[63], dst[(k + n - 1, -k, 0)].reshape(64, 64, 64)[63])


@pytest.mark.parametrize("res", [1, 7, 64, 1024])
def test_resolutions(res):
    """7. resolutions 1, 7 (odd: h truncated), 64 and 1024 under a general pose"""
    import warpsense_amd as W
    src, dst = {(0, 0, 0): S.draw(71, True), (0, 1, 0): S.draw(72, True)}, {(0, 0, 0): S.draw(73, False)}
    pose = W.fuse_pose(S.rot(5, 2, -3, (13 * res / 64, -7, 4)), (32 * res, 64 * res, 32 * res))
    _, st, _ = check(dst, src, pose, res=res)
    assert st.averaged > 1000 and st.set > 1000


def test_resolution_out_of_range_is_refused():
    dst_chunks = {(0, 0, 0): S.draw(73, False)}
    dst, src = S.make_store(dst_chunks), S.make_store({(0, 0, 0): S.draw(71, True)})
    for res in (1025, 0, -3):
        rc, stats = raw_fuse(dst, src, F.identity_pose(), res=res)
        assert rc == WS_ERR_RANGE and np.all(stats == 77)
    assert F.same((S.read(dst), ()), (dst_chunks, ()))


def test_count_only():
    """8. the statistics are the real call's; the keys and every chunk of DST are unchanged"""
    g = general_case()
    dst, src = S.make_store(g["dst"]), S.make_store(g["src"])
    st = dst.fuse(src, g["pose"], MW, count_only=True, resolution=RES)
    assert st.as_tuple() == tuple(int(v) for v in g["want"][1]) and st.created >= 1
    assert dst.keys() == sorted(g["dst"]) and F.same((S.read(dst), ()), (g["dst"], ()))
    assert st.disagreement_mm == st.sum_abs_diff / st.averaged


def test_refusals_change_nothing():
    """9. every refusal leaves DST's keys and bytes as they were, WS_ERR_CAPACITY one chunk short included"""
    import warpsense_amd as W
    g = general_case()
    need = len(g["want"][0])
    dst, src = S.make_store(g["dst"], max_chunks=need - 1), S.make_store(g["src"])
    bad_rot = g["pose"].copy()
    bad_rot[4] = -F.Q30 - 1
    other = W.Context(0)
    foreign = W.DeviceGlobalMap(TAU, 0, ctx=other)
    observed_fill = S.make_store(g["dst"], fill=(TAU, 1))
    cases = [(None, src, g["pose"], MW, 0), (dst, None, g["pose"], MW, 0), (dst, src, None, MW, 0), (dst, dst, g["pose"], MW, 0), (dst, foreign, g["pose"], MW, 0),
             (dst, src, g["pose"], 0, 0), (dst, src, g["pose"], 32768, 0), (dst, src, bad_rot, MW, 0), (dst, src, g["pose"], MW, 2), (observed_fill, src, g["pose"], MW, 0)]
    for d, s, pose, mw, flags in cases:
        stats = np.full(6, 77, dtype=np.uint64)
        rc = dst._L.ws_store_fuse(d.handle if d else None, s.handle if s else None, _p(pose), RES, mw, flags, _p(stats))
        assert rc == WS_ERR_INVALID and np.all(stats == 77), (mw, flags)
    assert dst._L.ws_store_fuse(dst.handle, src.handle, _p(g["pose"]), RES, MW, 0, None) == WS_ERR_INVALID
    rc, stats = raw_fuse(dst, src, g["pose"])
    assert rc == WS_ERR_CAPACITY and np.all(stats == 77)
    assert dst.keys() == sorted(g["dst"]) and F.same((S.read(dst), ()), (g["dst"], ()))
    assert F.same((S.read(observed_fill), ()), (g["dst"], ()))
    # one more chunk allowed: the same stores fuse
    roomy = S.make_store(g["dst"], max_chunks=need)
    assert roomy.fuse(src, g["pose"], MW, resolution=RES).as_tuple() == tuple(int(v) for v in g["want"][1]) and roomy.count() == need
    foreign.close()


def test_empty_and_unobserved_src():
    """10. an empty SRC, and a SRC whose voxels all have weight <= 0: WS_OK, nothing fused, no chunk created"""
    dst_chunks = {(0, 0, 0): S.draw(101, False)}
    dst = S.make_store(dst_chunks)
    rc, stats = raw_fuse(dst, S.make_store({}), F.identity_pose())
    assert rc == WS_OK and np.all(stats == 0)
    value, weight = F.unpack(S.draw(102, False))
    unobserved = {(0, 0, 0): F.pack(value, -np.abs(weight)), (1, 0, 0): F.pack(value, 0 * weight)}
    rc, stats = raw_fuse(dst, S.make_store(unobserved), F.identity_pose())
    assert rc == WS_OK and stats[0] > 0 and np.all(stats[1:] == 0)
    assert dst.keys() == [(0, 0, 0)] and F.same((S.read(dst), ()), (dst_chunks, ()))


def test_two_runs_give_equal_bytes():
    """11."""
    g = general_case()
    runs = []
    for _ in range(2):
        dst, src = S.make_store(g["dst"]), S.make_store(g["src"])
        st = dst.fuse(src, g["pose"], MW, resolution=RES)
        runs.append((S.read(dst), st.as_tuple()))
    assert F.same(runs[0], (runs[1][0], runs[1][1]))


def test_ordering_with_saves_and_queries():
    """12. a save_box into SRC enqueued just before the fuse is seen by it; ws_store_mesh on DST after it sees the fused voxels; DST's
    earlier surface result is still valid and unchanged"""
    import raycast_model as R
    size = (17, 17, 17)
    rng = np.random.default_rng(12)
    # the window [-8, 8]^3 around the origin; with offset = size / 2 storage order is world order
    box = F.pack(rng.integers(-TAU, TAU, size), rng.integers(1, 50, size))
    t, _ = R.upload(size, (0, 0, 0), tuple(s // 2 for s in size), [box, box], tau=TAU, mw=MW, res=RES)
    dst_chunks = {(0, 0, 0): S.draw(121, False)}
    dst, src = S.make_store(dst_chunks), S.make_store({})
    before = dst.surface(TAU, RES, device=True)
    kept = before.clone()
    src.save_box(t, (-8, -8, -8), (8, 8, 8))  # stream-ordered, no wait
    st = dst.fuse(src, F.identity_pose(), MW, resolution=RES)
    src_chunks = {}
    for key in [(i, j, k) for i in (-1, 0) for j in (-1, 0) for k in (-1, 0)]:
        c = np.full((64, 64, 64), FILL, dtype=np.uint32)
        sl = tuple(slice(56, 64) if k < 0 else slice(0, 9) for k in key)
        c[sl] = box[tuple(slice(0, 8) if k < 0 else slice(8, 17) for k in key)]
        src_chunks[key] = c.reshape(-1)
    want = F.fuse(dst_chunks, src_chunks, F.identity_pose(), RES, MW, FILL)
    assert F.same((S.read(dst), st.as_tuple()), want) and st.created == 7 and st.averaged + st.set == 17 ** 3
    import store_scenes as SM
    vert, face = dst.mesh(RES)
    mv, mf = SM.model_store(want[0], RES)
    assert vert.tobytes() == mv.tobytes() and face.tobytes() == mf.tobytes() and len(vert) > 0
    assert bool((before == kept).all()) and len(kept) > 0


def test_merge_map_and_align_map():
    """13. the synthetic room built twice on a small window, two scans each, the second map in a frame offset by a known small
    pose: align_map from the identity gives a pose under which a count-only fuse disagrees less than under the identity (two
    measured values, no tolerance); merge_map at that pose reports the count-only statistics, leaves the window holding the merged
    voxels, and takes a host GlobalMap as well"""
    import warpsense_amd as W
    import store_scenes as SM
    from window_routes import _params
    from warpsense_amd import synthetic as SY
    size, res = (65, 65, 65), SM.RES
    truth = S.rot(1.0, 0, 0, (45, -30, 20))  # frame B -> frame A
    inv = np.linalg.inv(truth)
    maps = []
    for frame in (np.eye(4), inv):
        store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
        tm = W.TSDFRegistration(_params(size), W.LocalMap(*size, SM.TAU, 0), device_global_map=store)
        for k, sensor in enumerate([(0.0, 0.0, 0.0), (300.0, -200.0, 100.0)]):
            pts = SY.os1_128_scan(sensor_mm=sensor, rings=32, azimuths=256, half_extents_mm=(1700.0, 1300.0, 900.0), seed=30 + k)
            pts = np.rint(pts @ frame[:3, :3].T + frame[:3, 3]).astype(np.int32)
            pos = np.floor((frame[:3, :3] @ np.asarray(sensor) + frame[:3, 3]) / res).astype(np.int32)
            tm.update_tsdf(pts, pos_rm=pos, up_rm=(0, 0, 32768))
        tm.global_surface_cloud()  # the window goes into the store
        maps.append((tm, store))
    (ta, a), (tb, b) = maps
    T = ta.align_map(b, np.eye(4), max_points=20000)
    at_identity = a.fuse(b, np.eye(4), MW, count_only=True, resolution=res)
    at_aligned = a.fuse(b, T, MW, count_only=True, resolution=res)
    print("disagreement_mm: identity", at_identity.disagreement_mm, "aligned", at_aligned.disagreement_mm, "points", ta.last_align_points, "T", T[:3, 3])
    assert at_identity.averaged > 1000 and at_aligned.averaged > 1000
    assert at_aligned.disagreement_mm < at_identity.disagreement_mm
    # merge_map: the statistics of the count-only call with the map's max_weight, then the window holds what the store holds
    mw = ta.params_.map.max_weight
    want = a.fuse(b, T, mw, count_only=True, resolution=res)
    assert ta.merge_map(b, T, count_only=True).as_tuple() == want.as_tuple()
    host = W.GlobalMap(SM.TAU, 0)
    b.flush_to(host)
    before = S.read(a)
    st = ta.merge_map(host, T)
    assert st.as_tuple() == want.as_tuple() and st.averaged > 1000
    after = S.read(a)
    assert any(not np.array_equal(after[k], before[k]) for k in before)
    lo, hi = ta.local_map_.window()
    window = np.asarray(ta.tsdf().avg_map().extract_box(lo, hi)).reshape(-1)
    probe = W.GlobalMap(SM.TAU, 0)
    for k, v in after.items():
        probe.activate_chunk(*k)[:] = v
    assert np.array_equal(window, probe.load_box(lo, hi))
    for _, store in maps:
        store.close()
