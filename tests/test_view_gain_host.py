"""The view gain on the host: the numpy model of view_gain_model.py on scenes checkable by hand, the conditions of every scene the GPU
tests use (asserted on the model's output), the host helpers, and the declarations of the new entry points."""
import ctypes as C

import numpy as np
import pytest

import query_model as QM
import store_raycast_scenes as SR
import store_scenes as SM
import view_gain_model as VM
import view_gain_scenes as VS
from view_gain_scenes import RES, filled

NEW = [f"ws_{o}view_gain{s}" for o in ("map_", "store_") for s in ("", "_records_dev", "_rays_dev", "_download")] + ["ws_debug_view_gain_timing", "ws_debug_store_view_gain_timing"]
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.int64) * 1000
CENTRE = np.array([[375, 375, 375]])  # the centre of voxel (7, 7, 7) of a 15^3 box at lo = 0, RES 50
sq = lambda a, b: sum(k * k for k in range(a, b + 1))


def test_free_box_from_its_centre_matches_the_closed_form():
    rec, rays = VM.model(filled((15, 15, 15), 500, 64), (0, 0, 0), RES, CENTRE, AXES, 1000)
    # +axis: floor((375 + 25 k) / 50) <= 14 iff k <= 14; -axis: 375 - 25 k >= 0 iff k <= 15
    assert rec["free"][0] == 3 * 15 + 3 * 16 and rec["free_k2"][0] == 3 * sq(0, 14) + 3 * sq(0, 15) == 6765
    assert rec["unknown"][0] == rec["unknown_k2"][0] == rec["blocked"][0] == 0 and rec["live"][0] == 6
    assert np.all(rays["stop"] == -1) and np.all(rays["unknown"] == 0)


def test_a_plane_stops_the_ray_at_the_hand_computed_sample():
    box = filled((15, 15, 15), 500, 64)
    box[11] = filled((15, 15), -200, 64)
    rec, rays = VM.model(box, (0, 0, 0), RES, CENTRE, AXES, 1000)
    # floor((375 + 25 k) / 50) == 11 first at 375 + 25 k >= 550: k = 7
    assert rays["stop"][0].tolist() == [7, -1, -1, -1, -1, -1] and rec["blocked"][0] == 1
    assert rec["free"][0] == 7 + 16 + 2 * 15 + 2 * 16 and rec["free_k2"][0] == sq(0, 6) + 3 * sq(0, 15) + 2 * sq(0, 14)
    # min_value above the free value: the origin's own voxel blocks every ray
    rec, rays = VM.model(box, (0, 0, 0), RES, CENTRE, AXES, 1000, min_value=501)
    assert np.all(rays["stop"] == 0) and rec["blocked"][0] == 6 and rec["free"][0] == rec["unknown"][0] == 0


def test_an_unobserved_slab_behind_free_space():
    box = filled((15, 15, 15), 500, 64)
    box[10:13] = filled((3, 15, 15), 123, 0)
    rec, rays = VM.model(box, (0, 0, 0), RES, CENTRE, AXES[:1], 1000)
    # voxel 10 .. 12 iff 500 <= 375 + 25 k < 650: k = 5 .. 10; unknown does not block: free again for k = 11 .. 14
    assert rec["unknown"][0] == 6 and rec["unknown_k2"][0] == sq(5, 10) == 355 and rays["unknown"][0, 0] == 6
    assert rec["free"][0] == 5 + 4 and rec["free_k2"][0] == sq(0, 4) + sq(11, 14) and rays["stop"][0, 0] == -1
    # a negative weight is UNKNOWN by default and observed under ANY_WEIGHT
    box[10:13] = filled((3, 15, 15), -5, -3)
    assert VM.model(box, (0, 0, 0), RES, CENTRE, AXES[:1], 1000)[0]["unknown"][0] == 6
    assert VM.model(box, (0, 0, 0), RES, CENTRE, AXES[:1], 1000, any_weight=True)[1]["stop"][0, 0] == 5


def test_an_origin_outside_the_box():
    w = VM.march(filled((15, 15, 15), 500, 64), (0, 0, 0), RES, [[-300, 375, 375]], AXES[:2], 1000)
    # +x enters at -300 + 25 k >= 0: k = 12, leaves at 25 k - 300 >= 750: k = 42 > K = 40; -x never enters
    assert w["outside"][0].tolist() == [12, 41] and w["free"][0].tolist() == [29, 0] and w["free_k2"][0, 0] == sq(12, 40)
    assert w["stop"][0].tolist() == [-1, -1]


def test_dead_rays_k_zero_and_an_occupied_origin():
    box = filled((15, 15, 15), 500, 64)
    dirs = np.array([[0, 0, 0], [2 ** 30, 1, 1], [-2 ** 31, 0, 0], [2 ** 30 - 1, 0, 0]], dtype=np.int64)
    rec, rays = VM.model(box, (0, 0, 0), RES, CENTRE, dirs, 1000)
    assert rays["stop"][0].tolist() == [-2, -2, -2, -1] and rec["live"][0] == 1 and rec["free"][0] == 15
    rec, rays = VM.model(box, (0, 0, 0), RES, CENTRE, AXES, 24)  # max_range < step: K = 0
    assert rec["free"][0] == 6 and rec["free_k2"][0] == 0
    box[7, 7, 7] = filled((), -1, 64)
    rec, rays = VM.model(box, (0, 0, 0), RES, CENTRE, AXES, 1000)
    assert np.all(rays["stop"] == 0) and rec["blocked"][0] == 6 and rec["free"][0] == 0 and rec["unknown"][0] == 0
    u, b, l = VM.from_rays(rays)
    assert (u[0], b[0], l[0]) == (rec["unknown"][0], rec["blocked"][0], rec["live"][0])


@pytest.mark.parametrize("size", VS.SIZES, ids=lambda s: "x".join(map(str, s)))
def test_the_random_window_scenes_meet_their_conditions(size):
    lo, _ = QM.window(size, VS.POS)
    o, d = VS.views(size), VS.fan()
    wlo, whi = lo * RES, (lo + np.asarray(size)) * RES
    assert np.any(np.any((o < wlo) | (o >= whi), axis=1)) and np.all(np.all((o >= wlo) & (o < whi), axis=1)[:1])
    for which, box in enumerate(VS.window_boxes(size)):
        for min_value in VS.MIN_VALUES:
            for any_weight in (False, True):
                w = VM.march(box, lo, RES, o, d, 3000, min_value, any_weight)
                for n in (63, 64, 65, 1034):
                    print(size, which, min_value, any_weight, n, VS.check_scene(w, n))
                rec, rays = VM.records(w)
                u, b, l = VM.from_rays(rays)
                assert np.array_equal(u, rec["unknown"]) and np.array_equal(b, rec["blocked"]) and np.array_equal(l, rec["live"])
                assert np.all(rec["live"] == 1034 - len(VS.DEAD_DIRS))


def test_the_chunk_scenes_meet_their_conditions():
    for name, chunks, lo, hi, o, d, rng in VS.store_scenes():
        w = VM.march(SM.assemble(chunks, lo, hi), lo, RES, o, d, rng)
        got = VS.check_scene(w, len(d), outside_origins=False) if len(d) >= 63 else None
        absent = VS.absent_ray_count(w, chunks, lo, hi, RES, o, d, rng)
        print(name, got, absent)
        assert absent >= 1, name


@pytest.mark.parametrize("res", [2, 51, 64])
def test_the_edge_scenes_meet_their_conditions(res):
    for sign in (1, -1):
        pos, box, lo, o, d, rng = VS.edge_scene(res, sign)
        assert abs(int(o[0, 0])) + rng + 2 * res == 2 ** 31 - 1
        print(res, sign, VS.check_scene(VM.march(box, lo, res, o, d, rng), len(d), outside_origins=False))


@pytest.mark.parametrize("where", ["+", "-"])
def test_the_one_millimetre_store_scene_at_the_edge_of_int32(where):
    chunks, lo, hi, o, d, rng = VS.store_edge_scene(where)
    w = VM.march(SM.assemble(chunks, lo, hi), lo, 1, o, d, rng)
    print(where, rng, VS.check_scene(w, len(d), outside_origins=False), VS.absent_ray_count(w, chunks, lo, hi, 1, o, d, rng))
    assert VS.absent_ray_count(w, chunks, lo, hi, 1, o, d, rng) >= 10


def test_the_big_sum_scene_exceeds_32_bits():
    chunks, lo, hi, o, d, rng = VS.big_sum_scene()
    w = VM.march(SM.assemble(chunks, lo, hi), lo, RES, o, d, rng)
    rec = VM.records(w)[0]
    assert int(w["unknown_k2"].max()) >= 2 ** 32 and int(rec["unknown_k2"][0]) >= 2 ** 40 and int(rec["free_k2"][0]) > 0
    assert int(rec["unknown"][0]) > 2 ** 20 and len(set(w["unknown"][0].tolist())) > 50


def test_on_the_oracles_map_the_next_best_view_sees_more_than_staying_put():
    """the scan of the synthetic room from pose A through the oracle's update: next_best_view, restated on the models, has at least
    two candidates, and its winner's unknown_k2 exceeds that of pose A with the same fan -- what test_gpu_view_gain.py then asserts
    on the device's map of the same scan"""
    box, lo = VS.oracle_room()
    a, cand, goals, records, order = VS.next_view_model(box, lo)
    print("A", int(a["unknown_k2"][0]), "candidates", len(cand), "gains", records["unknown_k2"][order].tolist())
    assert len(cand) >= 2 and a["live"][0] == len(VS.room_fan()) and a["free"][0] >= 100
    assert int(records["unknown_k2"][order[0]]) > int(a["unknown_k2"][0])


def test_view_fan_is_integer_scaled_and_never_zero():
    import warpsense_amd as W
    for rings, az, fov in [(1, 1, 0.0), (1, 64, 30.0), (16, 64, 45.0), (5, 7, 170.0)]:
        d = W.view_fan(rings, az, fov)
        assert d.dtype == np.int32 and d.shape == (rings * az, 3)
        assert np.all(np.max(np.abs(d.astype(np.int64)), axis=1) == 2 ** 20) and not np.any(np.all(d == 0, axis=1))
    assert W.view_fan(1, 4, 0.0).tolist() == [[2 ** 20, 0, 0], [0, 2 ** 20, 0], [-2 ** 20, 0, 0], [0, -2 ** 20, 0]]
    with pytest.raises(W.WsError):
        W.view_fan(0, 4, 10.0)


def test_rank_views_and_gain_volume():
    import warpsense_amd as W
    rec = np.zeros(5, dtype=W.VIEW_GAIN_RECORD)
    rec["unknown_k2"] = [100, 400, 400, 9000, 0]
    cost = np.array([0, 10, 10, 0xFFFFFFFF, 0], dtype=np.uint32)
    order, score = W.rank_views(rec, cost, 50, 0.0)
    assert order.tolist() == [1, 2, 0, 4, 3] and score[3] == -np.inf and score[1] == 400.0  # ties to the lower index, unreachable last
    order, score = W.rank_views(rec, np.array([0, 200000, 10, 0, 0], dtype=np.uint32), 50, 1.0)  # 200000 * 50 / 10 mm = 1 km
    assert order.tolist()[:2] == [3, 2] and np.isclose(score[2], 400.0 * np.exp(-0.05))
    with pytest.raises(W.WsError):
        W.rank_views(rec, cost[:3], 50, 0.0)
    vol = W.gain_volume_m3(rec, 50, 0.01)
    assert np.allclose(vol, rec["unknown_k2"] * 0.025 ** 3 * 0.01) and vol.dtype == np.float64
    assert W.gain_volume_m3(rec, 1, 1.0)[0] == 100 * 1e-9  # step = max(res / 2, 1)


def test_dtypes_and_declarations():
    import warpsense_amd as W
    from warpsense_amd import _lib
    assert W.VIEW_GAIN_RECORD.itemsize == 32 and W.VIEW_GAIN_RAY.itemsize == 8
    assert W.VIEW_GAIN_RECORD == VM.RECORD and W.VIEW_GAIN_RAY == VM.RAY
    assert (W.WS_GAIN_DEFAULT, W.WS_GAIN_ANY_WEIGHT, W.WS_GAIN_RAYS) == (0, 1, 2)
    L = _lib.load()
    ctype = dict(SR.CTYPE, **{"uint64_t *": C.c_void_p})
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        ret, params = QM._declared(name)
        fn = getattr(L, name)
        assert list(fn.argtypes) == [ctype[p] for p in params], (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name
        else:
            assert ret == "int" and fn.restype is C.c_int, name
    assert len(QM._declared("ws_map_view_gain")[1]) == 12 and len(QM._declared("ws_store_view_gain")[1]) == 12
    for m in ("view_gain", "view_gain_timing"):
        assert hasattr(W.DeviceMapMemWrapper, m) and hasattr(W.DeviceGlobalMap, m)
    for m in ("view_gain", "global_view_gain", "next_best_view"):
        assert hasattr(W.TSDFMapping, m)
