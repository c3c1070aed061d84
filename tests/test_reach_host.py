"""The reach query without a GPU: the model (reach_model.py) against cases small enough to write out by hand, against a plain
repeat-until-stable relaxation as a second witness for the minimum, and the boundary -- the header declares the entry points, and
warpsense_amd._lib lists and types each of them."""
import ctypes as C
import re

import numpy as np

import distance_model as DM
import query_model as QM
import reach_model as RM
from frontier_scenes import random_box

INF = RM.INF
NEW_MAP = ["ws_map_reach", "ws_map_reach_dev", "ws_map_reach_download", "ws_map_reach_box", "ws_map_reach_lookup", "ws_map_reach_lookup_dev", "ws_map_reach_paths",
           "ws_debug_reach_timing", "ws_debug_reach_params", "ws_debug_reach_active"]
NEW_STORE = ["ws_store_reach", "ws_store_reach_dev", "ws_store_reach_download", "ws_store_reach_box", "ws_store_reach_lookup", "ws_store_reach_lookup_dev", "ws_store_reach_paths",
             "ws_debug_store_reach_timing"]
FLAGS = {"WS_REACH_DEFAULT": "0u", "WS_REACH_UNKNOWN_FREE": "1u", "WS_REACH_UNREACHABLE": "0xFFFFFFFFu"}
CTYPE = dict(QM.CTYPE, **{"ws_store *": C.c_void_p, "const ws_store *": C.c_void_p, "const int32_t *": C.c_void_p, "int32_t [8]": C.c_void_p, "int32_t [3]": C.c_void_p,
                           "uint32_t [3]": C.c_void_p, "int32_t *": C.c_void_p})


# ------------------------------------------------------------------------------------------------ the boundary
def test_header_declares_and_lib_lists_and_types_the_entry_points():
    from warpsense_amd import _lib
    import warpsense_amd as W
    L = _lib.load()
    h = QM._header()
    for name in NEW_MAP + NEW_STORE:
        assert re.search(r"\b" + name + r"\s*\(", h), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
        ret, params = QM._declared(name)
        fn = getattr(L, name)
        assert list(fn.argtypes) == [CTYPE[p] for p in params], (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name
        else:
            assert ret == "int" and fn.restype is C.c_int, name
    for name, value in FLAGS.items():
        assert re.search(r"#define\s+" + name + r"\s+" + value + r"\b", h), name
        assert getattr(_lib, name) == int(value.rstrip("u"), 0) and getattr(W, name) == int(value.rstrip("u"), 0)
    assert W.REACH_PATH_HEADER == RM.HEADER and W.REACH_PATH_RECORD == RM.RECORD
    assert W.REACH_PATH_HEADER.itemsize == 16 and W.REACH_PATH_RECORD.itemsize == 16
    assert L.ws_version() == 1
    p = (C.c_int32 * 8)()
    assert L.ws_debug_reach_params(p) == 0 and p[0] >= 1 and p[1] * p[2] * p[3] == p[4] * p[5] and p[7] == 0


def test_reach_mm_and_write_path_ply(tmp_path):
    import warpsense_amd as W
    assert list(W.reach_mm(np.array([0, 10, 14, INF], np.uint32), 50)) == [0.0, 50.0, 70.0, np.inf]
    hdr = np.array([(24, 2, 3, 0), (INF, 0, 0, 1)], dtype=RM.HEADER)
    rec = np.zeros((2, 4), dtype=RM.RECORD)
    rec[0, :3] = [(2, 1, 0, 24), (1, 0, 0, 10), (0, 0, 0, 0)]
    path = tmp_path / "p.ply"
    assert W.write_path_ply(str(path), hdr, rec, 50) == (3, 2)
    head, body = path.read_bytes().split(b"end_header\n", 1)
    assert b"element vertex 3" in head and b"element edge 2" in head and len(body) == 3 * 20 + 2 * 8


# ------------------------------------------------------------------------------------------------ by hand
def _plate():
    """a 5 x 5 x 1 plate, first voxel (10, 20, 30): a wall along x = 2 with a gap at y = 3"""
    free = np.ones((5, 5, 1), dtype=bool)
    free[2, :, 0] = False
    free[2, 3, 0] = True
    return RM.records_from(free), (10, 20, 30)


def test_a_plate_with_a_wall_and_a_gap():
    rec, lo = _plate()
    cost, kept, reached = RM.field(rec, lo, [(10, 20, 30)])
    want = np.array([[0, 10, 20, 30, 40],
                     [10, 14, 24, 34, 44],
                     [INF, INF, INF, 38, INF],
                     [72, 62, 52, 48, 52],  # through the gap: 38 + 10 straight on, 38 + 14 to either side
                     [76, 66, 62, 58, 62]], dtype=np.uint32)
    assert np.array_equal(cost[:, :, 0], want) and (kept, reached) == (1, 21)
    # the same plate as a column map: 8-neighbourhood, z of the seed ignored
    cost2, kept2, reached2 = RM.field(rec[:, :, 0], lo, [(10, 20, -999)])
    assert np.array_equal(cost2, want) and (kept2, reached2) == (1, 21)
    # clearance 2 closes the gap's neighbourhood: d2 of every free voxel here is 1
    assert RM.field(rec, lo, [(10, 20, 30)], clear_d2=2)[1:] == (0, 0)


def test_a_diagonal_shortcut_14_against_20():
    free = np.ones((2, 2, 1), dtype=bool)
    rec = RM.records_from(free)
    cost, _, _ = RM.field(rec, (0, 0, 0), [(0, 0, 0)])
    assert cost[1, 1, 0] == 14 and cost[1, 0, 0] == cost[0, 1, 0] == 10
    free[1, 0, 0] = free[0, 1, 0] = False  # the diagonal passes between two sites unless the clearance forbids it
    assert RM.field(RM.records_from(free), (0, 0, 0), [(0, 0, 0)])[0][1, 1, 0] == 14
    cube = RM.records_from(np.ones((2, 2, 2), dtype=bool))
    assert RM.field(cube, (0, 0, 0), [(0, 0, 0)])[0][1, 1, 1] == 17


def test_a_pocket_is_unreachable_and_seeds_are_dropped_and_counted():
    free = np.ones((7, 7, 1), dtype=bool)
    free[2:5, 2:5, 0] = False
    free[3, 3, 0] = True  # a free voxel sealed by a ring of sites
    rec = RM.records_from(free)
    cost, kept, reached = RM.field(rec, (0, 0, 0), [(0, 0, 0), (2, 2, 0), (9, 9, 9), (0, 0, 0)])
    assert kept == 2 and cost[3, 3, 0] == INF and reached == 49 - 9  # the obstacle seed and the outside seed are dropped; a voxel given twice counts twice
    assert list(RM.lookup(cost, (0, 0, 0), [(3, 3, 0), (6, 6, 0), (7, 0, 0), (0, 0, 1)])) == [INF, 3 * 14 + 6 * 10, INF, INF]  # around the block: three diagonal and six straight steps
    none, kept, reached = RM.field(rec, (0, 0, 0), [(2, 2, 0)])
    assert (kept, reached) == (0, 0) and np.all(none == INF)
    # unknown records: blocked by default, passable under unknown_free
    cls = np.where(free, 1, 0).astype(np.uint32)
    rec = RM.records_from(free, d2=np.full(free.shape, 9), cls=cls)
    assert RM.field(rec, (0, 0, 0), [(0, 0, 0)])[0][3, 3, 0] == INF
    assert RM.field(rec, (0, 0, 0), [(0, 0, 0)], unknown_free=True)[0][3, 3, 0] == 3 * 14


def test_a_tie_where_the_offset_order_decides_the_path():
    rec = RM.records_from(np.ones((3, 3, 1), dtype=bool))
    cost, _, _ = RM.field(rec, (0, 0, 0), [(0, 0, 0)])
    assert cost[2, 1, 0] == 24  # by (1, 0) then (1, 1), or by (1, 1) then (1, 0)
    hdr, steps = RM.paths(cost, (0, 0, 0), [(2, 1, 0), (0, 0, 0), (5, 5, 5)], 4)
    # the predecessors of (2, 1) in ascending (dx, dy, dz): (-1, -1) -> (1, 0) cost 10 + 14 comes before (-1, 0) -> (1, 1) cost 14 + 10
    assert [tuple(int(v) for v in s) for s in steps[0][:3]] == [(2, 1, 0, 24), (1, 0, 0, 10), (0, 0, 0, 0)]
    assert tuple(hdr[0]) == (24, 2, 3, 0) and tuple(hdr[1]) == (0, 0, 1, 0) and tuple(hdr[2]) == (INF, 0, 0, 2)
    assert RM.legal_path(steps[0], 3, cost)
    hdr, steps = RM.paths(cost, (0, 0, 0), [(2, 1, 0)], 2)  # a cap below the path: the prefix, the true number of steps
    assert tuple(hdr[0]) == (24, 2, 2, 0) and tuple(steps[0][1]) == (1, 0, 0, 10)
    hdr, steps = RM.paths(cost, (0, 0, 0), [(2, 1, 0)], 0)
    assert tuple(hdr[0]) == (24, 2, 0, 0) and steps.shape == (1, 0)


# ------------------------------------------------------------------------------------------------ the second witness
def test_dijkstra_against_plain_relaxation_on_a_random_box():
    raw = random_box((9, 8, 10), seed=5)
    for columns in (False, True):
        rec, _ = DM.model_box(raw, 3, columns=columns)
        for clear_d2, unknown_free in [(0, False), (1, True), (2, True)]:
            trav = RM.traversable(rec, clear_d2, unknown_free)
            seeds = np.argwhere(RM._volume(trav))[::37][:3] + np.array([4, -2, 7])
            cost, kept, reached = RM.field(rec, (4, -2, 7), seeds, clear_d2, unknown_free)
            assert kept == len(seeds) and reached >= kept
            assert np.array_equal(cost, RM.relax(rec, (4, -2, 7), seeds, clear_d2, unknown_free)), (columns, clear_d2, unknown_free)
            assert np.all((cost != INF) <= trav)
