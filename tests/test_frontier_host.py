"""The frontier query without a GPU: the numpy model (frontier_model.py) against cases small enough to check by eye, the host helper
frontier_goals, and the boundary -- the header declares the twelve entry points, and warpsense_amd._lib lists and types them."""
import ctypes as C
import re

import numpy as np

import frontier_model as FM
import query_model as QM

TAU = 1000
NEW_MAP = ["ws_map_frontier", "ws_map_frontier_records_dev", "ws_map_frontier_labels_dev", "ws_map_frontier_clusters_dev", "ws_map_frontier_download",
           "ws_debug_frontier_timing"]
NEW_STORE = ["ws_store_frontier", "ws_store_frontier_records_dev", "ws_store_frontier_labels_dev", "ws_store_frontier_clusters_dev",
             "ws_store_frontier_download", "ws_debug_store_frontier_timing"]
FLAGS = {"WS_FRONTIER_DEFAULT": 0, "WS_FRONTIER_ANY_WEIGHT": 1, "WS_FRONTIER_CLUSTERS": 2}
CTYPE = dict(QM.CTYPE, **{"ws_store *": C.c_void_p, "const ws_store *": C.c_void_p, "float [4]": C.c_void_p})


# ------------------------------------------------------------------------------------------------ the boundary
def test_header_declares_and_lib_lists_and_types_the_twelve_entry_points():
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
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"u\b", h), name
        assert getattr(_lib, name) == value and getattr(W, name) == value
    assert W.FRONTIER_RECORD == FM.RECORD and W.FRONTIER_CLUSTER == FM.CLUSTER
    assert W.FRONTIER_CLUSTER.itemsize == 64 and W.FRONTIER_CLUSTER.fields["sum"][1] == 32


# ------------------------------------------------------------------------------------------------ by hand
def _block():
    """a 3^3 free block (value tau, weight 1) in the middle of a 5^3 box of never-observed voxels, first world voxel (10, 20, 30)"""
    value, weight = np.zeros((5, 5, 5), np.int32), np.zeros((5, 5, 5), np.int32)
    value[1:4, 1:4, 1:4], weight[1:4, 1:4, 1:4] = TAU, 1
    return FM.pack(value, weight), (10, 20, 30)


def test_a_free_block_in_unknown():
    raw, lo = _block()
    rec, labels, table = FM.frontier(raw, lo)
    # every voxel of the block but its centre touches the unknown shell: 26 records, in (x, y, z) order, one cluster
    assert len(rec) == 26 and (rec["x"][0], rec["y"][0], rec["z"][0], rec["mask"][0]) == (11, 21, 31, 0b010101)
    assert (rec["x"][-1], rec["y"][-1], rec["z"][-1], rec["mask"][-1]) == (13, 23, 33, 0b101010)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    assert not np.any(np.all(xyz == (12, 22, 32), axis=1))  # the centre is free and knows all its neighbours
    face_centre = rec[np.all(xyz == (12, 22, 31), axis=1)]
    assert len(face_centre) == 1 and face_centre["mask"][0] == 0b010000  # only -z
    order = np.lexsort((rec["z"], rec["y"], rec["x"]))
    assert np.array_equal(order, np.arange(26))
    assert np.all(labels == 0) and len(table) == 1
    row = table[0]
    assert (row["first"], row["count"], row["pad"]) == (0, 26, 0)
    assert tuple(row["lo"]) == (11, 21, 31) and tuple(row["hi"]) == (13, 23, 33)
    assert tuple(row["sum"]) == (26 * 12, 26 * 22, 26 * 32)  # the missing centre is the centroid
    centroid, size, blo, bhi = FM.goals(table, resolution=50)
    assert np.allclose(centroid, [[0.6, 1.1, 1.6]]) and list(size) == [26]


def test_a_neighbour_outside_the_box_is_ignored():
    raw, lo = _block()
    # the box cut to the block itself: no unknown voxel is left in it, the rim is no frontier
    inner = raw[1:4, 1:4, 1:4]
    assert len(FM.records(inner, (11, 21, 31))) == 0
    # the box cut along x only: the faces at x = 11 and x = 13 are the rim, the other four faces still touch unknown
    rec = FM.records(raw[1:4], (11, 20, 30))
    assert len(rec) == 24 and not np.any(rec["mask"] & 0b000011)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    for x in (11, 12, 13):  # the centre column of every x plane knows all its neighbours in the box
        assert not np.any(np.all(xyz == (x, 22, 32), axis=1))
    # ... so the result of a box is not the restriction of the larger box's result
    whole = FM.records(raw, lo)
    assert len(whole[(whole["x"] >= 11) & (whole["x"] <= 13)]) == 26


def test_min_value_edges():
    value = np.array([[[0, 1, TAU - 1, TAU, 32767, -1, -32768, 0]]], dtype=np.int32)
    weight = np.array([[[1, 1, 1, 1, 1, 1, 1, 0]]], dtype=np.int32)
    weight2 = np.concatenate([weight, np.zeros_like(weight)], axis=1)  # every voxel has an unknown neighbour at +y
    value2 = np.concatenate([value, np.zeros_like(value)], axis=1)
    raw = FM.pack(value2, weight2)
    z = lambda mv: list(FM.records(raw, (0, 0, 0), min_value=mv)["z"])
    assert z(0) == [0, 1, 2, 3, 4]          # any non-negative value; -1, -32768 and the unknown voxel are not free
    assert z(1) == [1, 2, 3, 4]
    assert z(TAU) == [3, 4]
    assert z(TAU + 1) == [4] and z(32767) == [4]
    rec = FM.records(raw, (0, 0, 0))
    assert list(rec["mask"]) == [0b001000] * 4 + [0b001000]  # z = 6 is known (occupied), z = 7 unknown: not a neighbour of z = 4
    # z = 6 (value -32768, weight 1) is occupied and known; its neighbour z = 7 is unknown but z = 6 is not free
    assert 6 not in z(0)


def test_negative_weights_and_any_weight():
    value = np.full((1, 1, 4), TAU, np.int32)
    weight = np.array([[[1, -1, 1, 0]]], dtype=np.int32)
    raw = FM.pack(value, weight)
    # default: weight -1 is UNKNOWN, so z = 0 and z = 2 touch it (and z = 2 touches z = 3)
    rec = FM.records(raw, (0, 0, 0))
    assert list(rec["z"]) == [0, 2] and list(rec["mask"]) == [0b100000, 0b110000]
    # any_weight: weight -1 is VALID and free; only z = 2 touches the unknown z = 3
    rec = FM.records(raw, (0, 0, 0), any_weight=True)
    assert list(rec["z"]) == [2] and list(rec["mask"]) == [0b100000]
    raw = FM.pack(value, np.array([[[1, 1, -1, 0]]]))
    assert list(FM.records(raw, (0, 0, 0), any_weight=True)["z"]) == [2] and list(FM.records(raw, (0, 0, 0))["z"]) == [1]


def test_absent_chunk_voxels_are_unknown_whatever_they_hold():
    value, weight = np.full((1, 1, 3), TAU, np.int32), np.ones((1, 1, 3), np.int32)
    raw = FM.pack(value, weight)
    assert len(FM.records(raw, (0, 0, 0))) == 0
    present = np.array([[[True, True, False]]])
    rec = FM.records(raw, (0, 0, 0), present=present)
    assert list(rec["z"]) == [1] and list(rec["mask"]) == [0b100000]


def test_components_numbering_and_table():
    # two free voxels that touch only at a corner, a third one two voxels away; all in unknown
    value, weight = np.zeros((6, 6, 6), np.int32), np.zeros((6, 6, 6), np.int32)
    for p in [(1, 1, 1), (2, 2, 2), (4, 2, 2)]:
        value[p], weight[p] = TAU, 1
    rec, labels, table = FM.frontier(FM.pack(value, weight), (-3, -3, -3))
    assert len(rec) == 3 and list(labels) == [0, 0, 1] and len(table) == 2
    assert (table["first"][0], table["count"][0], tuple(table["lo"][0]), tuple(table["hi"][0]), tuple(table["sum"][0])) == (0, 2, (-2, -2, -2), (-1, -1, -1), (-3, -3, -3))
    assert (table["first"][1], table["count"][1], tuple(table["sum"][1])) == (2, 1, (1, -1, -1))
    # one voxel further apart: three clusters, numbered by their first records
    value[:], weight[:] = 0, 0
    for p in [(1, 1, 1), (3, 2, 2), (5, 2, 2)]:
        value[p], weight[p] = TAU, 1
    rec, labels, table = FM.frontier(FM.pack(value, weight), (0, 0, 0))
    assert list(labels) == [0, 1, 2] and list(table["first"]) == [0, 1, 2]
    # the first member of a cluster, not its position, numbers it: a cluster that starts later in record order gets the larger number
    value[:], weight[:] = 0, 0
    for p in [(0, 5, 0), (1, 0, 0), (1, 4, 0)]:  # records 0 and 2 are neighbours, record 1 is alone
        value[p], weight[p] = TAU, 1
    rec, labels, table = FM.frontier(FM.pack(value, weight), (0, 0, 0))
    assert list(labels) == [0, 1, 0] and list(table["first"]) == [0, 1] and list(table["count"]) == [2, 1]


def test_frontier_goals_orders_largest_first_ties_by_first():
    import warpsense_amd as W
    table = np.zeros(4, dtype=W.FRONTIER_CLUSTER)
    table["first"], table["count"] = [0, 5, 9, 20], [3, 7, 3, 1]
    table["sum"] = [[3, 6, 9], [70, 0, -7], [0, 0, 3], [5, 5, 5]]
    table["lo"], table["hi"] = -1, 9
    centroid, size, lo, hi = W.frontier_goals(table, resolution=50)
    assert list(size) == [7, 3, 3, 1] and np.allclose(centroid, [[0.5, 0, -0.05], [0.05, 0.1, 0.15], [0, 0, 0.05], [0.25, 0.25, 0.25]])
    want = FM.goals(table, 50)
    assert all(np.array_equal(a, b) for a, b in zip((centroid, size, lo, hi), want))
    centroid, size, lo, hi = W.frontier_goals(table, resolution=50, min_size=3)
    assert list(size) == [7, 3, 3] and lo.shape == (3, 3) and hi.shape == (3, 3)
    assert W.frontier_goals(table[:0], 50)[0].shape == (0, 3)


def test_write_frontier_ply(tmp_path):
    import warpsense_amd as W
    raw, lo = _block()
    rec, labels, table = FM.frontier(raw, lo)
    path = tmp_path / "f.ply"
    assert W.write_frontier_ply(str(path), rec, 50, labels) == 26
    blob = path.read_bytes()
    head, body = blob.split(b"end_header\n", 1)
    assert b"element vertex 26" in head and b"property int cluster" in head and len(body) == 26 * 17
    assert W.write_frontier_ply(str(path), rec, 50) == 26 and len(path.read_bytes().split(b"end_header\n", 1)[1]) == 26 * 13
