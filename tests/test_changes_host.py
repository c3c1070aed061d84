"""CPU tests of the rule of ws_store_changes: the numpy model (changes_model.py) held to its own properties -- the self-comparison,
the identity pose against a comparison written without the sample, the swap of the two maps, the edges of the classes and of
min_weight -- and the declaration of the entry points.  No GPU."""
import numpy as np
import pytest

import changes_model as M
import fuse_model as F
import query_model as QM
from warpsense_amd import _lib

BAND, FREE, TAU = 64, 600, 600


def draw(seed, weights=(0, 1, 2, 3, 40)):
    """a chunk whose values sit on and around every class edge, with weights around min_weight"""
    rng = np.random.default_rng(seed)
    edges = np.array([-32768, -TAU, -BAND, -BAND + 1, -1, 0, BAND - 1, BAND, FREE - 1, FREE, 32767])
    value = np.where(rng.random(F.CW) < 0.5, rng.choice(edges, F.CW), rng.integers(-TAU, TAU + 1, F.CW))
    return F.pack(value, rng.choice(np.array(weights), F.CW))


def two_maps():
    cur = {(0, 0, 0): draw(1), (-1, 0, 0): draw(2), (0, -1, 1): draw(3)}
    ref = {(0, 0, 0): draw(4), (-1, 0, 0): draw(5), (0, -1, 1): draw(6)}
    return cur, ref


def test_a_map_against_itself_is_empty():
    cur, _ = two_maps()
    for mw in (1, 3):
        rec, labels, table, stats = M.changes(cur, cur, F.identity_pose(), 64, BAND, FREE, mw, flags=M.APPEARED | M.VANISHED | M.CLUSTERS)
        known = sum(int((F.unpack(c)[1] >= mw).sum()) for c in cur.values())
        assert len(rec) == 0 and len(labels) == 0 and len(table) == 0 and stats.tolist() == [3, known, 0, 0, 0, 0]


@pytest.mark.parametrize("mw", [1, 2, 3])
def test_identity_pose_is_the_plain_comparison(mw):
    """every fraction is 0: the sample is the REF entry itself, valid iff its weight > 0"""
    cur, ref = two_maps()
    del ref[(0, -1, 1)]  # present in CUR only: new ground, no record
    ref[(5, 5, 5)] = draw(7)  # present in REF only: never examined
    for pivot in ((0, 0, 0), (1000, -77, 13)):
        rec, _, _, stats = M.changes(cur, ref, F.identity_pose(pivot), 64, BAND, FREE, mw)
        want, wstats = M.direct(cur, ref, BAND, FREE, mw)
        assert rec.tobytes() == want.tobytes() and stats.tolist() == [3] + wstats and len(rec) > 1000
        assert stats[4] >= int((F.unpack(cur[(0, -1, 1)])[1] >= mw).sum()) > 0


def test_swapping_the_maps_swaps_the_kinds():
    cur, ref = two_maps()
    a = M.changes(cur, ref, F.identity_pose(), 64, BAND, FREE, 2)
    b = M.changes(ref, cur, F.identity_pose(), 64, BAND, FREE, 2)
    assert np.array_equal(a[0][["x", "y", "z"]], b[0][["x", "y", "z"]]) and np.array_equal(a[0]["kind"], 3 - b[0]["kind"])
    assert a[3][[1, 5]].tolist() == b[3][[1, 5]].tolist() and a[3][2] == b[3][3] and a[3][3] == b[3][2] and a[3][2] > 0 and a[3][3] > 0


def test_class_edges():
    d = np.array([-32768, -BAND, -BAND + 1, 0, BAND - 1, BAND, FREE - 1, FREE, 32767])
    assert M.classes(d, BAND, FREE).tolist() == [0, 0, 1, 1, 1, 0, 0, 2, 2]
    # band == free_value: the two classes touch and stay apart
    assert M.classes(np.array([BAND - 1, BAND]), BAND, BAND).tolist() == [1, 2]
    # through the whole model: one voxel per pair of values
    n = len(d)
    ev, nv = np.repeat(d, n), np.tile(d, n)
    cur, ref = np.full(F.CW, F.pack(TAU, 0), dtype=np.uint32), np.full(F.CW, F.pack(TAU, 0), dtype=np.uint32)
    cur[:n * n], ref[:n * n] = F.pack(ev, 5), F.pack(nv, 5)
    rec, _, _, stats = M.changes({(0, 0, 0): cur}, {(0, 0, 0): ref}, F.identity_pose(), 64, BAND, FREE)
    ce, cn = M.classes(ev, BAND, FREE), M.classes(nv, BAND, FREE)
    want = np.where((ce == 1) & (cn == 2), 1, np.where((ce == 2) & (cn == 1), 2, 0))
    assert stats.tolist() == [1, n * n, int((want == 1).sum()), int((want == 2).sum()), 0, int(np.abs(nv - ev).sum())]
    assert rec["kind"].tolist() == want[want != 0].tolist() and rec["ref_value"].tolist() == nv[want != 0].tolist() and int((want == 1).sum()) == 6


def test_min_weight_at_its_edge_on_either_side():
    mw = 7
    w = np.array([-5, 0, mw - 1, mw, 32767])
    ew, nw = np.repeat(w, len(w)), np.tile(w, len(w))
    kind, both, alone = M.kinds(np.zeros(25), ew, nw > 0, np.full(25, FREE), nw, BAND, FREE, mw)
    assert both.tolist() == ((ew >= mw) & (nw >= mw)).tolist() and alone.tolist() == ((ew >= mw) & (nw < mw)).tolist()
    assert kind.tolist() == np.where(both, 1, 0).tolist() and int(both.sum()) == 4 and int(alone.sum()) == 6
    # a valid sample below min_weight is not known; a sample that is not valid is not known whatever nw says
    assert M.kinds([0], [mw], [False], [FREE], [32767], BAND, FREE, mw)[2].tolist() == [True]


def test_kind_selection_filters_the_records_and_keeps_the_statistics():
    cur, ref = two_maps()
    full = M.changes(cur, ref, F.identity_pose(), 64, BAND, FREE)
    for flag in (M.APPEARED, M.VANISHED):
        part = M.changes(cur, ref, F.identity_pose(), 64, BAND, FREE, flags=flag)
        assert part[0].tobytes() == full[0][full[0]["kind"] == flag].tobytes() and part[3].tolist() == full[3].tolist() and len(part[0]) > 0


def test_stats_dataclass_and_record_layout():
    import warpsense_amd as W
    s = W.ChangeStats(3, 100, 5, 7, 11, 900)
    assert s.as_tuple() == (3, 100, 5, 7, 11, 900) and s.changed_volume_m3(64) == pytest.approx(12 * 0.064 ** 3) and s.disagreement_mm == 9.0
    assert W.CHANGE_RECORD == M.RECORD
    word = np.array([(0xFFFE & 0xFFFF) | (2 << 16)], dtype="<u4").view([("ref_value", "<i2"), ("kind", "<u2")])
    assert int(word["ref_value"][0]) == -2 and int(word["kind"][0]) == 2


def test_symbols_are_declared_bound_and_exported():
    L = _lib.load()
    names = {"ws_store_changes": 13, "ws_store_changes_records_dev": 2, "ws_store_changes_labels_dev": 2, "ws_store_changes_clusters_dev": 2,
             "ws_store_changes_download": 8, "ws_debug_store_changes_timing": 3}
    for name, n_params in names.items():
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        ret, params = QM._declared(name)
        assert len(params) == n_params and len(getattr(L, name).argtypes) == n_params, (name, params)
    assert QM._declared("ws_store_changes")[1] == ["ws_store *", "ws_store *", "const ws_fuse_pose *", "int32_t", "const int32_t [3]", "const int32_t [3]", "int32_t",
                                                   "int32_t", "int32_t", "uint32_t", "size_t *", "size_t *", "uint64_t [6]"]
    header = QM._header()
    for name, value in (("APPEARED", 1), ("VANISHED", 2), ("CLUSTERS", 4), ("DEFAULT", 3)):
        assert f"#define WS_CHANGES_{name} {value}u" in header and getattr(_lib, "WS_CHANGES_" + name) == value
