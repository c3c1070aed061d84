"""The point sample without a GPU: the boundary (symbols, header, ctypes signatures, flag values), the numpy model of the rules of
ws_map_sample / ws_store_sample on the fields of the ray-cast tests (test_gpu_raycast.Ring and field, test_store_raycast_host.Chunks)
against hand-computed literals, the model's own properties, the chunk lookup for points in absent chunks, and the inputs of the GPU
tests (tests/test_gpu_sample.py, tests/test_gpu_store_sample.py): every class and the non-zero gradients occur at least 16 times.

Everything is integer and compared exactly; there is no tolerance anywhere."""
import ctypes as C
import itertools
import re

import numpy as np

import query_model as QM
import raycast_model as R
from sample_model import CLASS_NAMES, FREE, INSIDE, RESOLUTIONS, SAMPLE, SURFACE, TAU, UNKNOWN, model, store_points, window_case
import store_raycast_scenes as SH
NEW_MAP = ["ws_map_sample", "ws_map_sample_dev", "ws_map_sample_records_dev", "ws_map_sample_gradient_dev", "ws_map_sample_selected_dev",
           "ws_map_sample_download", "ws_debug_sample_timing"]
NEW_STORE = ["ws_store_sample", "ws_store_sample_dev", "ws_store_sample_records_dev", "ws_store_sample_gradient_dev", "ws_store_sample_selected_dev",
             "ws_store_sample_download", "ws_debug_store_sample_timing"]
FLAGS = {"WS_SAMPLE_DEFAULT": 0, "WS_SAMPLE_ANY_WEIGHT": 1, "WS_SAMPLE_GRADIENT": 2, "WS_SAMPLE_SELECT_UNKNOWN": 4, "WS_SAMPLE_SELECT_FREE": 8,
         "WS_SAMPLE_SELECT_SURFACE": 16, "WS_SAMPLE_SELECT_INSIDE": 32}
CTYPE = dict(SH.CTYPE, **{"uint64_t [4]": C.c_void_p})


# ------------------------------------------------------------------------------------------------ the boundary
def test_library_exports_and_header_declares_the_sample_entry_points():
    from warpsense_amd import _lib
    L = _lib.load()
    h = QM._header()
    for name in NEW_MAP + NEW_STORE:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    for name, value in FLAGS.items():
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"u\b", h), name
        assert getattr(_lib, name) == value
    bits = [v for v in FLAGS.values() if v]
    assert len(set(bits)) == len(bits) and all(v & (v - 1) == 0 for v in bits)  # distinct single bits
    assert [FLAGS["WS_SAMPLE_SELECT_" + c.upper()] for c in CLASS_NAMES] == [4 << c for c in range(4)] and _lib.SAMPLE_CLASSES == CLASS_NAMES
    flat = " ".join(h.replace("\n *", " ").split())  # the comment as running text: re-wrapping it changes nothing
    for phrase in ("int32 d_mm = floor(T(p) / res^3), or 0 if the cell is not valid", "nearest voxel g = floor(p / res)", "2 SURFACE  -band < d_mm < band",
                   "a dead point: class 0, record all zero", "It is an ordered compaction", "On a refusal nothing is launched and the last result stays",
                   "a voxel of an absent chunk is not valid whatever fill_entry is", "return the same bytes in all three arrays"):
        assert " ".join(phrase.split()) in flat, phrase


def test_ctypes_signatures_agree_with_the_header():
    from warpsense_amd import _lib
    import warpsense_amd as W
    L = _lib.load()
    for name in NEW_MAP + NEW_STORE:
        ret, params = QM._declared(name)
        fn = getattr(L, name)
        assert list(fn.argtypes) == [CTYPE[p] for p in params], (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name
        else:
            assert ret == "int" and fn.restype is C.c_int, name
    assert W.SAMPLE == SAMPLE and W.SAMPLE.itemsize == 16


# ------------------------------------------------------------------------------------------------ by hand
def _cell(values, weights, lo=(0, 0, 0)):
    import warpsense_amd as W
    box = W.pack_entry(np.asarray(values).reshape(-1), np.asarray(weights).reshape(-1)).astype(np.uint32).reshape(2, 2, 2)
    return R.Ring.of_box(box, lo), box


def test_hand_computed_cell():
    """res = 50, h = 25, the cell at base voxel (0, 0, 0), the point (35, 50, 74): q = (10, 25, 49) = f.  Weights per axis: x (40, 10),
    y (25, 25), z (1, 49).  Values v[cx][cy][cz] = 100, 200 | -50, 30 || 400, -300 | 60, -20:
      T = 100 1000 + 200 49000 - 50 1000 + 30 49000 + 400 250 - 300 12250 + 60 250 - 20 12250
        = 100000 + 9800000 - 50000 + 1470000 + 100000 - 3675000 + 15000 - 245000 = 7515000
      d_mm = floor(7515000 / 125000) = floor(60.12) = 60.  band 60: FREE (d >= band); band 61: SURFACE.
      g = floor(p / 50) = (0, 1, 1): raw is the entry (30, weight 13).  The smallest weight is 10."""
    values = [[[100, 200], [-50, 30]], [[400, -300], [60, -20]]]
    weights = 10 + np.arange(8)
    ring, box = _cell(values, weights)
    p = np.array([[35, 50, 74]])
    ok, T = R.field(ring, 50, p.astype(np.int64), False)
    assert ok[0] and int(T[0]) == 7515000
    rec, counts, grad, sel = model(ring, 50, p, 60, select=(FREE,))
    assert (int(rec["d_mm"][0]), int(rec["weight"][0]), int(rec["cls"][0])) == (60, 10, FREE)
    assert int(rec["raw"][0]) == int(box[0, 1, 1]) == (30 | (13 << 16))
    assert counts.tolist() == [0, 1, 0, 0] and sel.tolist() == [[35, 50, 74]] and not grad.any()
    rec, counts, _, sel = model(ring, 50, p, 61, select=(FREE,))
    assert int(rec["cls"][0]) == SURFACE and counts.tolist() == [0, 0, 1, 0] and len(sel) == 0
    # the mirrored values: T = -7515000, floor(-60.12) = -61 where truncation gives -60.  band 61: INSIDE; band 62: SURFACE
    ring_n, _ = _cell(-np.asarray(values), weights)
    rec = model(ring_n, 50, p, 61)[0]
    assert (int(rec["d_mm"][0]), int(rec["cls"][0])) == (-61, INSIDE)
    assert int(model(ring_n, 50, p, 62)[0]["cls"][0]) == SURFACE
    # a negative weight among the corners: not valid by default (record 0, 0, UNKNOWN, raw still given); under ANY_WEIGHT |weight| counts
    w2 = weights.copy()
    w2[5] = -3
    ring_w, box_w = _cell(values, w2)
    rec = model(ring_w, 50, p, 60)[0]
    assert (int(rec["d_mm"][0]), int(rec["weight"][0]), int(rec["cls"][0]), int(rec["raw"][0])) == (0, 0, UNKNOWN, int(box_w[0, 1, 1]))
    rec = model(ring_w, 50, p, 60, any_weight=True)[0]
    assert (int(rec["d_mm"][0]), int(rec["weight"][0]), int(rec["cls"][0])) == (60, 3, FREE)


def test_a_point_on_the_sample_lattice_returns_that_voxel():
    """f = 0: the point v res + h of voxel v.  At a negative coordinate floor and truncation differ: voxel (-3, -1, -2) at res 50 sits
    at (-125, -25, -75); trunc(-125 / 50) = -2, floor = -3."""
    values = np.array([[[100, 200], [-50, 30]], [[400, -300], [60, -20]]])
    for lo in ((0, 0, 0), (-3, -1, -2)):
        ring, box = _cell(values, np.full(8, 64), lo)
        for c in itertools.product((0, 1), repeat=3):
            v = np.asarray(lo) + np.asarray(c)
            rec = model(ring, 50, (v * 50 + 25)[None, :], 10_000)[0]
            # (only the cell at `lo` lies inside the 2 x 2 x 2 window: the other corners' cells reach out of it)
            want_ok = c == (0, 0, 0)
            assert int(rec["raw"][0]) == int(box[c]), (lo, c)
            assert (int(rec["d_mm"][0]), int(rec["cls"][0])) == ((int(values[c]), SURFACE) if want_ok else (0, UNKNOWN)), (lo, c)
    assert model(_cell(values, np.full(8, 64), (-3, -1, -2))[0], 50, [[-125, -25, -75]], 10_000)[0]["d_mm"][0] == 100


# ------------------------------------------------------------------------------------------------ the model's properties and the inputs
def test_model_properties_on_the_inputs_of_the_gpu_tests():
    for (size, seed), res in itertools.product(R.RANDOM_MAPS, RESOLUTIONS):
        for which in (0, 1):
            data, pos, off, ring, pts, band = window_case(size, seed, res, which)
            for any_weight in (False, True):
                rec, counts, grad, sel = model(ring, res, pts, band, any_weight, select=(FREE, INSIDE))
                n_grad = int(np.count_nonzero(np.any(grad != 0, axis=1)))
                print(size, res, which, any_weight, counts.tolist(), n_grad)
                # a condition on the INPUTS: every class, and the non-zero gradients, occur
                assert counts.min() >= 16 and n_grad >= 16, (size, res, which, any_weight, counts, n_grad)
                # the class partition is total and disjoint
                assert int(counts.sum()) == len(pts) and np.all(rec["cls"] <= 3)
                valid = rec["cls"] != UNKNOWN
                assert np.all(rec["d_mm"][~valid] == 0) and np.all(rec["weight"][~valid] == 0) and np.all(rec["weight"][valid] > 0)
                d = rec["d_mm"].astype(np.int64)
                assert np.array_equal(rec["cls"][valid], np.where(d >= band, FREE, np.where(d <= -band, INSIDE, SURFACE))[valid])
                # d_mm at a sample-lattice point equals the voxel's value, which is the nearest voxel's
                on = valid & np.all((pts - res // 2) % res == 0, axis=1)
                assert on.sum() >= 16 and np.array_equal(d[on], QM.unpack(rec["raw"][on])[0])
                # the selection is the ordered subsequence of the input
                keep = np.isin(rec["cls"], (FREE, INSIDE))
                assert np.array_equal(sel, pts[keep].astype(np.int32)) and len(sel) == int(counts[FREE] + counts[INSIDE])
                # dead points
                dead = np.any(np.abs(pts) >= 2 ** 30, axis=1)
                assert dead.sum() == 4 and not rec[dead].tobytes().strip(b"\0") and not grad[dead].any()


# ------------------------------------------------------------------------------------------------ the store: points in absent chunks
def test_chunk_lookup_route_for_points_in_absent_chunks():
    """ws_store_sample finds a point's chunk through the table of ws_store_raycast.  For the seam store (seven chunks around the origin,
    one of the eight absent): the table answers STORE_ABSENT for the base voxel's chunk of every point in the absent chunk, the model
    calls those points UNKNOWN with raw 0, and a point next to it whose cell has one voxel in it UNKNOWN with raw given."""
    import store_scenes as SM
    from warpsense_amd import _lib
    L = _lib.load()
    chunks = SM.seam_chunks()
    keys = sorted(chunks)
    rows = np.ascontiguousarray(np.concatenate([np.asarray(keys, dtype=np.int32), np.arange(len(keys), dtype=np.int32)[:, None]], axis=1))
    places = C.c_size_t(0)
    assert L.ws_debug_store_raycast_table(rows.ctypes.data_as(C.c_void_p), len(keys), None, 0, C.byref(places)) == 0
    table = np.zeros((places.value, 4), dtype=np.int32)
    assert L.ws_debug_store_raycast_table(rows.ctypes.data_as(C.c_void_p), len(keys), table.ctypes.data_as(C.c_void_p), places.value, C.byref(places)) == 0
    find = lambda key: L.ws_debug_store_raycast_find(table.ctypes.data_as(C.c_void_p), places.value, np.ascontiguousarray(key, dtype=np.int32).ctypes.data_as(C.c_void_p))
    fld = SH.Chunks(chunks)
    pts = store_points(seed=3)
    rec = model(fld, SM.RES, pts, TAU // 2, any_weight=True)[0]
    key_b = ((pts - SM.RES // 2) // SM.RES) >> 6
    key_g = (pts // SM.RES) >> 6
    absent = np.asarray(SM.ABSENT)
    in_absent_b, in_absent_g = np.all(key_b == absent, axis=1), np.all(key_g == absent, axis=1)
    assert in_absent_b.sum() >= 16
    for i in np.flatnonzero(in_absent_b)[:64]:
        assert find(key_b[i]) == 0xffffffff and int(rec["cls"][i]) == UNKNOWN
    for i in np.flatnonzero(~in_absent_g & np.all(np.abs(key_g) <= 1, axis=1) & np.all(key_g >= -1, axis=1) & np.all(key_g <= 0, axis=1))[:64]:
        assert find(key_g[i]) == keys.index(tuple(int(v) for v in key_g[i]))
    assert not rec["raw"][in_absent_g].any() and np.all(rec["cls"][in_absent_g] == UNKNOWN)
    # next to the absent chunk: the nearest voxel is in a present chunk, one corner of the cell is not
    beside = ~in_absent_g & np.all(np.abs(key_g) <= 1, axis=1) & (rec["cls"] == UNKNOWN) & (rec["raw"] != 0)
    touching = np.zeros(len(pts), dtype=bool)
    b = (pts - SM.RES // 2) // SM.RES
    for c in itertools.product((0, 1), repeat=3):
        touching |= np.all(((b + np.asarray(c)) >> 6) == absent, axis=1)
    assert np.count_nonzero(beside & touching) >= 16


def test_store_inputs_hold_every_class():
    import store_scenes as SM
    pts = store_points(seed=3)
    for any_weight in (False, True):
        rec, counts, grad, _ = model(SH.Chunks(SM.seam_chunks()), SM.RES, pts, TAU // 2, any_weight)
        n_grad = int(np.count_nonzero(np.any(grad != 0, axis=1)))
        print(any_weight, counts.tolist(), n_grad)
        assert counts.min() >= 16 and n_grad >= 16
