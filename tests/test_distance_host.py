"""The distance field without a GPU: the boundary (symbols, header, ctypes signatures), and the numpy model of the rules
(tests/test_gpu_distance.py) against a brute-force minimum over all (voxel, site) pairs, a hand-computed literal and -- where it
imports -- scipy's Euclidean transform; the input condition of the GPU tests' draws; the record helpers."""
import ctypes as C
import re

import numpy as np

from distance_model import CTYPE, brute
import distance_model as D
import query_model as QM

NEW = ["ws_map_distance", "ws_map_distance_dev", "ws_map_distance_download", "ws_debug_distance_timing"]
FLAGS = {"WS_DISTANCE_DEFAULT": 0, "WS_DISTANCE_ANY_WEIGHT": 1, "WS_DISTANCE_UNKNOWN_OCCUPIED": 2, "WS_DISTANCE_COLUMNS": 4}


def test_library_exports_and_header_declares_the_distance_entry_points():
    from warpsense_amd import _lib
    import warpsense_amd as W
    L = _lib.load()
    h = QM._header()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    for name, value in FLAGS.items():
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"u\b", h), name
        assert getattr(_lib, name) == value and getattr(W, name) == value
    # the rules are stated where the ABI is declared
    for phrase in ("min(R², min over sites", "x major, z fastest", "bits 30..31", "1 <= R <= 255", "Voxels outside the box are never sites", "nx ny records"):
        assert phrase in h, phrase


def test_ctypes_signatures_agree_with_the_header():
    from warpsense_amd import _lib
    L = _lib.load()
    for name in NEW:
        ret, params = QM._declared(name)
        fn = getattr(L, name)
        want = [CTYPE[p] for p in params]
        assert list(fn.argtypes) == want, (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name  # a pointer must not be cut to the default 32-bit int
        else:
            assert ret == "int" and fn.restype is C.c_int, name


def test_model_equals_the_brute_force_minimum():
    """the seven box shapes of the GPU tests, R in {1, 3, 7, 40, 255}, all flag combinations; scipy as a third witness where it is
    installed (the brute force is the judge)"""
    try:
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        distance_transform_edt = None
    compared = 0
    for size in D.SIZES:
        box = D.draw_entries(size, D.seeds_for(size, 0)).reshape(size)
        for kw in D.FLAGS:
            for R in D.RANGES:
                want, n_sites = brute(box, R, **kw)
                got, n_model = D.model_box(box, R, **kw)
                assert D.same(got, want) and n_model == n_sites, (size, kw, R)
                compared += 1
                if distance_transform_edt is not None and n_sites:
                    site = D.sites_and_classes(box, **kw)[0]
                    edt = np.rint(distance_transform_edt(~site) ** 2).astype(np.int64)
                    assert np.array_equal(np.minimum(edt, R * R), (got & np.uint32(0xFFFFFF)).astype(np.int64)), (size, kw, R)
    assert compared == 7 * 8 * 5


def test_model_reproduces_the_hand_computed_case():
    """One site in a 5 x 5 x 5 box, R = 3: the occupied voxel at (2, 1, 3), every other voxel free except (0, 0, 0), unknown.
    d2 = dx^2 + dy^2 + dz^2 where that is below 9, else 9; written out plane by plane (x = 0 .. 4; rows y, columns z)."""
    import warpsense_amd as W
    value, weight = np.full((5, 5, 5), 20), np.full((5, 5, 5), 64)
    value[2, 1, 3] = -1
    weight[0, 0, 0] = 0
    box = W.pack_entry(value.reshape(-1), weight.reshape(-1)).astype(np.uint32).reshape(5, 5, 5)
    plane2 = [[9, 5, 2, 1, 2],   # x = 2, y = 0: 1 + dz^2, dz = 3 .. -1
              [9, 4, 1, 0, 1],   # y = 1
              [9, 5, 2, 1, 2],   # y = 2
              [9, 8, 5, 4, 5],   # y = 3: 4 + dz^2
              [9, 9, 9, 9, 9]]   # y = 4: 9 + dz^2 >= 9
    plane1 = [[9, 6, 3, 2, 3],   # x = 1 and x = 3: one more
              [9, 5, 2, 1, 2],
              [9, 6, 3, 2, 3],
              [9, 9, 6, 5, 6],
              [9, 9, 9, 9, 9]]
    plane0 = [[9, 9, 6, 5, 6],   # x = 0 and x = 4: four more
              [9, 8, 5, 4, 5],
              [9, 9, 6, 5, 6],
              [9, 9, 9, 8, 9],
              [9, 9, 9, 9, 9]]
    d2 = np.array([plane0, plane1, plane2, plane1, plane0], dtype=np.uint32)
    want = d2 | np.uint32(1 << 30)
    want[2, 1, 3] = np.uint32(2 << 30)
    want[0, 0, 0] = 9
    rec, n_sites = D.model_box(box, 3)
    assert n_sites == 1 and D.same(rec, want) and rec.reshape(-1).size == 125
    assert D.same(brute(box, 3)[0], want)
    # the conservative reading: (0, 0, 0) is a site too, its neighbours are 1 away
    rec_u, n_u = D.model_box(box, 3, unknown_occupied=True)
    assert n_u == 2 and rec_u[0, 0, 0] == 0 and rec_u[0, 0, 1] == (1 << 30) | 1 and rec_u[1, 1, 1] == (1 << 30) | 3 and rec_u[2, 1, 3] == 2 << 30
    # columns: the site column is (2, 1); 2-D distances; column (0, 0) has free voxels, so it is free
    col, n_c = D.model_box(box, 3, columns=True)
    want_c = np.array([[5, 4, 5, 8, 9], [2, 1, 2, 5, 9], [1, 0, 1, 4, 9], [2, 1, 2, 5, 9], [5, 4, 5, 8, 9]], dtype=np.uint32) | np.uint32(1 << 30)
    want_c[2, 1] = np.uint32(2 << 30)
    assert n_c == 1 and D.same(col, want_c)
    # a box without any site; the clamp at R = 1
    assert np.all(D.model_box(box[3:], 3)[0] == (1 << 30) | 9) and D.model_box(box[3:], 3)[1] == 0
    assert sorted(set((D.model_box(box, 1)[0] & np.uint32(0xFFFFFF)).reshape(-1).tolist())) == [0, 1]
    assert W.distance_class(want).tolist() == (want >> 30).tolist() and W.distance_d2(want).tolist() == d2.tolist()
    mm = W.distance_mm(want, 50)
    assert mm.dtype == np.float32 and mm[2, 1, 3] == 0 and mm[2, 1, 2] == 50 and mm[4, 4, 4] == 150 and mm[1, 1, 2] == np.float32(50) * np.sqrt(np.float32(2))


def test_committed_seeds_meet_the_input_condition():
    """the draws of tests/test_gpu_distance.py, checked where no GPU is needed: per map, default flags, R in {3, 7}: at least 3
    sites, at least 3 % of the records strictly between 0 and R^2, at least 2 % at R^2"""
    for size in D.SIZES:
        for which in (0, 1):
            shares = D.check_inputs(D.draw_entries(size, D.seeds_for(size, which)), size)
            print(size, which, [(n, round(b, 3), round(c, 3)) for n, b, c in shares])
    for shape, seeds in (((21, 17, 13), (5, 1005)), ((15, 15, 15), (22, 1022))):
        for seed in seeds:
            D.check_inputs(D.draw_entries(shape, seed), shape)
    # under ANY_WEIGHT the three planted negative-weight entries with negative values join, nothing else does
    size = D.SIZES[0]
    box = D.draw_entries(size, D.seeds_for(size, 0)).reshape(size)
    assert D.model_box(box, 7, any_weight=True)[1] == D.model_box(box, 7)[1] + 3


def test_metres_to_voxels_rule():
    """TSDFMapping.distance_field: metres to whole millimetres (nearest), then ceil(mm / res) voxels"""
    import warpsense_amd as W

    class FakeMap:
        def distance(self, **kw):
            return kw["max_dist_vox"]

    class FakeTsdf:
        def avg_map(self):
            return FakeMap()
    tm = W.TSDFMapping.__new__(W.TSDFMapping)
    import threading
    tm.mutex_, tm.tsdf_ = threading.RLock(), FakeTsdf()
    tm.params_ = W.Params(W.MapParams(resolution=50))
    assert [tm.distance_field(max_dist_m=m) for m in (0.05, 0.051, 0.3, 0.301, 0.35, 1.0, 2.0, 12.75)] == [1, 2, 6, 7, 7, 20, 40, 255]
