"""The distance field of the store without a GPU: the boundary (symbols, header, ctypes signatures, the rule phrases), the model on a
box assembled from chunks (tests/test_gpu_store_distance.py) against the brute-force minimum over all (voxel, site) pairs, the input
condition of every draw the GPU tests use, and the metres-to-voxels rule of TSDFMapping.global_distance_field."""
import ctypes as C
import re

import numpy as np

import distance_model as DH
import query_model as QM
import store_distance_scenes as SD
import store_scenes as SM

NEW = ["ws_store_distance", "ws_store_distance_dev", "ws_store_distance_download", "ws_debug_store_distance_timing"]
CTYPE = dict(DH.CTYPE, **{"ws_store *": C.c_void_p, "const ws_store *": C.c_void_p})


def test_library_exports_and_header_declares_the_store_distance_entry_points():
    from warpsense_amd import _lib
    L = _lib.load()
    h = QM._header()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    for name in NEW:
        ret, params = QM._declared(name)
        fn = getattr(L, name)
        want = [CTYPE[p] for p in params]
        assert list(fn.argtypes) == want, (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name  # a pointer must not be cut to the default 32-bit int
        else:
            assert ret == "int" and fn.restype is C.c_int, name


def test_header_states_the_rules():
    h = QM._header()
    block = h[h.index("/* The distance field of the store"):h.index("int ws_debug_store_distance_timing")]
    flat = re.sub(r"\s*\n \*\s*", " ", block)
    for phrase in ("absent chunk is NOT VALID", "whatever fill_entry is", "it counts in *n_sites", "word for word the rule set of ws_map_distance",
                   "which lie inside the box only", "1 <= R <= 255", "min(R², min over sites", "bits 30..31", "x major, z fastest", "nx ny records, y fastest",
                   "occupied wins, then unknown-as-site, then free", "Extents are formed in 64 bits", "the bounding box of the present chunks",
                   "zero records and zero sites", "2^32 - 1 records", "2^19 present chunks", "nothing is launched and the last result stays",
                   "leaves the store usable", "this result is DENSE", "8 bytes per record", "absent chunks are never read",
                   "never follows the volume of the box",
                   "ws_map_distance on that window and box returns the same bytes and the same site count, under every flag combination"):
        assert phrase in flat, phrase


def test_assembled_model_equals_the_brute_force_minimum():
    """one cut box across the common corner of 8 chunks, one of them absent; all 8 flag combinations, R in {1, 3, 7}"""
    chunks = SD.seam_chunks()
    assert len(chunks) == 7 and SD.ABSENT not in chunks
    lo, hi = (-5, -4, -6), (4, 6, 3)
    box = SM.assemble(chunks, lo, hi)
    assert box.shape == (10, 11, 10) and not box[5:, 4:, :6].any() and np.count_nonzero(box) > 700  # the absent octant is raw 0
    compared = 0
    for kw in DH.FLAGS:
        for R in (1, 3, 7):
            want, n_sites = DH.brute(box, R, **kw)
            got, n_model = SD.model(chunks, lo, hi, R, **kw)
            assert DH.same(got, want) and n_model == n_sites, (kw, R)
            compared += 1
            if kw["unknown_occupied"] and not kw["columns"]:
                assert n_sites >= 5 * 7 * 6 and not got[5:, 4:, :6].any()  # every voxel of the absent chunk is a site
    assert compared == 8 * 3


def test_committed_seeds_meet_the_input_condition():
    """every draw of tests/test_gpu_store_distance.py: default flags, R in {3, 7}: at least 3 sites, at least 3 % of the records strictly
    between 0 and R^2, at least 2 % at R^2 (test_gpu_distance.check_inputs)"""
    assert len(SD.SEEDS) == 19 and len(set(SD.SEEDS)) == 19
    for shape, seed in SD.SEEDS:
        shares = DH.check_inputs(DH.draw_entries(shape, seed), shape)
        print(shape, seed, [(n, round(b, 3), round(c, 3)) for n, b, c in shares])
    # the chunks of the GPU tests are these draws
    assert np.array_equal(SD.seam_chunks()[(-1, -1, -1)], DH.draw_entries((64,) * 3, SD.SEAM_SEED))
    assert np.array_equal(SD.pillar_chunks(SD.PILLAR_Z, SD.PILLAR_Z_SEED)[(0, 0, 2)], DH.draw_entries((64,) * 3, SD.PILLAR_Z_SEED + 4))
    assert SD.PILLAR_Z[SD.HOLE] == (0, 0, 0) and (0, 0, 0) not in SD.pillar_chunks(SD.PILLAR_Z, SD.PILLAR_Z_SEED)
    assert SD.PILLAR_Y[SD.HOLE] == (0, 0, 0) and (0, 0, 0) not in SD.pillar_chunks(SD.PILLAR_Y, SD.PILLAR_Y_SEED)


def test_metres_to_voxels_rule_of_the_global_field():
    """TSDFMapping.global_distance_field: metres to whole millimetres (nearest), then ceil(mm / res) voxels, as distance_field; the
    window goes into the chunks first; without a device global map the error of global_mesh"""
    import threading

    import pytest
    import warpsense_amd as W
    calls = []

    class FakeStore:
        def save_box(self, tsdf, lo, hi):
            calls.append(("save", tuple(lo), tuple(hi)))

        def distance(self, **kw):
            calls.append(("distance", kw["lo"], kw["hi"], kw["columns"]))
            return kw["max_dist_vox"]

    class FakeLocalMap:
        def window(self):
            return (-3, -2, -1), (3, 2, 1)
    tm = W.TSDFMapping.__new__(W.TSDFMapping)
    tm.mutex_, tm.tsdf_, tm.local_map_, tm.device_global_map_ = threading.RLock(), object(), FakeLocalMap(), FakeStore()
    tm.wait_shift = lambda: calls.append(("wait",))
    tm.params_ = W.Params(W.MapParams(resolution=50))
    assert [tm.global_distance_field(max_dist_m=m) for m in (0.05, 0.051, 0.3, 0.301, 0.35, 1.0, 2.0, 12.75)] == [1, 2, 6, 7, 7, 20, 40, 255]
    assert calls[:3] == [("wait",), ("save", (-3, -2, -1), (3, 2, 1)), ("distance", None, None, False)]
    assert tm.global_distance_field(lo=(0, 0, 0), hi=(1, 1, 1), columns=True) == 20 and calls[-1] == ("distance", (0, 0, 0), (1, 1, 1), True)
    tm.device_global_map_ = None
    with pytest.raises(W.WsError, match="no device_global_map"):
        tm.global_distance_field()
