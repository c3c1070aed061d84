"""The ray cast of the store without a GPU: the boundary (symbols, header, ctypes signatures), the `Chunks` field that
tests/test_gpu_store_raycast.py hands to the numpy model of the window's ray cast (test_gpu_raycast.model), the chunk lookup of the
kernels against a dict, and the inputs of the GPU tests: for every ray set the model alone yields hits and no-hits.

The ray sets live here, so that the GPU tests and these checks use the same ones; a model result is computed once per process."""
import ctypes as C
import re

import numpy as np

import query_model as QM
import raycast_model as R
from store_raycast_scenes import CS, CTYPE, Chunks, STEP, all_cases, first_sample_in, gap_cases, gap_dirs, hits_of, seam_cases, want
import store_scenes as SM

NEW = ["ws_store_raycast", "ws_store_raycast_dev", "ws_store_raycast_records_dev", "ws_store_raycast_gradient_dev", "ws_store_raycast_download",
       "ws_debug_store_raycast_timing"]


# ------------------------------------------------------------------------------------------------ the tests
def test_library_exports_and_header_declares_the_store_raycast_entry_points():
    from warpsense_amd import _lib
    L = _lib.load()
    h = QM._header()
    for name in NEW + ["ws_debug_store_raycast_table", "ws_debug_store_raycast_find"]:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    for phrase in ("word for word those of ws_map_raycast", "chunk is NOT VALID, whatever fill_entry is", "Both NULL: everything",
                   "ws_map_raycast on that window returns the\n *     same bytes", "never anything that follows the volume of the box",
                   "apart from\n *     those of ws_store_mesh"):
        assert phrase in h, phrase


def test_ctypes_signatures_agree_with_the_header():
    from warpsense_amd import _lib
    L = _lib.load()
    for name in NEW:
        ret, params = QM._declared(name)
        fn = getattr(L, name)
        assert list(fn.argtypes) == [CTYPE[p] for p in params], (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name
        else:
            assert ret == "int" and fn.restype is C.c_int, name
    assert len(QM._declared("ws_store_raycast")[1]) == 10 and QM._declared("ws_store_raycast")[1] == QM._declared("ws_store_raycast_dev")[1]


def test_chunks_field_agrees_with_the_ring_of_the_assembled_box():
    chunks = SM.seam_chunks()
    rng = np.random.default_rng(5)
    for lo, hi in [SM.bounding_box(chunks), ((-40, -29, -50), (37, 45, 20)), ((-100, -90, -70), (90, 100, 130))]:
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        ring = R.Ring.of_box(SM.assemble(chunks, lo, hi), lo)
        assert np.array_equal(ring.lo, lo) and np.array_equal(ring.hi, hi)
        field = Chunks(chunks, lo, hi)
        v = rng.integers(-140, 141, (6000, 3))
        v[:1500] = rng.integers(-3, 4, (1500, 3))  # around the common corner, the absent chunk among them
        for any_weight in (False, True):
            (va, oka), (vb, okb) = field.entries(v, any_weight), ring.entries(v, any_weight)
            assert np.array_equal(oka, okb) and np.array_equal(va[oka], vb[okb])
            assert 500 < np.count_nonzero(oka) < 5500
        absent = np.all(v >> 6 == np.asarray(SM.ABSENT), axis=1)
        assert absent.sum() > 100 and not field.entries(v, True)[1][absent].any()
    # without a box: everything the chunks hold, nothing else
    free = Chunks(chunks)
    v = rng.integers(-140, 141, (4000, 3))
    inside = np.all((v >= -64) & (v <= 63), axis=1) & ~np.all(v >> 6 == np.asarray(SM.ABSENT), axis=1)
    assert not free.entries(v, True)[1][~inside].any() and free.entries(v, True)[1][inside].any()
    assert not Chunks({}).entries(v, True)[1].any()


def test_chunk_lookup_against_a_dict():
    from warpsense_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(23)
    for n in (0, 1, 2, 3, 7, 1000):
        keys = np.unique(rng.integers(-300, 301, (n, 3)), axis=0).astype(np.int32) if n else np.zeros((0, 3), dtype=np.int32)
        n = len(keys)
        rows = np.concatenate([keys, rng.permutation(n).astype(np.int32).reshape(n, 1)], axis=1).astype(np.int32)
        rows = np.ascontiguousarray(rows)
        places = C.c_size_t(0)
        assert L.ws_debug_store_raycast_table(rows.ctypes.data_as(C.c_void_p), n, None, 0, C.byref(places)) == 0
        size = places.value
        assert size >= max(2, 2 * n) and size & (size - 1) == 0 and size < max(4, 4 * n)  # a power of two >= 2 n, sized by the chunks
        table = np.zeros((size, 4), dtype=np.int32)
        assert L.ws_debug_store_raycast_table(rows.ctypes.data_as(C.c_void_p), n, table.ctypes.data_as(C.c_void_p), size, C.byref(places)) == 0
        assert np.count_nonzero(table[:, 3] != -1) == n
        want_slot = {tuple(int(v) for v in r[:3]): int(r[3]) for r in rows}
        probes = np.concatenate([keys, rng.integers(-310, 311, (500, 3)).astype(np.int32)])
        for key in probes:
            k3 = np.ascontiguousarray(key, dtype=np.int32)
            got = L.ws_debug_store_raycast_find(table.ctypes.data_as(C.c_void_p), size, k3.ctypes.data_as(C.c_void_p))
            assert got == want_slot.get(tuple(int(v) for v in key), 0xffffffff), key


def test_every_ray_set_has_hits_and_no_hits_in_the_model():
    for case in all_cases():
        if case["name"] in ("box one voxel thick", "box in the absent chunk", "box far away"):
            assert hits_of(want(case)[0]) == 0, case["name"]  # no cells: the case is that nothing hits
            continue
        rec, grad = want(case)
        n = hits_of(rec)
        assert 0 < n < len(rec), (case["name"], n, len(rec))
        assert np.any(grad[rec["range_mm"] >= 0] != 0) or case["name"].startswith(("gap", "range", "box two voxels")), case["name"]
    n_seam = [hits_of(want(c)[0]) for c in seam_cases()]
    assert min(n_seam[0], n_seam[1], n_seam[2]) > 100, n_seam


def test_gap_hits_start_at_the_first_sample_behind_the_gap():
    """the +x, +y, +z axis rays of the gap cases hit, and p_{k-1} of the hit is the FIRST sample whose base voxel lies in the far
    chunk, at every phase: a jump that lands one sample late loses the hit"""
    d = gap_dirs()
    n_first = 0
    for j, case in enumerate(gap_cases()):
        rec = want(case)[0]
        for r, key in ((0, (2, 0, 0)), (8, (0, 2, 0)), (16, (0, 0, 2))):  # the axis rays of the three + rows
            k0 = int(first_sample_in(case["origin"], d[r:r + 1], key, case["range"] // STEP)[0])
            assert k0 > 2 * CS and rec["range_mm"][r] >= 0, (j, r)
            assert k0 * STEP <= rec["range_mm"][r] <= (k0 + 1) * STEP, (j, r, k0, rec["range_mm"][r])
            n_first += 1
        assert hits_of(rec[[4, 12, 20, 24, 28]]) >= 4, j  # the - rows and the diagonal hit too
    assert n_first == 3 * 2 * STEP
