"""The surface cloud of the store without a GPU: the boundary (symbols, header, ctypes signatures), the model of the GPU tests --
test_gpu_surface.model_box on test_gpu_store_mesh.assemble -- against a hand-built two-chunk case, and the inputs of the GPU tests."""
import ctypes as C
import re

import numpy as np

import query_model as QM
import store_scenes as SM
import store_surface_scenes as SS
import surface_model as G

NEW = ["ws_store_surface", "ws_store_surface_records_dev", "ws_store_surface_marker_dev", "ws_store_surface_download", "ws_debug_store_surface_timing"]
CTYPE = dict(QM.CTYPE, **{"ws_store *": C.c_void_p, "const ws_store *": C.c_void_p, "float *": C.c_void_p})


def test_library_exports_and_header_declares_the_store_surface_entry_points():
    from warpsense_amd import _lib
    L = _lib.load()
    h = QM._header()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    # the semantics are stated where the ABI is declared
    flat = re.sub(r"\s*\n \*\s*", " ", h)  # (a phrase may run over a line break of the comment)
    for phrase in ("never qualifies, whatever fill_entry is", "across chunk borders", "ws_map_surface on that window and box returns the same bytes"):
        assert phrase in flat, phrase


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


def test_model_on_a_hand_built_two_chunk_case():
    import warpsense_amd as W
    tau, res, band = 1000, 50, 400
    a, b = np.zeros((64, 64, 64), dtype=np.uint32), np.zeros((64, 64, 64), dtype=np.uint32)
    e = lambda value, weight: np.uint32(W.pack_entry(value, weight))
    a[63, 2, 5], a[63, 2, 6], a[0, 0, 0], a[62, 63, 63] = e(100, 3), e(-399, 1), e(-50, 64), e(0, 1)   # qualify
    a[63, 2, 7], a[63, 3, 0], a[10, 10, 10] = e(100, 0), e(400, 5), e(-32768, 9)                        # weight; band; abs as int32
    b[0, 2, 5], b[0, 0, 63], b[63, 63, 63] = e(-200, 2), e(399, 640), e(1, 1)                           # qualify
    b[0, 2, 4], b[1, 1, 1] = e(10, -5), e(-400, 7)                                                      # weight; band
    chunks = {(-1, 0, 0): a.reshape(-1), (0, 0, 0): b.reshape(-1)}  # world x -64 .. -1 and 0 .. 63: the seam is the plane x = 0
    lo, hi = SM.bounding_box(chunks)
    rec, mk = G.model_box(SM.assemble(chunks, lo, hi), lo, tau, res, band)
    want = [(-64, 0, 0, e(-50, 64)), (-2, 63, 63, e(0, 1)), (-1, 2, 5, e(100, 3)), (-1, 2, 6, e(-399, 1)),
            (0, 0, 63, e(399, 640)), (0, 2, 5, e(-200, 2)), (63, 63, 63, e(1, 1))]
    assert [tuple(int(v) for v in r) for r in rec] == [tuple(int(v) for v in r) for r in want]
    F = np.float32
    assert mk.shape == (7, 7) and mk.dtype == F
    assert mk[3].tolist() == [F(-1) * F(50) / F(1000), F(2) * F(50) / F(1000), F(6) * F(50) / F(1000), 0.0, F(399) / F(1000), 0.0, 1.0]
    assert mk[4].tolist() == [0.0, 0.0, F(63) * F(50) / F(1000), F(399) / F(1000), 0.0, 0.0, 1.0]
    # SS.model_store is that model with the default box, and the band defaults to tau: the two voxels that failed on the band alone join
    assert SS.same2(SS.model_store(chunks, tau, res, band=band), (rec, mk))
    assert len(SS.model_store(chunks, tau, res)[0]) == 9
    # a box that cuts both chunks and reaches into absent space; one that lies in absent space
    cut = SS.model_store(chunks, tau, res, (-1, 2, -3), (0, 70, 5), band)[0]
    assert [tuple(int(v) for v in r)[:3] for r in cut] == [(-1, 2, 5), (0, 2, 5)]
    assert SS.model_store(chunks, tau, res, (0, 64, 0), (5, 70, 5))[0].shape == (0,) and SS.model_store({}, tau, res)[1].shape == (0, 7)


def test_inputs_of_the_gpu_tests():
    SS.check_seam_inputs()
    assert len(SS.seam_chunks()) == 7 and SM.ABSENT not in SS.seam_chunks()
    for key, data in SS.far_chunks().items():
        G.check_inputs(data)
        assert len(G.model_box(data.reshape(64, 64, 64), np.asarray(key, dtype=np.int64) * 64, SS.TAU, SS.RES)[0]) > 1000, key
    SS.check_far_inputs()
