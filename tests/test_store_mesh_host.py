"""The mesh of the store without a GPU: the boundary (symbols, header, ctypes signatures), the chunk-assembly helper of
tests/test_gpu_store_mesh.py against a hand-built two-chunk case, the world-order formula of store_mesh.hip against a sort, and the
inputs of the GPU tests (their models' meshes are not small)."""
import ctypes as C
import os
import re

import numpy as np

import mesh_model as M
import query_model as QM
import store_scenes as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ws_store_mesh", "ws_store_mesh_vertices_dev", "ws_store_mesh_faces_dev", "ws_store_mesh_download", "ws_debug_store_mesh_timing"]
CTYPE = dict(QM.CTYPE, **{"ws_store *": C.c_void_p, "const ws_store *": C.c_void_p})


def test_library_exports_and_header_declares_the_store_mesh_entry_points():
    from warpsense_amd import _lib
    L = _lib.load()
    h = QM._header()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    # the semantics are stated where the ABI is declared
    for phrase in ("A voxel of an absent chunk is NOT VALID", "the bounding box of the present chunks", "across chunk borders",
                   "ws_map_mesh on that window and box returns the same bytes", "never the volume of the box"):
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


def test_assemble_on_a_hand_built_two_chunk_case():
    a, b = np.zeros((64, 64, 64), dtype=np.uint32), np.zeros((64, 64, 64), dtype=np.uint32)
    a[63, 2, 5], a[0, 0, 0], b[0, 2, 5], b[63, 63, 63] = 11, 12, 21, 22
    chunks = {(-1, 0, 0): a.reshape(-1), (0, 0, 0): b.reshape(-1)}  # world x -64 .. -1 and 0 .. 63
    lo, hi = SM.bounding_box(chunks)
    assert lo.tolist() == [-64, 0, 0] and hi.tolist() == [63, 63, 63]
    box = SM.assemble(chunks, lo, hi)
    assert box.shape == (128, 64, 64) and box.dtype == np.uint32 and np.count_nonzero(box) == 4
    assert (box[63, 2, 5], box[0, 0, 0], box[64, 2, 5], box[127, 63, 63]) == (11, 12, 21, 22)
    # a box that cuts both chunks and reaches into absent space on every side: zeros there
    cut = SM.assemble(chunks, (-2, -3, 4), (1, 2, 70))
    assert cut.shape == (4, 6, 67) and np.count_nonzero(cut) == 2 and (cut[1, 5, 1], cut[2, 5, 1]) == (11, 21)
    assert not SM.assemble(chunks, (0, 64, 0), (5, 70, 5)).any()
    # ... and the model on it: the two voxels next to the seam make one surface across it
    import warpsense_amd as W
    value = np.full((128, 64, 64), 20)
    value[:64] = -30
    world = W.pack_entry(value.reshape(-1), np.full(value.size, 64)).astype(np.uint32).reshape(value.shape)
    chunks = {(-1, 0, 0): world[:64].reshape(-1), (0, 0, 0): world[64:].reshape(-1)}
    vert, face = SM.model_store(chunks, 50)
    assert len(vert) == 63 * 63 and len(face) == 2 * 62 * 62 and set(vert["x_mm"].tolist()) == {-50 + 25 + 30}
    assert SM.model_store({(0, 0, 0): chunks[(0, 0, 0)]}, 50)[0].shape == (0,) and SM.model_store({}, 50)[1].shape == (0, 3)


def test_world_order_formula_orders_words_like_a_sort():
    rng = np.random.default_rng(3)
    for trial in range(4):
        keys = np.unique(rng.integers(-3, 4, size=(40, 3)), axis=0)  # ascending (cx, cy, cz), like the directory
        assert 20 < len(keys) <= 40
        t = SM.word_index(keys)
        n = len(keys) * 4096
        assert t.shape == (len(keys), 64, 64) and sorted(t.reshape(-1).tolist()) == list(range(n))
        c, lx, ly = np.meshgrid(np.arange(len(keys)), np.arange(64), np.arange(64), indexing="ij")
        x, y, cz = 64 * keys[c, 0] + lx, 64 * keys[c, 1] + ly, keys[c, 2]
        order = np.lexsort((cz.reshape(-1), y.reshape(-1), x.reshape(-1)))  # by world x, then y, then cz
        assert np.array_equal(t.reshape(-1)[order], np.arange(n))
        # the way back of store_mesh.hip (StoreWord::find): no search, two table reads
        B = np.array([np.count_nonzero(keys[:, 0] < k[0]) for k in keys])
        N = np.array([np.count_nonzero(keys[:, 0] == k[0]) for k in keys])
        P = np.array([np.count_nonzero((keys[:, 0] == k[0]) & (keys[:, 1] < k[1])) for k in keys])
        m = np.array([np.count_nonzero((keys[:, 0] == k[0]) & (keys[:, 1] == k[1])) for k in keys])
        tt = t.reshape(-1)
        g = tt >> 12
        u = tt - 4096 * B[g]
        bx = u // (64 * N[g])
        v = u - bx * 64 * N[g]
        h = B[g] + (v >> 6)
        w = v - 64 * P[h]
        by = w // m[h]
        i = B[g] + P[h] + (w - by * m[h])
        assert np.array_equal(i, c.reshape(-1)) and np.array_equal(bx, lx.reshape(-1)) and np.array_equal(by, ly.reshape(-1))


def test_committed_inputs_give_meshes_that_are_not_small():
    SM.check_seam_inputs()
    for key, data in SM.far_chunks().items():
        nv, nf = M.model_counts(data.reshape(64, 64, 64))
        assert nv > 100 and nf > 100, key
