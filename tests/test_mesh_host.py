"""The mesh without a GPU: the boundary (symbols, header, ctypes signatures), the numpy model of the surface-nets rules
(tests/mesh_model.py) against a hand-computed literal and on two sphere maps (closed, Euler characteristic 2, volume, distance
to the sphere), holes in the map, and the PLY writer."""
import ctypes as C
import re
import struct

import numpy as np

from mesh_model import sphere_mesh_numbers
import mesh_model as M
from query_model import CTYPE, _declared, _header
NEW = ["ws_map_mesh", "ws_map_mesh_vertices_dev", "ws_map_mesh_faces_dev", "ws_map_mesh_download", "ws_debug_mesh_timing"]


def test_library_exports_and_header_declares_the_mesh_entry_points():
    from warpsense_amd import _lib
    L = _lib.load()
    h = _header()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    assert re.search(r"#define\s+WS_MESH_DEFAULT\s+0u", h) and re.search(r"#define\s+WS_MESH_ANY_WEIGHT\s+1u", h)
    assert (_lib.WS_MESH_DEFAULT, _lib.WS_MESH_ANY_WEIGHT) == (0, 1)
    # the rules are stated where the ABI is declared
    for phrase in ("(2 |va| res + m) / (2 m)", "ascending cell (x, y, z), z fastest", "ascending owner voxel (x, y, z), z fastest, then axis 0, 1, 2",
                   "may be referenced by no face"):
        assert phrase in h, phrase


def test_ctypes_signatures_agree_with_the_header():
    from warpsense_amd import _lib
    L = _lib.load()
    for name in NEW:
        ret, params = _declared(name)
        fn = getattr(L, name)
        want = [CTYPE[p] for p in params]
        assert list(fn.argtypes) == want, (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name  # a pointer must not be cut to the default 32-bit int
        else:
            assert ret == "int" and fn.restype is C.c_int, name


def test_model_reproduces_the_hand_computed_case():
    """3 x 3 x 3 voxels at lo = (0, 0, 0), res 50, all weights 64, value -30 at x = 0 and +20 at x >= 1:
    o = (2 * 30 * 50 + 50) / 100 = 30; four vertices, one quad (owner (0, 1, 1), axis 0), normal +x"""
    import warpsense_amd as W
    value = np.full((3, 3, 3), 20)
    value[0] = -30
    box = W.pack_entry(value.reshape(-1), np.full(27, 64)).astype(np.uint32).reshape(3, 3, 3)
    vert, face = M.model_box(box, (0, 0, 0), 50)
    assert [tuple(int(v[k]) for k in ("x_mm", "y_mm", "z_mm", "weight")) for v in vert] == [(55, 50, 50, 64), (55, 50, 100, 64), (55, 100, 50, 64), (55, 100, 100, 64)]
    assert face.tolist() == [[0, 2, 3], [0, 3, 1]] and face.dtype == np.uint32
    p = np.array([[v["x_mm"], v["y_mm"], v["z_mm"]] for v in vert], dtype=np.int64)
    assert np.cross(p[2] - p[0], p[3] - p[0]).tolist() == [2500, 0, 0]  # normal +x: towards the outside (value > 0)
    # mirrored: outside at x = 0: the other winding
    box2 = W.pack_entry((-value).reshape(-1), np.full(27, 64)).astype(np.uint32).reshape(3, 3, 3)
    vert2, face2 = M.model_box(box2, (0, 0, 0), 50)
    assert face2.tolist() == [[0, 3, 2], [0, 1, 3]] and int(vert2["x_mm"][0]) == 55  # |va| = 30 again: the same crossing
    assert M.model_counts(box) == (4, 2) and M.model_counts(box[:, :, :1]) == (0, 0)
    # |-32768| is 32768; m = 1
    assert (2 * 32768 * 50 + 65535) // (2 * 65535) == 25 and (2 * 0 * 50 + 1) // 2 == 0 and (2 * 1 * 50 + 1) // 2 == 50


def test_sphere_maps_give_closed_meshes_of_the_right_size():
    for edge, centre, radius in M.SPHERES:
        ratio, dist = sphere_mesh_numbers(edge, centre, radius)
        assert abs(ratio - 1.0) < 0.03 and dist < M.RES / 10


def test_holes_in_the_map_never_double_an_edge():
    for edge, centre, radius in M.SPHERES:
        box = M.sphere_box(edge, centre, radius).reshape(-1)
        rng = np.random.default_rng(edge)
        box[rng.random(box.size) < 0.05] &= np.uint32(0xFFFF)  # weight 0
        vert, face = M.model_box(box.reshape((edge,) * 3), M.SPHERE_LO, M.RES)
        rep = M.mesh_report(vert, face)
        assert len(face) > 100 and rep["directed_once"] and not rep["closed"], rep


def _read_ply(path):
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[2])
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["list", "uchar", "int", "vertex_indices"]]
    assert len(body) == 12 * nv + 13 * nf
    return [struct.unpack_from("<fff", body, 12 * i) for i in range(nv)], [struct.unpack_from("<Biii", body, 12 * nv + 13 * i) for i in range(nf)]


def test_ply_writer_round_trips(tmp_path):
    import warpsense_amd as W
    assert W.VERT == M.VERT
    vert = np.array([(55, 50, 50, 64), (-12775, 50, 100, 1), (55, 100, 50, 64), (1, 2, 3, 7)], dtype=W.VERT)
    face = np.array([[0, 2, 3], [0, 3, 1]], dtype=np.uint32)
    assert W.write_mesh_ply(tmp_path / "a.ply", vert, face) == (4, 2)
    v, f = _read_ply(tmp_path / "a.ply")
    f32 = np.float32
    assert v == [tuple(float(f32(c) / f32(1000.0)) for c in (r["x_mm"], r["y_mm"], r["z_mm"])) for r in vert]
    assert f == [(3, 0, 2, 3), (3, 0, 3, 1)]
    assert W.write_mesh_ply(tmp_path / "e.ply", np.empty(0, dtype=W.VERT), np.empty((0, 3), dtype=np.uint32)) == (0, 0)
    assert _read_ply(tmp_path / "e.ply") == ([], [])


def test_committed_seeds_give_meshes_that_are_not_small():
    """the draws of tests/mesh_model.py, checked where no GPU is needed"""
    for size in M.SIZES:
        for which in (0, 1):
            M.check_inputs(M.draw_entries(size, M.seeds_for(size, which)), size)
    for size, seeds in (((21, 17, 13), (5, 1005, 9, 1009)), ((15, 15, 15), (21, 1021))):
        for seed in seeds:
            M.check_inputs(M.draw_entries(size, seed), size)
