"""The surface cloud without a GPU: the boundary (symbols, header, ctypes signatures), the numpy model of publish_local_map
(tests/surface_model.py) against a hand-written literal of the reference's KAT map, the skeleton arithmetic against
hand-computed windows, and the PLY writer."""
import ctypes as C
import re
import struct

import numpy as np

from query_model import _declared, _header
import query_model as QM
import surface_model as G

NEW = ["ws_map_surface", "ws_map_surface_records_dev", "ws_map_surface_marker_dev", "ws_map_surface_download", "ws_debug_surface_timing"]


def test_library_exports_and_header_declares_the_surface_entry_points():
    from warpsense_amd import _lib
    L = _lib.load()
    h = _header()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    assert re.search(r"#define\s+WS_SURFACE_RECORDS\s+0u", h) and re.search(r"#define\s+WS_SURFACE_MARKER\s+1u", h)
    assert (_lib.WS_SURFACE_RECORDS, _lib.WS_SURFACE_MARKER) == (0, 1)
    assert "7 float32 per record" in h  # the marker layout is stated where the ABI is declared


CTYPE = {"ws_map *": C.c_void_p, "const ws_map *": C.c_void_p, "int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "size_t": C.c_size_t,
         "const int32_t [3]": C.c_void_p, "float [3]": C.c_void_p, "void *": C.c_void_p, "float *": C.c_void_p, "size_t *": C.POINTER(C.c_size_t)}


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


def test_model_reproduces_the_reference_kat_map():
    """test/map.cpp:9-90 (tsdf_write): tau = 3000, map_resolution = 1000, one ray along x; the voxels (1..8, 0, 0) hold the values
    3000, 3000, 2000, 1000, 0, -1000, -2000, 3000 (:51-89) with weight calc_weight(value) > 0 for the first seven and 0 for the last
    (the default entry).  By map.h:45 the voxels with abs(value) < 3000 qualify: x = 3..7; colours by map.h:55-64."""
    tau, res = 3000, 1000
    eps = tau // 10

    def calc_weight(v):  # update_tsdf.cu:90-94 / cpu/update_tsdf.h
        return 64 if v >= -eps else 64 * (tau + v) // (tau - eps)
    values = [3000, 3000, 2000, 1000, 0, -1000, -2000, 3000]
    weights = [calc_weight(v) for v in values[:7]] + [0]
    assert weights == [64, 64, 64, 64, 64, 47, 23, 0]
    size, pos, off = (21, 21, 21), (0, 0, 0), (10, 10, 10)
    data = np.full(21 ** 3, (tau & 0xFFFF), dtype=np.uint32)  # (tau, 0)
    for x, (v, w) in zip(range(1, 9), zip(values, weights)):
        idx = (((x + 10) % 21) * 21 + 10) * 21 + 10
        data[idx] = (v & 0xFFFF) | (w << 16)

    class Host:
        size_, pos_, offset_, data_ = np.array(size), np.array(pos), np.array(off), data
    rec, mk = G.model(Host, tau, res)
    f = np.float32
    assert [tuple(int(v) for v in (r["x"], r["y"], r["z"])) for r in rec] == [(3, 0, 0), (4, 0, 0), (5, 0, 0), (6, 0, 0), (7, 0, 0)]
    assert [int(r["raw"]) for r in rec] == [2000 | (64 << 16), 1000 | (64 << 16), 0 | (64 << 16), (-1000 & 0xFFFF) | (47 << 16), (-2000 & 0xFFFF) | (23 << 16)]
    want = np.array([[3, 0, 0, f(2000) / f(3000), 0, 0, 1],
                     [4, 0, 0, f(1000) / f(3000), 0, 0, 1],
                     [5, 0, 0, 0, 0, 0, 1],
                     [6, 0, 0, 0, f(1000) / f(3000), 0, 1],
                     [7, 0, 0, 0, f(2000) / f(3000), 0, 1]], dtype=np.float32)  # x * 1000 / 1000.f = x metres
    assert QM.same(mk, want)
    # a narrower band keeps |value| < 1500 only
    rec2, _ = G.model(Host, tau, res, band=1500)
    assert [int(r["x"]) for r in rec2] == [4, 5, 6]


def test_skeleton_end_points_for_two_hand_computed_windows():
    # 513^3 @ 50 mm around the origin: corners -256 * 0.05 = -12.8 -> -12, 256 * 0.05 = 12.8 -> 12; dims 24
    sk = G.skeleton_model((513, 513, 513), (0, 0, 0), 50)
    assert sk.shape == (24, 3)
    lo, hi = -12.0, 12.0
    want = [[lo, lo, lo], [hi, lo, lo], [hi, lo, lo], [hi, hi, lo], [hi, hi, lo], [lo, hi, lo], [lo, hi, lo], [lo, lo, lo],
            [lo, lo, hi], [hi, lo, hi], [hi, lo, hi], [hi, hi, hi], [hi, hi, hi], [lo, hi, hi], [lo, hi, hi], [lo, lo, hi],
            [hi, hi, hi], [hi, hi, lo], [lo, lo, lo], [lo, lo, hi], [lo, hi, hi], [lo, hi, lo], [hi, lo, lo], [hi, lo, hi]]
    assert np.array_equal(sk, np.array(want))
    # negative pos, 64 mm: size (101, 51, 21), pos (-230, 17, -4): corners (-280, -8, -14) and (-180, 42, 6) voxels, times 0.064f:
    # -17.92 -> -17, -0.512 -> 0, -0.896 -> 0 (truncation toward zero, not floor) and -11.52 -> -11, 2.688 -> 2, 0.384 -> 0
    sk = G.skeleton_model((101, 51, 21), (-230, 17, -4), 64)
    assert sk[0].tolist() == [-17.0, 0.0, 0.0] and sk[16].tolist() == [-11.0, 2.0, 0.0]
    assert sk[1].tolist() == [-11.0, 0.0, 0.0] and sk[3].tolist() == [-11.0, 2.0, 0.0]  # dims = (6, 2, 0)
    assert np.array_equal(sk[:8], sk[8:16])  # a flat box: dims[2] == 0


def _read_ply(path):
    """a minimal reader: the header's element count and properties, then the packed little-endian vertices"""
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    rows = [struct.unpack_from("<fffBBB", body, 15 * i) for i in range(n)]
    assert len(body) == 15 * n
    return rows


def test_ply_writer_round_trips(tmp_path):
    import warpsense_amd as W
    f = np.float32
    mk = np.array([[0.05, -1.25, 3.0, 0.5, 0, 0, 1], [12.8, 0, -0.05, 0, f(999) / f(1000), 0, 1], [1, 2, 3, 0, 0, 0, 1]], dtype=np.float32)
    assert W.write_surface_ply(tmp_path / "a.ply", mk) == 3
    rows = _read_ply(tmp_path / "a.ply")
    assert [r[:3] for r in rows] == [tuple(float(v) for v in m[:3]) for m in mk]
    assert [r[3:] for r in rows] == [(127, 0, 0), (0, 254, 0), (0, 0, 0)]
    assert W.write_surface_ply(tmp_path / "empty.ply", np.zeros((0, 7), dtype=np.float32)) == 0 and _read_ply(tmp_path / "empty.ply") == []


def test_committed_seeds_give_well_populated_inputs():
    """the draws of tests/surface_model.py, checked where no GPU is needed: planted categories present, share in [0.10, 0.40]"""
    for size in G.SIZES:
        n = int(np.prod(size))
        for which in (0, 1):
            G.check_inputs(G.draw_entries(n, seed=sum(size) + 1000 * which))
    for n, seeds in ((21 * 17 * 13, (5, 1005, 9, 1009)), (15 ** 3, (21, 1021, 31, 1031)), (16 * 18 * 20, (77,))):
        for seed in seeds:
            G.check_inputs(G.draw_entries(n, seed))
