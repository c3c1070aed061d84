"""The ray cast without a GPU: the boundary (symbols, header, ctypes signatures), the numpy model of the rules
(tests/test_gpu_raycast.py) against hand-computed literals and on the sphere maps, the committed draws, the PLY writer and the
pose-to-integers rule of TSDFMapping.raycast."""
import ctypes as C
import re
import struct

import numpy as np

import mesh_model as M
import query_model as QM
import raycast_model as R

NEW = ["ws_map_raycast", "ws_map_raycast_dev", "ws_map_raycast_records_dev", "ws_map_raycast_gradient_dev", "ws_map_raycast_download",
       "ws_debug_raycast_timing"]
FLAGS = {"WS_RAYCAST_DEFAULT": 0, "WS_RAYCAST_ANY_WEIGHT": 1, "WS_RAYCAST_GRADIENT": 2, "WS_RAYCAST_TARGETS": 4}


def test_library_exports_and_header_declares_the_raycast_entry_points():
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
    for phrase in ("b = floor(q / res)", "the trilinear interpolant times res^3, never divided", "L = floor(sqrt(dx^2 + dy^2 + dz^2)) exactly",
                   "p_k = o + trunc(d s_k / L)", "t = s_{k-1} + floor(step T_{k-1} / (T_{k-1} - T_k))", "no hit: 0, 0, 0, -1",
                   "value(g + e_k) - value(g - e_k)", "d_i = point_i - origin"):
        assert phrase in h, phrase


CTYPE = dict(QM.CTYPE)
CTYPE.update({"const int32_t *": C.c_void_p, "int32_t *": C.c_void_p})


def test_ctypes_signatures_agree_with_the_header():
    from warpsense_amd import _lib
    L = _lib.load()
    for name in NEW:
        ret, params = QM._declared(name)
        fn = getattr(L, name)
        want = [CTYPE[p] for p in params]
        assert list(fn.argtypes) == want, (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name
        else:
            assert ret == "int" and fn.restype is C.c_int, name


def _slab(front=20, behind=-30, weight=64):
    """4 x 4 x 4 voxels at lo = (0, 0, 0): value `front` for x <= 1, `behind` for x >= 2"""
    value = np.full((4, 4, 4), front)
    value[2:] = behind
    return value, np.full((4, 4, 4), weight)


def _cast(value, weight, o, d, max_range, **kw):
    import warpsense_amd as W
    box = W.pack_entry(value.reshape(-1), weight.reshape(-1)).astype(np.uint32).reshape(value.shape)
    rec, grad = R.model(R.Ring.of_box(box, (0, 0, 0)), 50, o, np.asarray(d).reshape(-1, 3), max_range, **kw)
    return [tuple(int(r[k]) for k in R.RAY.names) for r in rec], grad.tolist()


def test_model_reproduces_the_hand_computed_case():
    """res 50, h = 25, step 25.  Ray from o = (25, 75, 75) -- the sample point of voxel (0, 1, 1) -- along d = (1, 0, 0), L = 1:
    p_k = (25 + 25 k, 75, 75), q = (25 k, 50, 50), b = (floor(k / 2), 1, 1), f = (25 (k mod 2), 0, 0).  fy = fz = 0 leaves the two
    corners (bx, 1, 1) and (bx + 1, 1, 1): T = (value(bx) (50 - fx) + value(bx + 1) fx) * 50 * 50.
      k = 0: 20 * 50 * 2500 = 2 500 000     k = 1: (20 * 25 + 20 * 25) * 2500 = 2 500 000     k = 2: b = 1, 20 * 50 * 2500 = 2 500 000
      k = 3: b = 1, (20 * 25 - 30 * 25) * 2500 = -625 000: the first crossing from outside to inside
    t = s_2 + floor(25 * 2 500 000 / (2 500 000 + 625 000)) = 50 + floor(62 500 000 / 3 125 000) = 50 + 20 = 70; hit (95, 75, 75) --
    where the line from +20 at x = 75 to -30 at x = 125 passes zero.  Gradient at g = (1, 1, 1): (-30 - 20, 0, 0)."""
    import math
    import warpsense_amd as W
    value, weight = _slab()
    o = (25, 75, 75)
    ring = R.Ring.of_box(W.pack_entry(value.reshape(-1), weight.reshape(-1)).astype(np.uint32).reshape(4, 4, 4), (0, 0, 0))
    for k, want in enumerate([2_500_000, 2_500_000, 2_500_000, -625_000]):
        ok, T = R.field(ring, 50, np.array([[25 + 25 * k, 75, 75]], dtype=np.int64), False)
        assert bool(ok[0]) and int(T[0]) == want, (k, T)
    ok, _ = R.field(ring, 50, np.array([[175, 75, 75]], dtype=np.int64), False)  # k = 6: b = 3, the corner x = 4 is outside the window
    assert not bool(ok[0])
    assert _cast(value, weight, o, (1, 0, 0), 150) == ([(95, 75, 75, 70)], [[-50, 0, 0]])
    assert _cast(value, weight, o, (7, 0, 0), 150) == ([(95, 75, 75, 70)], [[-50, 0, 0]])      # any length
    assert _cast(value, weight, o, (1, 0, 0), 74)[0] == [(0, 0, 0, -1)]                        # K = 2: the crossing is not reached
    assert _cast(value, weight, o, (1, 0, 0), 75)[0] == [(95, 75, 75, 70)]                     # K = 3
    # as targets: d = (125, 75, 75) - o = (100, 0, 0)
    assert _cast(value, weight, o, (125, 75, 75), 150, targets=True) == ([(95, 75, 75, 70)], [[-50, 0, 0]])
    # the mirrored map (inside first): the crossing is from inside to outside, walked past
    assert _cast(-value, weight, o, (1, 0, 0), 150) == ([(0, 0, 0, -1)], [[0, 0, 0]])
    mv, mw = _slab(front=-30, behind=20)
    assert _cast(mv, mw, o, (1, 0, 0), 150)[0] == [(0, 0, 0, -1)]
    # d = 0; a component of 2^30
    assert _cast(value, weight, o, (0, 0, 0), 150) == ([(0, 0, 0, -1)], [[0, 0, 0]])
    assert _cast(value, weight, o, (2 ** 30, 0, 0), 150)[0] == [(0, 0, 0, -1)] and _cast(value, weight, o, (2 ** 30 - 1, 0, 0), 150)[0] == [(95, 75, 75, 70)]
    # a ray that starts outside the window: never inside within its range / the same crossing, four samples later (t = 150 + 20)
    assert _cast(value, weight, (-200, 75, 75), (1, 0, 0), 150)[0] == [(0, 0, 0, -1)]
    assert _cast(value, weight, (-75, 75, 75), (1, 0, 0), 200)[0] == [(95, 75, 75, 170)]
    # a crossing with an invalid corner: voxel (2, 2, 2) is a corner of the cells b = (1, 1, 1) and (2, 1, 1)
    w0 = weight.copy()
    w0[2, 2, 2] = 0
    assert _cast(value, w0, o, (1, 0, 0), 150) == ([(0, 0, 0, -1)], [[0, 0, 0]])
    w0[2, 2, 2] = -5  # observed under the registration's rule only
    assert _cast(value, w0, o, (1, 0, 0), 150)[0] == [(0, 0, 0, -1)]
    assert _cast(value, w0, o, (1, 0, 0), 150, any_weight=True) == ([(95, 75, 75, 70)], [[-50, 0, 0]])
    # the gradient needs its six neighbours: (1, 0, 1) unobserved
    w1 = weight.copy()
    w1[1, 0, 1] = 0
    assert _cast(value, w1, o, (1, 0, 0), 150) == ([(95, 75, 75, 70)], [[0, 0, 0]])
    # integer square root, not sqrtf: 2^30 - 1 on every axis
    big = 2 ** 30 - 1
    assert math.isqrt(3 * big * big) == 1859775391 and R.tdiv(np.array([-7]), np.array([2]))[0] == -3


def test_sphere_maps_hit_where_the_sphere_is():
    """the model on the sphere maps of test_gpu_mesh: seen 1 477 / 1 479 rays within 0.8 R, all of them hit; largest distance of a
    hit to the sphere 2.7 / 1.8 mm, largest range error of the 0.8 R rays 4.02 / 3.50 mm (bound: res / 10 = 5 mm)"""
    seen = []
    for edge, centre, radius in M.SPHERES:
        box = M.sphere_box(edge, centre, radius).reshape((edge,) * 3)
        o, d, c_mm = R.sphere_rays(centre, radius)
        rec, grad = R.model(R.Ring.of_box(box, M.SPHERE_LO), R.RES, o, d, 4000)
        seen.append(R.check_sphere(rec, o, d, c_mm, radius * R.RES)[0])
        rec_t, grad_t = R.model(R.Ring.of_box(box, M.SPHERE_LO), R.RES, o, o + d, 4000, targets=True)
        assert R.same((rec_t, grad_t), (rec, grad))
    assert seen == [1477, 1479]


def test_committed_seeds_give_ray_casts_that_are_not_small():
    """a condition on the INPUTS of tests/test_gpu_raycast.py: the model hits on more than 500 rays under either weight rule"""
    counts = []
    for size, seed in R.RANDOM_MAPS:
        box = M.draw_entries(size, seed).reshape(size)
        o, d = R.random_rays(size, seed)
        for any_weight in (False, True):
            rec, grad = R.model(R.Ring.of_box(box, R.RANDOM_LO), R.RES, o, d, 3000, any_weight)
            n = int(np.count_nonzero(rec["range_mm"] >= 0))
            assert n > 500 and np.count_nonzero(np.any(grad != 0, axis=1)) > 100, (size, any_weight, n)
            counts.append(n)
    assert counts == [1018, 1525, 1659, 1983]
    for size in R.SIZES:
        for which in (0, 1):
            box = M.draw_entries(size, M.seeds_for(size, which)).reshape(size)
            lo = -(np.asarray(size) // 2)
            o, d = R.random_rays(size, seed=sum(size), lo=lo)
            for any_weight in (False, True):
                rec, _ = R.model(R.Ring.of_box(box, lo), R.RES, o, d, 3000, any_weight)
                assert np.count_nonzero(rec["range_mm"] >= 0) > 100, (size, which, any_weight)


def _read_ply(path, names):
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    assert [l.split()[1:] for l in lines if l.startswith("property")] == [["float", n] for n in names]
    assert len(body) == 4 * len(names) * nv
    return [struct.unpack_from("<" + "f" * len(names), body, 4 * len(names) * i) for i in range(nv)]


def test_ply_writer_round_trips(tmp_path):
    import warpsense_amd as W
    assert W.RAY == R.RAY
    rec = np.array([(95, 75, 75, 70), (0, 0, 0, -1), (-12775, 50, 100, 1), (1, 2, 3, 0)], dtype=W.RAY)
    grad = np.array([[-50, 0, 0], [9, 9, 9], [3, -4, 0], [0, 0, 0]], dtype=np.int32)
    f32 = np.float32
    xyz = [tuple(float(f32(c) / f32(1000.0)) for c in (r["x_mm"], r["y_mm"], r["z_mm"])) for r in rec[[0, 2, 3]]]
    assert W.write_raycast_ply(tmp_path / "a.ply", rec) == 3
    assert _read_ply(tmp_path / "a.ply", ["x", "y", "z"]) == xyz
    assert W.write_raycast_ply(tmp_path / "b.ply", rec, grad) == 3
    normals = [(-1.0, 0.0, 0.0), (float(f32(0.6)), float(f32(-0.8)), 0.0), (0.0, 0.0, 0.0)]
    assert _read_ply(tmp_path / "b.ply", ["x", "y", "z", "nx", "ny", "nz"]) == [p + n for p, n in zip(xyz, normals)]
    assert W.write_raycast_ply(tmp_path / "e.ply", np.empty(0, dtype=W.RAY), np.empty((0, 3), dtype=np.int32)) == 0
    assert _read_ply(tmp_path / "e.ply", ["x", "y", "z", "nx", "ny", "nz"]) == []


def test_pose_to_integers_rule():
    import warpsense_amd as W
    # identity rotation: the longest component becomes 2^20, the others keep their ratio; a zero direction stays zero
    pose = np.eye(4)
    pose[:3, 3] = (0.0625, -0.1875, 10.0)
    o, d = W.TSDFMapping.raycast_rays(pose, [[1.0, 0.5, -0.25], [0.0, -3.0, 1.0], [0.0, 0.0, 0.0]])
    assert o.dtype == np.int32 and d.dtype == np.int32
    assert o.tolist() == [62, -188, 10000]  # 62.5 and -187.5 are ties: to the even neighbour
    assert d.tolist() == [[1048576, 524288, -262144], [0, -1048576, 349525], [0, 0, 0]]
    # a quarter turn about z: sensor x goes to map y, sensor y to map -x
    pose = np.array([[0.0, -1.0, 0.0, -2.0], [1.0, 0.0, 0.0, 0.0254], [0.0, 0.0, 1.0, 0.3], [0.0, 0.0, 0.0, 1.0]])
    o, d = W.TSDFMapping.raycast_rays(pose, [[2.0, 0.0, 1.0], [1.0, 4.0, 0.0]])
    assert o.tolist() == [-2000, 25, 300]
    assert d.tolist() == [[0, 1048576, 524288], [-1048576, 262144, 0]]
    assert np.allclose(np.linalg.norm(W.synthetic.os1_128_dirs(), axis=1), 1.0) and W.synthetic.os1_128_dirs().shape == (131072, 3)
