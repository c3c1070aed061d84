"""CPU tests that PIN the oracle (oracle/ws_oracle.c) — no GPU needed.

1. the reference's own known-answer tests for this path,
2. golden vectors produced by the reference's own headers -- since round 4 also cu_avg_tsdf_krnl's body through TSDFEntry's
   accessors and calc_jacobis_krnl's lookups through cuda::DeviceMap / Vector3::cross -- (oracle/_ref -> tests/golden/ref_headers.npz,
   generator: tests/golden/make_ref_goldens.py), and — where /root/reference is present — oracle/_ref live,
3. the whole-scan counters the survey recorded from the reference kernel source.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from warpsense_amd import synthetic as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_headers.npz")
GOLD_INDEX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_get_index.npz")


def calc_weight(value, tau, weight_epsilon):
    """include/warpsense/test/common.h:16-26"""
    w = 64
    if value < -weight_epsilon:
        w = int(64 * (tau + value) / (tau - weight_epsilon))
    return w


# ------------------------------------------------------------------ 0. hand-derived vectors
# The reference's own tests pin the accept rule only for weight-0 entries and the integrate / Jacobian kernels not at all
# (SURVEY §8c).  The vectors below are worked out BY HAND from the cited reference lines -- a second, independent reading of
# the same source, not an execution of it (the .cu files cannot be built here): they catch a slip in the C restatement, they
# do not replace a reference run.
def _accept(old, new):
    """include/warpsense/cuda/util.h:74-78 for one thread: the stored entry survives iff |old.value| < |new.value| or
    old.weight > 0; otherwise the new entry is written (ties on |value| replace)."""
    (ov, ow), (nv, nw) = old, new
    return old if (abs(ov) < abs(nv) or ow > 0) else new


def test_hand_accept_rule_truth_table():
    L = O.lib()
    vals = (-1000, -300, -1, 0, 1, 300, 1000)
    weights = (-64, -10, 0, 10, 64)
    cell = (C.c_uint32 * 1)()
    n = 0
    for ov in vals:
        for ow in weights:
            for nv in vals:
                for nw in weights:
                    cell[0] = int(O.pack(ov, ow))
                    L.wso_tsdf_min(cell, int(O.pack(nv, nw)))
                    assert tuple(int(t) for t in O.unpack(cell[0])) == _accept((ov, ow), (nv, nw)), ((ov, ow), (nv, nw))
                    n += 1
    assert n == 35 * 35
    # a sequence: negative-weight candidates fold to the smallest |value| (latest on ties) until a positive weight freezes the voxel
    cell[0] = int(O.pack(1000, 0))
    for v, w in ((-400, -64), (250, -30), (-250, -20), (600, 64), (100, 64), (-50, -64)):
        L.wso_tsdf_min(cell, int(O.pack(v, w)))
    # (-400,-64) -> (250,-30) -> (-250,-20) [tie replaces] -> (600, 64) rejected (600 > 250) -> (100, 64) accepted, frozen
    assert tuple(int(t) for t in O.unpack(cell[0])) == (100, 64)


@pytest.mark.parametrize("existing,fresh,want", [
    ((10, 3), (-7, 2), (3, 5)),          # both weights > 0: (10*3 + -7*2) / 5 = 16 / 5 -> 3 (update_tsdf.cu:25-28)
    ((-10, 3), (3, 2), (-4, 5)),         # (-30 + 6) / 5 = -24 / 5 -> -4: C division truncates toward zero
    ((200, 600), (100, 64), (190, 640)),  # (120000 + 6400) / 664 = 190; weight min(max_weight = 640, 664)
    ((1000, 0), (-120, -47), (-120, -47)),  # first write (existing weight <= 0) copies negative weights too (:31-35)
    ((77, -5), (40, 64), (40, 64)),      # existing weight < 0, new positive: overwritten
    ((77, -5), (40, -9), (40, -9)),      # existing weight < 0, new negative: overwritten
    ((77, 12), (40, -9), (77, 12)),      # existing observed, new weight negative: neither branch -> unchanged
    ((77, 12), (40, 0), (77, 12)),       # new weight 0: unchanged
    ((77, 0), (40, 0), (77, 0)),         # both unobserved: unchanged
])
def test_hand_integrate_rule(existing, fresh, want):
    """cu_avg_tsdf_krnl, src/warpsense/cuda/update_tsdf.cu:13-43: int arithmetic, then new_map is reset to (tau, 0)."""
    tau = 1000
    avg = np.array([O.pack(*existing)], dtype=np.uint32)
    new = np.array([O.pack(*fresh)], dtype=np.uint32)
    O.lib().wso_update_avg(O._p(new), O._p(avg), 1, 640, tau)
    assert tuple(int(t) for t in O.unpack(avg[0])) == want
    assert tuple(int(t) for t in O.unpack(new[0])) == (tau, 0)


def test_hand_calc_jacobis_vector():
    """calc_jacobis_krnl, src/warpsense/cuda/registration.cu:194-257, for one point in a 7^3 map at 50 mm: voxel (1, 0, -1)
    holds (120, w 5); x neighbours (200 | 100) -> gradient.x = 50; y neighbours (50 | 30) -> 10; z_next unobserved -> 0;
    then with y_last = -30 (strictly opposite signs) -> gradient.y = 0.  J = (point x gradient, gradient) with the point taken
    relative to the (int) translation of the transform."""
    om = O.OracleMap((7, 7, 7), 1000, 0)
    om.set_entry(1, 0, -1, 120, 5)
    om.set_entry(2, 0, -1, 200, 1)
    om.set_entry(0, 0, -1, 100, 1)
    om.set_entry(1, 1, -1, 50, 1)
    om.set_entry(1, -1, -1, 30, 1)
    om.set_entry(1, 0, 0, 80, 0)     # z_next: weight 0 -> no z gradient
    om.set_entry(1, 0, -2, 60, 1)
    p = np.array([[70, 10, -60]], dtype=np.int32)  # / 50 -> (1, 0, -1) (C truncation: -60 / 50 = -1)
    J, vals, mask = O.calc_jacobis(om, np.eye(4, dtype=np.float32), p, 50)
    # gradient (50, 10, 0); cross = (qy*gz - qz*gy, qz*gx - qx*gz, qx*gy - qy*gx) = (600, -3000, 700 - 500)
    assert mask[0] == 1 and vals[0] == 120 and J[0].tolist() == [600, -3000, 200, 50, 10, 0]
    # a pure translation by (100, 0, 0): the transformed point is (70, 10, -60) again for p = (-30, 10, -60), and the
    # Jacobian uses point - center = (-30, 10, -60): cross.z = -30*10 - 10*50 = -800
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = 100.0
    J, vals, mask = O.calc_jacobis(om, T, np.array([[-30, 10, -60]], dtype=np.int32), 50)
    assert mask[0] == 1 and vals[0] == 120 and J[0].tolist() == [600, -3000, -800, 50, 10, 0]
    # strictly opposite signs across the voxel: no gradient on that axis (registration.cu:239-242)
    om.set_entry(1, -1, -1, -30, 1)
    J, vals, mask = O.calc_jacobis(om, np.eye(4, dtype=np.float32), p, 50)
    assert J[0].tolist() == [0, -3000, -500, 50, 0, 0]
    # a zero on one side is not "opposite": (50 - 0) / 2 = 25
    om.set_entry(1, -1, -1, 0, 1)
    J, _, _ = O.calc_jacobis(om, np.eye(4, dtype=np.float32), p, 50)
    assert J[0].tolist()[3:] == [50, 25, 0]
    # unobserved centre voxel, and a voxel on the border (in_bounds_with_buffer_neg(buf, 1), :217): no correspondence
    om.set_entry(1, 0, -1, 120, 0)
    assert O.calc_jacobis(om, np.eye(4, dtype=np.float32), p, 50)[2][0] == 0
    om.set_entry(3, 0, 0, 120, 5)
    assert O.calc_jacobis(om, np.eye(4, dtype=np.float32), np.array([[160, 10, 10]], dtype=np.int32), 50)[2][0] == 0


# ------------------------------------------------------------------ 1. reference KATs
def test_kat_tsdf_write_cuda_semantics():
    """test/map.cpp:9-90 and test/cuda.cpp:268-414: point (5500,500,500), res 1000, tau 3000, 21^3 map."""
    tau, res, mw = 3000, 1000, 10 * 64
    avg = O.OracleMap((20, 20, 20), tau, 0)
    new = avg.copy()
    assert list(avg.size) == [21, 21, 21] and list(avg.offset) == [10, 10, 10] and list(avg.pos) == [0, 0, 0]  # test/test.cu:63-126
    pos, up = O.convert_pose(np.eye(4), res)
    assert list(pos) == [0, 0, 0] and list(up) == [0, 0, 32768]
    st = O.update_tsdf(avg, new, np.array([[5500, 500, 500]], dtype=np.int32), pos, up, tau, mw, res)
    expect = [3000, 3000, 2000, 1000, 0, -1000, -2000]
    for x, v in zip(range(1, 8), expect):
        val, w = avg.entry(x, 0, 0)
        assert val == v and w == calc_weight(v, tau, tau // 10), (x, val, w)
    assert [avg.entry(x, 0, 0)[1] for x in range(1, 8)] == [64, 64, 64, 64, 64, 47, 23]
    assert avg.entry(8, 0, 0) == (3000, 0)
    assert st.write_calls == 7 and int((avg.data != O.pack(tau, 0)).sum()) == 7
    assert np.all(new.data == O.pack(tau, 0))


def test_kat_tsdf_write_cpu_port():
    """the same KAT through the CPU-baseline port (the reference runs it on src/cpu/update_tsdf.cpp:397-564)."""
    tau, res, mw = 3000, 1000, 640
    for threads in (1, 2):
        m = O.OracleMap((20, 20, 20), tau, 0)
        O.cpu_update_tsdf(m, np.array([[5500, 500, 500]], dtype=np.int32), [0, 0, 0], [0, 0, 32768], tau, mw, res, threads)
        assert [m.entry(x, 0, 0) for x in range(1, 9)] == [(3000, 64), (3000, 64), (2000, 64), (1000, 64), (0, 64),
                                                           (-1000, 47), (-2000, 23), (3000, 0)]


def test_kat_map_bounds():
    """test/cuda.cpp:28-105 / test/map.cpp:240-300: 5^3 map, default (4, 6)."""
    m = O.OracleMap((5, 5, 5), 4, 6)
    assert list(m.size) == [5, 5, 5] and list(m.offset) == [2, 2, 2]
    for (x, y, z), (v, w) in {(-2, 2, 0): (0, 0), (-1, 2, 0): (1, 1), (-2, 1, 0): (2, 1), (-1, 1, 0): (3, 2),
                              (-2, 0, 0): (4, 3), (-1, 0, 0): (5, 5)}.items():
        m.set_entry(x, y, z, v, w)
    assert m.in_bounds(0, 2, -2) and not m.in_bounds(22, 0, 0)
    assert m.entry(0, 0, 0) == (4, 6) and m.entry(-1, 2, 0) == (1, 1)
    # shifted window of test/map.cpp:303-309: pos (24,0,0), offset (26 % 5, 2, 2)
    s = O.OracleMap((5, 5, 5), 4, 6, pos=(24, 0, 0), offset=(26 % 5, 2, 2))
    assert not s.in_bounds(0, 2, -2) and s.in_bounds(22, 0, 0)
    seen = {s.index(x, y, z) for x in range(22, 27) for y in range(-2, 3) for z in range(-2, 3)}
    assert seen == set(range(125))  # the ring mapping is a bijection onto the storage


def test_kat_ring_buffer_shift():
    """test/map.cpp:240-365 (map_raw) on the host LocalMap mirror: offsets after shifts, values survive unload/reload."""
    import warpsense_amd as W
    lm = W.LocalMap(5, 5, 5, 4, 6)
    for (x, y, z), (v, w) in {(-2, 2, 0): (0, 0), (-1, 2, 0): (1, 1), (-2, 1, 0): (2, 1), (-1, 1, 0): (3, 2),
                              (-2, 0, 0): (4, 3), (-1, 0, 0): (5, 5)}.items():
        lm.set_value(x, y, z, v, w)
    for x in (5, 10, 15, 20, 24):
        lm.shift((x, 0, 0))
    assert list(lm.pos) == [24, 0, 0] and list(lm.offset) == [26 % 5, 2, 2]
    assert not lm.in_bounds(0, 2, -2) and lm.in_bounds(22, 0, 0) and lm.value(24, 0, 0) == (4, 6)
    lm.set_value(24, 0, 0, 24, 0)
    lm.shift((24, 5, 0)); lm.set_value(24, 5, 0, 24, 5)
    lm.shift((19, 5, 0)); lm.set_value(19, 5, 0, 19, 5)
    lm.shift((19, 0, 0)); lm.set_value(19, 0, 0, 19, 0)
    lm.shift((24, 0, 0)); assert lm.value(24, 0, 0) == (24, 0)
    lm.shift((19, 0, 0)); assert lm.value(19, 0, 0) == (19, 0)
    lm.shift((24, 5, 0)); assert lm.value(24, 5, 0) == (24, 5)
    lm.shift((19, 5, 0)); assert lm.value(19, 5, 0) == (19, 5)
    lm.shift((24, 0, 0)); assert lm.value(24, 0, 0) == (24, 0)
    for x in (19, 14, 9, 4, 0):
        lm.shift((x, 0, 0))
    assert list(lm.pos) == [0, 0, 0] and list(lm.offset) == [2, 2, 2]
    assert lm.value(0, 0, 0) == (4, 6) and lm.value(-1, 2, 0) == (1, 1)
    # the oracle's index math agrees with the mirror after shifting
    om = O.OracleMap((5, 5, 5), 4, 6, pos=lm.pos, offset=lm.offset, data=lm.data.copy())
    assert om.entry(-1, 2, 0) == (1, 1)


def test_kat_atomic_tsdf_min():
    """test/cuda.cpp:968-990: 100 000 entries (v, 0), v in [1, 1000] -> the minimum value survives."""
    rng = np.random.default_rng(3)
    vals = rng.integers(1, 1001, 100_000).astype(np.int16)
    cell = (C.c_uint32 * 1)(int(O.pack(32767, 0)))
    L = O.lib()
    for v in vals:
        L.wso_tsdf_min(cell, int(O.pack(int(v), 0)))
    assert O.unpack(cell[0])[0] == vals.min()
    # a positive weight freezes the voxel (cuda/util.h:74-78)
    cell[0] = int(O.pack(500, 64))
    assert L.wso_tsdf_min(cell, int(O.pack(1, 64))) == 0 and O.unpack(cell[0]) == (500, 64)
    # ties are replaced (|new| <= |old|), sign of the value is ignored by the comparison
    cell[0] = int(O.pack(-300, -64))
    assert L.wso_tsdf_min(cell, int(O.pack(300, -10))) == 1 and O.unpack(cell[0]) == (300, -10)


@pytest.mark.parametrize("J", [[0, 1, 2, 3, 4, 5], [-1, 1, 2, 3, 4, -5], [0, 1, -2, 12, 4, 5], [0, -1, 20, 3, -4, 5]])
def test_kat_jacobi_outer_product(J):
    """test/cuda.cpp:837-923: h == J J^T for the four vectors."""
    jac = np.array([J], dtype=np.int64)
    vals = np.array([7], dtype=np.int16)
    mask = np.array([1], dtype=np.uint8)
    h = np.zeros(36, dtype=np.int64)
    g = np.zeros(6, dtype=np.int64)
    e, c = C.c_int32(0), C.c_int32(0)
    O.lib().wso_reduce(O._p(jac), O._p(vals), O._p(mask), 1, O._p(h), O._p(g), C.byref(e), C.byref(c), 0)
    Jv = np.array(J, dtype=np.int64)
    assert np.array_equal(h.reshape(6, 6).T, np.outer(Jv, Jv))
    assert np.array_equal(g, Jv * 7) and e.value == 7 and c.value == 1


def test_kat_transform_point():
    """test/cuda.cpp:760-827: (1,0,0) rotated by +-90 deg about z -> (0,+-1,0) in fixed point."""
    for theta, want in ((np.pi / 2, (0, 1, 0)), (-np.pi / 2, (0, -1, 0))):
        T = np.eye(4, dtype=np.float32)
        T[0, 0] = np.cos(np.float32(theta)); T[0, 1] = -np.sin(np.float32(theta))
        T[1, 0] = np.sin(np.float32(theta)); T[1, 1] = np.cos(np.float32(theta))
        M = np.zeros(16, dtype=np.int32)
        O.lib().wso_to_int_mat(O._p(O.colmajor(T)), O._p(M))
        out = np.zeros(3, dtype=np.int32)
        O.lib().wso_transform_point(O._p(np.array([1, 0, 0], dtype=np.int32)), O._p(M), O._p(out))
        assert tuple(out) == want


def test_kat_data_sizes_and_consts():
    """test/test.cu:48-61, include/warpsense/consts.h."""
    g = np.load(GOLD)
    assert list(g["consts"]) == [32768, 64, 4, 8]
    assert O.lib().wso_dz_per_distance() == 100


# ------------------------------------------------------------------ 2. golden vectors from the reference headers
def _check_against(get_index, in_bounds, in_pos, in_neg, l2i, l2l, cross, ray_setup, pack):
    g = np.load(GOLD)
    for m, q, r in zip(g["ring_maps"], g["ring_queries"], g["ring_results"]):
        om = O.OracleMap(m[0:3], 0, 0, pos=m[3:6], offset=m[6:9])
        v = om.view()
        x, y, z = (int(t) for t in q)
        inb, idx, ipos, ineg, buf = (int(t) for t in r)
        assert bool(O.lib().wso_in_bounds(C.byref(v), x, y, z)) == bool(inb)
        if inb:
            assert O.lib().wso_get_index(C.byref(v), x, y, z) == idx
        assert bool(O.lib().wso_in_bounds_with_buffer_pos(C.byref(v), x, y, z, buf)) == bool(ipos)
        assert bool(O.lib().wso_in_bounds_with_buffer_neg(C.byref(v), x, y, z, buf)) == bool(ineg)
    L = O.lib()
    L.wso_l2norm_i.restype = C.c_int32
    L.wso_l2norm_l.restype = C.c_int64
    L.wso_l2norm_l.argtypes = [C.c_int64] * 3
    # Where the int sum of squares wraps to a negative number sqrtf gives NaN and float->int is undefined in C++: the
    # host build of the reference header (the golden) shows x86's INT_MIN, the reference's CUDA device code gives 0
    # (cvt.rzi of NaN), and so does gfx950.  The oracle restates the device: 0 there, the golden everywhere else.
    got = np.array([L.wso_l2norm_i(int(a), int(b), int(c)) for a, b, c in g["l2_in"]])
    v = g["l2_in"].astype(np.int64)
    wrapped = (((v * v).sum(axis=1) + 2 ** 31) % 2 ** 32) - 2 ** 31
    nan = wrapped < 0
    assert nan.sum() > 0 and np.all(g["l2_i"][nan] == -2 ** 31) and np.all(got[nan] == 0)
    assert np.array_equal(got[~nan], g["l2_i"][~nan])
    # 64-bit: CUDA's cvt.rzi.s64.f32 (__float2ll_rz) gives 0x8000000000000000 for NaN -- the value x86 gives too, so the
    # golden of the host-built header holds for every vector, the wrapped ones included
    got_l = np.array([L.wso_l2norm_l(int(a), int(b), int(c)) for a, b, c in g["l2l_in"]])
    assert (g["l2_l"] == -2 ** 63).sum() > 0
    assert np.array_equal(got_l, g["l2_l"])
    out = np.zeros(3, dtype=np.int32)
    for a, b, want in zip(g["cross_a"], g["cross_b"], g["cross_out"]):
        L.wso_cross_i(O._p(np.ascontiguousarray(a)), O._p(np.ascontiguousarray(b)), O._p(out))
        assert np.array_equal(out, want)
    iv = np.zeros(3, dtype=np.int64)
    for p, pos, up, dist, want_iv, rc in zip(g["ray_points"], g["ray_pos"], g["ray_up"], g["ray_distance"], g["ray_interp"], g["ray_rc"]):
        d = C.c_int32(0)
        got = L.wso_ray_setup(O._p(np.ascontiguousarray(p)), O._p(np.ascontiguousarray(pos)), O._p(np.ascontiguousarray(up)),
                              C.byref(d), O._p(iv))
        assert got == rc and d.value == dist
        if rc == 0:
            assert np.array_equal(iv, want_iv)
    assert np.array_equal(O.pack(g["entry_vw"][:, 0], g["entry_vw"][:, 1]), g["entry_raw"])
    # at(i,j) = 10 i + j written through the reference accessors: storage must be column-major
    assert np.array_equal(g["m4_layout"].reshape(4, 4).T, np.add.outer(10 * np.arange(4), np.arange(4)))
    assert np.array_equal(g["m6_layout"].reshape(6, 6).T, np.add.outer(10 * np.arange(6), np.arange(6)))


def test_golden_reference_headers():
    _check_against(*[None] * 9)


def test_golden_integrate_through_the_reference_accessors():
    """cu_avg_tsdf_krnl's per-voxel body (update_tsdf.cu:19-41) evaluated with the reference's own TSDFEntry accessors
    (oracle/ref_driver.cpp: ref_integrate_entry) on 12 000 entry pairs -- int16 wrap of the stored average and of the weight
    sum, negative and zero weights on either side, the default entry -- against wso_update_avg (until round 4
    this kernel was pinned by hand-derived vectors only)."""
    g = np.load(GOLD)
    mw, tau = (int(x) for x in g["avg_params"])
    avg = g["avg_existing"].copy()
    new = g["avg_fresh"].copy()
    O.lib().wso_update_avg(new.ctypes.data_as(C.c_void_p), avg.ctypes.data_as(C.c_void_p), avg.size, mw, tau)
    bad = np.nonzero(avg != g["avg_existing_out"])[0]
    assert bad.size == 0, f"{bad.size} entries differ, first: existing {g['avg_existing'][bad[0]]:#x} fresh {g['avg_fresh'][bad[0]]:#x}"
    assert np.array_equal(new, g["avg_fresh_out"])
    # the cases the fixture is there for are in it
    ew = (g["avg_existing"] >> 16).astype(np.int16).astype(np.int32)
    nw = (g["avg_fresh"] >> 16).astype(np.int16).astype(np.int32)
    assert ((ew > 0) & (nw > 0)).sum() > 2000 and ((nw != 0) & (ew <= 0)).sum() > 1000 and (nw == 0).sum() > 500 and (nw < 0).sum() > 1000
    assert ((ew > 0) & (nw > 0) & (ew + nw > 32767)).sum() > 10  # the weight sum leaves int16 before the clamp


def test_golden_jacobians_through_the_reference_types():
    """calc_jacobis_krnl's map half (registration.cu:217-253) -- bounds test with the buffer, the seven lookups, the gradient
    rule, the cross product -- evaluated through cuda::DeviceMap::value_unchecked / in_bounds_with_buffer_neg and
    rmagine::Vector3::cross of the reference (oracle/ref_driver.cpp: ref_jacobi) on 24 maps of random entries x 500 points, ring
    buffer offsets and window positions included, against wso_calc_jacobis driven with the pure integer translation that makes
    the kernel's fixed-point transform exact (the transform itself: reference KAT test/cuda.cpp:760-827)."""
    g = np.load(GOLD)
    n_masked = 0
    for case, (m, pts, want) in enumerate(zip(g["jac_maps"], g["jac_points"], g["jac_out"])):
        size, pos, offset, res, t = m[0:3], m[3:6], m[6:9], int(m[9]), m[10:13]
        om = O.OracleMap(size, 0, 0, pos=pos, offset=offset, data=g[f"jac_data_{case}"])
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = t
        J, vals, mask = O.calc_jacobis(om, T, pts, res)
        assert np.array_equal(mask.astype(np.int64), want[:, 0]), f"case {case}: mask differs at {np.nonzero(mask != want[:, 0])[0][:5]}"
        on = mask.astype(bool)
        assert np.array_equal(vals[on].astype(np.int64), want[on, 1]), f"case {case}: values differ"
        assert np.array_equal(J[on], want[on, 2:]), f"case {case}: Jacobians differ at {np.nonzero((J[on] != want[on, 2:]).any(axis=1))[0][:5]}"
        n_masked += int(on.sum())
    assert n_masked > 2000  # thousands of points fall on observed voxels inside the window: the gradient rule is exercised, not just the bounds test
    out = g["jac_out"]
    assert (np.abs(out[:, :, 2:5]).max() > 2 ** 31 - 2 ** 27) or (np.abs(out[:, :, 5:]).max() > 1000)


def test_live_reference_headers_if_present():
    """Ring-buffer index math on random maps and queries (O.ring_index_cases) against the answers of the reference header
    recorded from oracle/_ref (tests/golden/ref_get_index.npz), and where oracle/_ref was built, against it directly."""
    g = np.load(GOLD_INDEX)
    R = O.ref_lib()
    L = O.lib()
    cases = O.ring_index_cases()
    assert len(cases) == len(g["maps"])
    for case, (size, pos, off, qs) in enumerate(cases):
        # the fixture was recorded on these very inputs
        assert np.array_equal(g["maps"][case], np.concatenate([size, pos, off])) and np.array_equal(g["queries"][case], qs)
        om = O.OracleMap(size, 0, 0, pos=pos, offset=off)
        v = om.view()
        got = np.array([L.wso_get_index(C.byref(v), int(x), int(y), int(z)) for x, y, z in qs])
        assert np.array_equal(got, g["index"][case]), f"case {case}: differs at {np.nonzero(got != g['index'][case])[0][:5]}"
        if R is not None:
            data = np.zeros(int(np.prod(size)), dtype=np.uint32)
            h = R.ref_map_create(size.ctypes.data, pos.ctypes.data, off.ctypes.data, data.ctypes.data)
            live = np.array([R.ref_get_index(h, int(x), int(y), int(z)) for x, y, z in qs])
            R.ref_map_destroy(h)
            assert np.array_equal(live, got), f"case {case}"


# ------------------------------------------------------------------ 3. whole-scan counters of the reference kernel source
def test_synthetic_scan_counters_match_reference_kernel():
    """BASELINE.md §2 / SURVEY.md §8d: the reference's cu_min_tsdf_krnl on the synthetic OS1-128 scan makes
    V = 35 442 598 write_tsdf_min calls, touches T = 13 901 324 voxels, 1 522 214 of them end with a negative weight
    (513^3 map, res 50, tau 1000, serial order).  The oracle must reproduce all three (the last one is order dependent)."""
    pts = S.os1_128_scan()
    assert pts.shape == (131072, 3)
    assert abs(np.sqrt((pts.astype(np.float64) ** 2).sum(1)).mean() - 9276) < 1.0
    new = O.OracleMap((512, 512, 512), 1000, 0)
    st = O.update_min(new, pts, (0, 0, 0), (0, 0, 32768), 1000, 50)
    _, w = O.unpack(new.data)
    assert st.write_calls == 35_442_598
    assert int((new.data != O.pack(1000, 0)).sum()) == 13_901_324
    assert int((w < 0).sum()) == 1_522_214


# ------------------------------------------------------------------ 4. the 6x6 solve against the reference's algorithm class
def test_solver_agrees_with_a_lapack_solve_on_real_normal_equations():
    """tsdf_registration.cpp:69 inverts with Eigen (PartialPivLU for a 6x6) and multiplies.  The oracle's wso_solve6 is a
    Gauss-Jordan elimination with partial pivoting whose multipliers come from the pivots' reciprocals (the order of operations
    is this repository's choice: on the GPU the solve is one wave's dependent chain).  Parity for that step is unpinned by
    design -- the Eigen version is not fixed by the reference -- so it is held against LAPACK's partial-pivoting solve
    (numpy), the same algorithm class: normal equations of a real registration (every iteration's h, g with the damping of
    :66), relative difference far below what the pose's float32 keeps."""
    import ctypes as C
    size, tau, res, mw = (96, 96, 48), 1000, 50, 640
    pts = S.os1_128_scan(rings=32, azimuths=256, half_extents_mm=(2000.0, 1700.0, 800.0), seed=1)
    oa = O.OracleMap(size, tau, 0)
    on = oa.copy()
    O.update_tsdf(oa, on, pts, (0, 0, 0), (0, 0, 32768), tau, mw, res)
    q = S.transform_points_mm(pts, S.perturbation(30, 20, 0, 1.5))
    L = O.lib()
    T = np.eye(4)
    worst = 0.0
    for it in range(12):
        h, g, e, c = O.reg_iterate(oa, T, q, res)
        assert c > 0
        hf = np.asarray(h, dtype=np.float64).reshape(6, 6).T.copy() + np.eye(6) * float(np.float32(0.1 * it) * np.float32(c))
        gf = np.asarray(g, dtype=np.float64).copy()
        x = np.zeros(6)
        assert L.wso_solve6(hf.ctypes.data_as(C.c_void_p), gf.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p)) == 0
        ref = np.linalg.solve(hf, gf)
        worst = max(worst, float(np.abs(x - ref).max() / np.abs(ref).max()))
        # move on a little so that the systems differ
        T = T.copy()
        T[:3, 3] += (-2.0, -1.5, 0.0)
    assert worst < 1e-9, worst


@pytest.mark.parametrize("scene", [0, 1, 2])
def test_gauss_newton_loop_with_eigens_inverse_gives_the_oracles_registration(scene):
    """VERDICT r5 #12 / task 8a: the 6x6 step `xi = -hf.inverse() * gf` (tsdf_registration.cpp:69) is third-party arithmetic (Eigen,
    unpinned), and round 5 changed the oracle's own elimination (LU -> Gauss-Jordan with pivot reciprocals) -- held against LAPACK
    per SOLVE only.  Here the WHOLE Gauss-Newton loop (tsdf_registration.cpp:55-92) is restated with the step written the way
    the reference writes it -- an explicit inverse times the gradient (numpy / LAPACK), and once more as a plain solve -- around the
    oracle's own perform_registration and xi_to_transform, and compared with wso_register_cloud on three scenes: the same
    number of iterations and a pose within the north star's 1e-4 m / 1e-4 rad (in fact within a float32 ulp or two)."""
    import ctypes as C
    from warpsense_amd import synthetic as S
    tau, res, mw = 1000, 50, 640
    size, rings, az, he, pert = [((96, 96, 48), 32, 128, (2000.0, 1700.0, 800.0), (25, -15, 5, 1.2)),
                                 ((128, 128, 64), 64, 256, (2600.0, 2300.0, 1000.0), (100, 100, 0, 5.0)),
                                 ((128, 96, 64), 48, 192, (2400.0, 1500.0, 1100.0), (-60, 35, 12, -3.0))][scene]
    pts = S.os1_128_scan(rings=rings, azimuths=az, half_extents_mm=he, seed=40 + scene)
    avg = O.OracleMap(size, tau, 0)
    new = avg.copy()
    O.update_tsdf(avg, new, pts, (0, 0, 0), (0, 0, 32768), tau, mw, res)
    cloud = S.transform_points_mm(pts, S.perturbation(*pert))
    max_it, grad, eps = 200, np.float32(0.1), np.float32(0.03)
    T_ref, it_ref, _ = O.register_cloud(avg, cloud, np.eye(4), max_it, float(grad), float(eps), res)

    def loop(step):
        T = np.eye(4, dtype=np.float32)
        center = np.array([int(T[0, 3]), int(T[1, 3]), int(T[2, 3])], dtype=np.int32)  # fixed for the call, :33
        alpha = np.float32(0.0)
        prev = [np.float32(0)] * 4
        it = 0
        finished = False
        while not finished and it < max_it:
            h, g, e, c = O.reg_iterate(avg, T, cloud, res)
            it += 1
            if c == 0:
                break
            hf = h.astype(np.float64) + float(np.float32(alpha * np.float32(c))) * np.eye(6)  # alpha * gpu_c: a float product, :66
            xi = -step(hf, g.astype(np.float64))
            tr = np.zeros(16, dtype=np.float32)
            O.lib().wso_xi_to_transform(O._p(np.ascontiguousarray(xi, dtype=np.float64)), O._p(center), O._p(tr))
            tr = tr.reshape(4, 4).T  # column-major -> math layout
            alpha = np.float32(alpha + grad)
            # total = transform * total in float32, element by element like the reference's Eigen product / the oracle's matmul4f
            Tn = np.zeros((4, 4), dtype=np.float32)
            for i in range(4):
                for j in range(4):
                    s = np.float32(0)
                    for k in range(4):
                        s = np.float32(s + np.float32(tr[i, k] * T[k, j]))
                    Tn[i, j] = s
            T = Tn
            err = np.float32(np.float32(e) / np.float32(c))
            if abs(np.float32(err - prev[2])) < eps and abs(np.float32(err - prev[0])) < eps:
                finished = True
            prev = [prev[1], prev[2], prev[3], err]
        return T, it

    for name, step in (("inverse", lambda hf, gf: np.linalg.inv(hf) @ gf), ("solve", np.linalg.solve)):
        T, it = loop(step)
        assert it == it_ref and it > 5, (name, it, it_ref)
        dt = np.linalg.norm(T[:3, 3].astype(np.float64) - T_ref[:3, 3]) / 1000.0
        R = T[:3, :3].astype(np.float64) @ np.asarray(T_ref, dtype=np.float64)[:3, :3].T
        k = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
        ang = np.arctan2(np.linalg.norm(k), (np.trace(R) - 1) / 2)
        assert dt < 1e-4 and ang < 1e-4, (name, dt, ang)
