"""The numpy models of the queries where tests/test_gpu_query_domain.py leans on them, without a GPU: hand-worked single-cell ray
casts at res 2, 3 and 1024, the sphere at res 51 and 1024 through the ray cast's and the mesh's model, the translation of every
model by whole voxels up to the far positions of the GPU tests, and the inputs of those tests: in the model alone every fixture
clears the thresholds the GPU tests assert."""
import numpy as np
import pytest

import distance_model as D
import mesh_model as M
import query_domain_scenes as Q
import query_model as QM
import raycast_model as R
import store_scenes as SM
import surface_model as G


# ------------------------------------------------------------------------------------------------ hand-worked single cells
def _slab_ring(front, behind):
    """4 x 4 x 4 voxels at lo = (0, 0, 0), all weights 64: value `front` for x <= 1, `behind` for x >= 2"""
    import warpsense_amd as W
    value = np.full((4, 4, 4), front)
    value[2:] = behind
    return R.Ring.of_box(W.pack_entry(value.reshape(-1), np.full(64, 64)).astype(np.uint32).reshape(4, 4, 4), (0, 0, 0))


def _T(ring, res, x, y):
    ok, T = R.field(ring, res, np.array([[x, y, y]], dtype=np.int64), False)
    assert bool(ok[0])
    return int(T[0])


def _cast(ring, res, o, d, max_range):
    rec, grad = R.model(ring, res, o, np.asarray(d).reshape(-1, 3), max_range)
    return [tuple(int(r[k]) for k in R.RAY.names) for r in rec], grad.tolist()


def test_hand_worked_cell_at_res_2():
    """res 2: h = 1, step = max(2 / 2, 1) = 1.  Values +20 for x <= 1, -30 for x >= 2.  Ray from o = (1, 3, 3) -- the sample point of
    voxel (0, 1, 1) -- along (1, 0, 0): p_k = (1 + k, 3, 3), q = (k, 2, 2), b = (floor(k / 2), 1, 1), f = (k mod 2, 0, 0).  fy = fz = 0:
    T = (value(bx) (2 - fx) + value(bx + 1) fx) * 2 * 2.
      k = 0: 20 * 2 * 4 = 160    k = 1: (20 + 20) * 4 = 160    k = 2: b = 1, 20 * 2 * 4 = 160    k = 3: b = 1, (20 - 30) * 4 = -40
    t = s_2 + floor(1 * 160 / (160 + 40)) = 2 + 0 = 2; hit (3, 3, 3).  Gradient at g = floor(3 / 2) = (1, 1, 1): (-30 - 20, 0, 0)."""
    ring = _slab_ring(20, -30)
    assert [_T(ring, 2, 1 + k, 3) for k in range(4)] == [160, 160, 160, -40]
    assert _cast(ring, 2, (1, 3, 3), (1, 0, 0), 6) == ([(3, 3, 3, 2)], [[-50, 0, 0]])
    assert _cast(ring, 2, (1, 3, 3), (5, 0, 0), 3)[0] == [(3, 3, 3, 2)] and _cast(ring, 2, (1, 3, 3), (1, 0, 0), 2)[0] == [(0, 0, 0, -1)]  # K = 3 / K = 2


def test_hand_worked_cell_at_res_3():
    """res 3: h = 3 / 2 = 1 and step = max(3 / 2, 1) = 1, not 3 / 2 rounded; the fractions are 0, 1, 2.  Values +20 for x <= 1, -30 for
    x >= 2.  Ray from o = (1, 4, 4) -- the sample point of voxel (0, 1, 1) -- along (1, 0, 0): p_k = (1 + k, 4, 4), q = (k, 3, 3),
    b = (floor(k / 3), 1, 1), f = (k mod 3, 0, 0).  T = (value(bx) (3 - fx) + value(bx + 1) fx) * 3 * 3.
      k = 0 .. 3: 20 * 3 * 9 = 540 (b = 0, both corners +20; k = 3: b = 1, f = 0)
      k = 4: b = 1, f = 1: (20 * 2 - 30 * 1) * 9 = 90          k = 5: b = 1, f = 2: (20 * 1 - 30 * 2) * 9 = -360
    t = s_4 + floor(1 * 90 / (90 + 360)) = 4 + 0 = 4; hit (5, 4, 4) -- the line from +20 at x = 4 to -30 at x = 7 passes zero at 5.2.
    Gradient at g = floor(5 / 3) = (1, 1, 1): (-30 - 20, 0, 0).  With a step of 2 the samples k = 2, 3 would be p = 5, 7, T = 90, -810,
    t = 4 + floor(2 * 90 / 900) = 4: this ray alone would not tell; the sample before the crossing does: p_4 = 5, not 9."""
    ring = _slab_ring(20, -30)
    assert [_T(ring, 3, 1 + k, 4) for k in range(6)] == [540, 540, 540, 540, 90, -360]
    assert _cast(ring, 3, (1, 4, 4), (1, 0, 0), 9) == ([(5, 4, 4, 4)], [[-50, 0, 0]])
    assert _cast(ring, 3, (1, 4, 4), (1, 0, 0), 5)[0] == [(5, 4, 4, 4)] and _cast(ring, 3, (1, 4, 4), (1, 0, 0), 4)[0] == [(0, 0, 0, -1)]  # K = 5 / K = 4


def test_hand_worked_cells_at_res_1024():
    """res 1024: h = 512, step = 512.  Ray from o = (512, 1536, 1536) -- the sample point of voxel (0, 1, 1) -- along (1, 0, 0):
    p_k = (512 + 512 k, 1536, 1536), q = (512 k, 1024, 1024), b = (floor(k / 2), 1, 1), f = (512 (k mod 2), 0, 0).
    T = (value(bx) (1024 - fx) + value(bx + 1) fx) * 2^20; at f = 0 the weight of corner (0, 0, 0) is exactly 1024^3 = 2^30.
    (a) values +32767 for x <= 1, -32767 for x >= 2:
      k = 0, 1, 2: 32767 * 2^30 = 35 183 298 347 008 (k = 2: b = 1, f = 0)      k = 3: b = 1, f = 512: (32767 - 32767) * 512 * 2^20 = 0
      T_3 <= 0: t = s_2 + floor(512 * T_2 / (T_2 - 0)) = 1024 + 512 = 1536; hit (2048, 1536, 1536); g = (2, 1, 1): (-32767 - 32767, 0, 0).
    (b) values +32767 for x <= 1, -16384 for x >= 2:
      k = 3: (32767 - 16384) * 512 * 2^20 = 16383 * 2^29 = 8 795 556 151 296 > 0       k = 4: b = 2, f = 0: -16384 * 2^30 = -2^44
      t = s_3 + floor(512 * 16383 * 2^29 / (16383 * 2^29 + 2^44)) = 1536 + floor(8 388 096 / 49 151) = 1536 + 170 = 1706
      (step T_3 = 2^52.0); hit (2218, 1536, 1536); g = (2, 1, 1): (-16384 - 32767, 0, 0)."""
    a = _slab_ring(32767, -32767)
    assert [_T(a, 1024, 512 + 512 * k, 1536) for k in range(4)] == [32767 * 2 ** 30] * 3 + [0] and 32767 * 2 ** 30 == 35_183_298_347_008
    assert _cast(a, 1024, (512, 1536, 1536), (1, 0, 0), 3000) == ([(2048, 1536, 1536, 1536)], [[-65534, 0, 0]])
    b = _slab_ring(32767, -16384)
    assert [_T(b, 1024, 512 + 512 * k, 1536) for k in (3, 4)] == [16383 * 2 ** 29, -2 ** 44] and 16383 * 2 ** 29 == 8_795_556_151_296
    assert 49151 * 170 <= 8_388_096 < 49151 * 171
    assert _cast(b, 1024, (512, 1536, 1536), (1, 0, 0), 3000) == ([(2218, 1536, 1536, 1706)], [[-49151, 0, 0]])
    assert _cast(b, 1024, (512, 1536, 1536), (1, 0, 0), 2047)[0] == [(0, 0, 0, -1)]  # K = 3


# ------------------------------------------------------------------------------------------------ the sphere at other resolutions
SPHERE_RES = {51: (1020, 2.31, 2.92, 0.0219, 4.60, [1475, 1480]), 1024: (20480, 35.6, 55.7, 0.0214, 51.0, [1477, 1478])}


@pytest.mark.parametrize("res", sorted(SPHERE_RES))
def test_sphere_at_other_resolutions(res):
    """The sphere maps of test_gpu_mesh at res 51 (tau 1020) and res 1024 (tau 20480: 20 voxels, as 1000 is at res 50), the model
    against the analytic sphere.  Measured, small sphere / large sphere:
      res 51:   ray cast: 1 475 / 1 480 rays within 0.8 R, all of them hit; largest distance of a hit to the sphere 2.28 / 2.30 mm,
                largest range error of the 0.8 R rays 2.91 / 1.95 mm; mesh: volume 0.9782 / 0.9934 of the sphere's, largest distance of
                a vertex to the sphere 4.59 / 3.70 mm
      res 1024: ray cast: 1 477 / 1 478 rays; 35.6 / 20.2 mm; 55.6 / 31.0 mm; mesh: volume 0.9787 / 0.9934, 50.9 / 29.4 mm
    (res / 10 would be 5.1 and 102.4 mm; at res 50 the same code measures 2.7 / 1.8, 4.02 / 3.50, 0.9787 / 0.9933 and 3.34 / 2.93.)
    The bounds are the larger measured figure plus a quarter of it; for the volume, the larger shortfall plus a quarter.  The input is
    fixed, so nothing varies from run to run."""
    tau, ray_dist, ray_err, vol, mesh_dist, cores = SPHERE_RES[res]
    seen = []
    for edge, centre, radius in M.SPHERES:
        box = M.sphere_box(edge, centre, radius, res=res, tau=tau).reshape((edge,) * 3)
        o, d, c_mm = R.sphere_rays(centre, radius, res=res)
        rec, grad = R.model(R.Ring.of_box(box, M.SPHERE_LO), res, o, d, 80 * res)
        core, dist, err = R.check_sphere(rec, o, d, c_mm, radius * res, bound=1.25 * ray_err)  # every core ray hits, none that misses does
        assert dist <= 1.25 * ray_dist
        seen.append(core)
        ratio, far = M.sphere_mesh_numbers(edge, centre, radius, res=res, tau=tau)
        assert abs(ratio - 1.0) < 1.25 * vol and far < 1.25 * mesh_dist
    assert seen == cores


# ------------------------------------------------------------------------------------------------ translation by whole voxels
@pytest.mark.parametrize("row", Q.FAR_ROWS + [(r, p) for r in (50, 1024, 2) for p in (Q.edge_case(r, 1)[0], Q.edge_case(r, -1)[0])],
                         ids=lambda row: f"res{row[0]}-x{row[1][0]}")
def test_every_model_moves_with_the_window(row):
    """the same entries at NEAR and at a far position, origin and targets moved by s res: the ray cast's ranges and gradients, the
    mesh's faces and weights, the distance records and the surface's raw entries are identical; hit points and vertices move by s res,
    surface voxels by s"""
    res, pos = row
    s = np.asarray(pos, dtype=np.int64) - Q.NEAR
    near, far = Q.ring(Q.NEAR), Q.ring(pos)
    (o0, d, rng), (o1, _, _) = Q.rays(res, Q.NEAR), Q.rays(res, pos)
    assert np.array_equal(o1 - o0, s * res)
    for any_weight in (False, True):
        a, b = R.model(near, res, o0, d, rng, any_weight), R.model(far, res, o1, d, rng, any_weight)
        assert Q.counts(a)[0] > 500 and R.same(b, (Q.moved(a[0], s * res), a[1]))
    dr = d[:Q.N_RANDOM]
    a, b = R.model(near, res, o0, o0 + dr, rng, False, True), R.model(far, res, o1, o1 + dr, rng, False, True)
    assert R.same(b, (Q.moved(a[0], s * res), a[1])) and R.same(a, R.model(near, res, o0, dr, rng))
    views = [type("V", (), dict(data_=e, size_=np.asarray(Q.SIZE), pos_=np.asarray(p), offset_=np.asarray(Q.OFF)))
             for p in (Q.NEAR, pos) for e in Q.entries()]  # near avg, near new, far avg, far new
    for any_weight in (False, True):
        (va, fa), (vb, fb) = M.model(views[0], res, any_weight=any_weight), M.model(views[2], res, any_weight=any_weight)
        assert len(fa) > 100 and M.same((vb, fb), (Q.moved_vert(va, s * res), fa))
    (ra, ma), (rb, mb) = G.model(views[0], Q.TAU, res), G.model(views[2], Q.TAU, res)
    assert len(ra) > 100 and QM.same(rb, Q.moved_surface(ra, s)) and np.array_equal(ma[:, 3:], mb[:, 3:])
    for kw in ({}, dict(unknown_occupied=True), dict(columns=True)):
        assert D.same(D.model(views[3], 5, **kw)[0], D.model(views[1], 5, **kw)[0])


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
def test_window_fixtures_clear_their_thresholds_in_the_model():
    """per row: hits and non-zero gradients of the 2058 rays under both weight rules (more than 500 / 300), vertices and faces of the
    window and of the inner box (more than 100), surface records (more than 100), distance sites"""
    for res, pos in Q.ROWS:  # (the windows at the edge of the origin range: test_every_model_moves_with_the_window)
        ring = Q.ring(pos)
        o, d, rng = Q.rays(res, pos)
        for any_weight in (False, True):
            n_hit, n_grad = Q.counts(R.model(ring, res, o, d, rng, any_weight))
            print(res, pos, any_weight, "hits", n_hit, "gradients", n_grad)
            assert n_hit > 500 and n_grad > 300
    lo, hi = QM.window(Q.SIZE, Q.NEAR)
    for a, b in ((lo, hi), Q.inner_box(Q.NEAR)):
        box = QM.ring_box(Q.entries()[0], Q.SIZE, Q.NEAR, Q.OFF, a, b)
        for any_weight in (False, True):
            nv, nf = M.model_counts(box, any_weight)
            print("mesh", tuple(b - a + 1), any_weight, nv, nf)
            assert nv > 100 and nf > 100
        assert len(G.model_box(box, a, Q.TAU, 50)[0]) > 100
        dbox = QM.ring_box(Q.entries()[1], Q.SIZE, Q.NEAR, Q.OFF, a, b)
        for kw in ({}, dict(unknown_occupied=True), dict(columns=True)):
            rec, n_sites = D.model_box(dbox, 5, **kw)
            d2 = rec & np.uint32(0xFFFFFF)
            assert n_sites >= 3 and np.count_nonzero((d2 > 0) & (d2 < 25)) > 20, kw
    assert all(int(v) != 0 for v in Q.OFF) and Q.SIZE in G.SIZES


def test_wrapping_targets_are_dead_in_the_model_and_would_hit_in_32_bits():
    for res in (50, 1024, 2):
        pos, o, rng = Q.edge_case(res, -1)
        tgt = Q.wrap_targets(o, rng, res)
        d = tgt - o
        assert np.all(d[:64, 0] == 2 ** 30 - 1) and np.all(d[64:128, 0] == 2 ** 30) and np.all(d[128:, 0] > 2 ** 32 - 70000)
        hit = R.model(Q.ring(pos), res, o, tgt, rng, True, True)[0]["range_mm"] >= 0
        wrapped = o + ((d + 2 ** 31) % 2 ** 32 - 2 ** 31)  # the targets a 32-bit subtraction would see
        hit32 = R.model(Q.ring(pos), res, o, wrapped, rng, True, True)[0]["range_mm"] >= 0
        print(res, [int(hit[k:k + 64].sum()) for k in (0, 64, 128)], [int(hit32[k:k + 64].sum()) for k in (0, 64, 128)])
        assert hit[:64].sum() > 16 and not hit[64:].any() and hit32[128:].sum() > 16


@pytest.mark.parametrize("case", Q.STORE_CASES, ids=Q.store_id)
def test_store_fixtures_clear_their_thresholds_in_the_model(case):
    res, where = case
    chunks = Q.store_chunks(res, where)
    K, x_lone = Q.store_keys(res, where)
    lo, hi = SM.bounding_box(chunks)
    assert len(chunks) == 8 and all((abs(int(c)) + 1) * res <= Q.I32 for c in list(lo) + list(hi))  # the mesh's range rule passes
    if where != "near":
        assert Q.I32 - (max(abs(int(lo[0])), abs(int(hi[0]))) + 1) * res < Q.CS * res  # within one chunk of the end of int32
        assert abs(x_lone) >= 2 ** 20 or res > 30
    for name, (o, d, rng) in Q.store_rays(res, where).items():
        assert all(abs(int(c)) + rng + 2 * res <= Q.I32 for c in o) and np.all((d >= -2 ** 31) & (d < 2 ** 31)), name  # the ray cast's range rule passes
    for any_weight in (False, True):
        n_hit, n_grad = Q.counts(Q.store_model(res, where, "in", None, any_weight))
        print(Q.store_id(case), any_weight, "in: hits", n_hit, "gradients", n_grad)
        assert n_hit > 500 and n_grad > 300
    rec = Q.store_model(res, where, "gap")[0]
    o, d, rng = Q.store_rays(res, where)["gap"]
    hit = rec["range_mm"] >= 0
    lone_lo = x_lone * Q.CS * res
    print(Q.store_id(case), "gap: hits", int(hit.sum()), "of", len(d), "range", rng)
    hit[256:] = False  # (the rays behind the first 256 run the other way, into the block)
    assert hit.sum() > 50 and np.all((rec["x_mm"][hit] >= lone_lo) & (rec["x_mm"][hit] < lone_lo + Q.CS * res))  # in the isolated chunk
    assert np.all(rec["range_mm"][hit] > (Q.GAP - 2) * Q.CS * res)
