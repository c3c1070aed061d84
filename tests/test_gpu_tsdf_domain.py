"""GPU parity of the TSDF update and the registration at the integer-domain edges of the ray set-up (ray_setup_block,
tsdf_setup.hip): odd resolutions and free tau / max_weight, rays on both sides of each term of the `fast` predicate, windows
beyond the biased route's reach (MarchFrame::biased_ok), the record key's step / fan fields at every split of rec_format, and
key-range rays at the edges of the set-up's workgroups.  Every case states the boundary it is about and asserts -- through a
numpy restatement of the set-up's per-ray predicates -- that its scan holds rays on both sides of it."""
import numpy as np
import pytest

import oracle_lib as O
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu

UP = (0, 0, 32768)
MR = 32768


# ---------------------------------------------------------------- the set-up's per-ray predicates, restated in int64
def _wrap32(a):
    return ((np.asarray(a, dtype=np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _tdiv(a, b):
    """C division (toward zero) of int64 arrays"""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def rec_format(n):
    P = 1
    while (1 << P) < n:
        P += 1
    R = 38 - P
    F = 5 + (R - 18) // 3
    Sb = R - F
    if Sb > 16:
        Sb, F = 16, min(8, R - 16)
    return Sb, F


def biased_ok(res, size, pos):
    reach = max(abs(int(p)) + int(s) // 2 + 4 for p, s in zip(pos, size))
    return reach < (1 << 22) and reach * res < (1 << 30)


def ray_predicates(pts, sensor, res, tau, size, pos, n=None):
    """per ray: accepted (in_bounds_with_buffer_pos, distance > 0), distance, steps, fan width, the six terms of `fast`, fast,
    RAY_SIMPLE and whether the scan's key split holds the ray -- ray_setup_block line by line (iv from the int64 formulas)"""
    p = np.asarray(pts, dtype=np.int64)
    n = p.shape[0] if n is None else n
    size = np.asarray(size, dtype=np.int64)
    mpos = np.asarray(pos, dtype=np.int64)
    half = res // 2
    c = np.floor(p.astype(np.float32) / np.float32(res)).astype(np.int64)
    ok = np.all(np.abs(c - mpos) <= size // 2 + tau // res // 2, axis=1)
    spos = _wrap32(np.asarray(sensor, dtype=np.int64) * res + half)
    d = _wrap32(p - spos)
    sq = _wrap32((d * d).sum(axis=1) % 2 ** 32)
    dist = np.where(sq < 0, 0, np.floor(np.sqrt(np.maximum(sq, 0).astype(np.float32))).astype(np.int64))
    ok &= dist > 0
    dsafe = np.maximum(dist, 1)
    nd = _tdiv(d * MR, dsafe[:, None])
    u = np.asarray(UP, dtype=np.int64)
    c1 = np.stack([_tdiv(nd[:, 1] * u[2] - nd[:, 2] * u[1], MR), _tdiv(nd[:, 2] * u[0] - nd[:, 0] * u[2], MR),
                   _tdiv(nd[:, 0] * u[1] - nd[:, 1] * u[0], MR)], axis=1)
    with np.errstate(over="ignore"):
        iv = np.stack([nd[:, 1] * c1[:, 2] - nd[:, 2] * c1[:, 1], nd[:, 2] * c1[:, 0] - nd[:, 0] * c1[:, 2],
                       nd[:, 0] * c1[:, 1] - nd[:, 1] * c1[:, 0]], axis=1)
        isq = (iv * iv).sum(axis=1)
    inorm = np.where(isq < 0, np.iinfo(np.int64).min, np.floor(np.sqrt(np.maximum(isq, 0).astype(np.float32).astype(np.float64)).astype(np.float32)).astype(np.int64))
    ok &= inorm != 0
    with np.errstate(over="ignore"):
        # (a wrapped sum of squares gives INT64_MIN, and every quotient by it is 0)
        ivn = np.where((inorm == np.iinfo(np.int64).min)[:, None], 0, _tdiv(iv * MR, np.where(inorm <= 0, 1, inorm)[:, None]))
    L = dist + tau
    steps = _tdiv(L - 1, half) + 1
    mdz = 100 * L // MR
    fan = (2 * mdz) // res + 1
    Sb, F = rec_format(n)
    # (the third rejection term: a normalised fan direction outside int32, which only a wrapped iv can give)
    small_iv = np.all((ivn >= np.iinfo(np.int32).min) & (ivn <= np.iinfo(np.int32).max), axis=1)
    in_key = (steps <= (1 << Sb)) & (fan <= (1 << F) - 1) & small_iv
    in_widest = (steps <= 1 << 16) & (fan <= 255) & small_iv
    dmax = np.abs(d).max(axis=1)
    pmax = int(np.abs(spos).max())
    ivmax = np.abs(ivn).max(axis=1)
    terms = {"dmax<=dist": dmax <= dist, "dmax*len": dmax * L < 2 ** 31, "pmax": pmax + dmax + 2 * res + tau < 2 ** 30,
             "res*dist": res * dist < 2 ** 32, "fan*iv": (2 * mdz + res) * ivmax < 2 ** 31, "len^2": (L + 2 * res) ** 2 < 2 ** 31}
    fast = np.ones(len(p), dtype=bool)
    for t in terms.values():
        fast &= t
    margin = 4 + (mdz + res) // res
    end = spos[None, :] + _tdiv(d * L[:, None], dsafe[:, None])
    ev = _tdiv(end, res)
    lim = size[None, :] // 2 - margin[:, None]
    simple = fast & biased_ok(res, size, pos) & np.all(np.abs(np.asarray(sensor, dtype=np.int64) - mpos)[None, :] <= lim, axis=1) & \
        np.all(np.abs(ev - mpos[None, :]) <= lim, axis=1)
    return dict(ok=ok, dist=dist, steps=steps, fan=fan, terms=terms, fast=fast, simple=simple, in_key=in_key, in_widest=in_widest,
                S=Sb, F=F)


def both_sides(mask, ok, what):
    m = np.asarray(mask)[ok]
    assert m.any() and (~m).any(), f"coverage: no rays on both sides of {what} ({int(m.sum())} of {m.size})"


# ---------------------------------------------------------------- maps
def _pair_at(size, tau, res, mw, pos, offset, data=None):
    import warpsense_amd as W
    size = [s if s % 2 == 1 else s + 1 for s in size]
    n = int(np.prod(np.asarray(size, dtype=np.int64)))
    if data is None:
        data = np.full(n, O.pack(tau, 0), dtype=np.uint32)
    view = W.DeviceMap(size, offset, data.copy(), pos)
    t = W.TSDFCuda(view, tau, mw, res)
    oa = O.OracleMap(size, tau, 0, pos=pos, offset=offset, data=data.copy())
    return view, t, oa, oa.copy()


def _download(t, view, which):
    import warpsense_amd as W
    host = W.DeviceMap(view.size_.copy(), view.offset_.copy(), np.empty_like(view.data_), view.pos_.copy())
    (t.avg_map() if which == 0 else t.new_map()).to_host(host)
    return host.data_


def boundary_points(sensor, res, pos, size, rng, n_rand=400):
    """int32 points at voxel boundaries (+-k res, +-k res +- 1, the zero cell), the scanner position itself, points with zero
    direction components, duplicates that contest one voxel -- inside the window (+ its buffer) around `pos`"""
    spos = np.asarray(sensor, dtype=np.int64) * res + res // 2
    lo = (np.asarray(pos) - np.asarray(size) // 2) * res
    hi = (np.asarray(pos) + np.asarray(size) // 2) * res
    out = [spos.copy()]  # distance 0
    for ax in range(3):
        for k in (1, 2, 3, 5, 8, 13):
            for e in (-1, 0, 1):
                for s in (-1, 1):
                    q = spos.copy()
                    q[ax] = (spos[ax] // res + s * k) * res + e
                    out.append(q)
    for v in range(-res + 1, res, max(1, res // 7)):  # the zero cell [-res + 1, res - 1] of the truncating division
        out.append(np.array([v, spos[1] + 3 * res, spos[2]]))
        out.append(np.array([spos[0] + 3 * res, v, spos[2]]))
    r = rng.integers(lo, hi + 1, size=(n_rand, 3))
    out.extend(list(r))
    dup = rng.integers(lo, hi + 1, size=(8, 3))
    for q in dup:
        out.extend([q, q, q + 1])  # the same voxel, several times
    a = np.asarray(out, dtype=np.int64)
    keep = np.all((a >= lo - res) & (a <= hi + res), axis=1)
    return a[keep].astype(np.int32)


def scan_in_window(sensor, res, pos, size, seed, rings=32, az=256):
    """os1_128_scan room fitted to the window and moved to the sensor"""
    he = tuple(0.45 * s * res for s in size)
    p = S.os1_128_scan(rings=rings, azimuths=az, seed=seed, half_extents_mm=he).astype(np.int64)
    p += np.asarray(pos, dtype=np.int64) * res
    return p.astype(np.int32)


def run_case(view, t, oa, on, scans, sensor, res, tau, mw, expect_error=0, oracle_scans=None):
    """scatter + integrate for scans[0], update_tsdf for the rest: new_map / avg_map bit for bit against the oracle"""
    import torch
    oracle_scans = scans if oracle_scans is None else oracle_scans
    t.scatter(torch.from_numpy(scans[0]).cuda(), sensor, UP)
    O.update_min(on, oracle_scans[0], sensor, UP, tau, res)
    st = t.stats()  # (first: it takes the error bits, which the download would raise)
    got = _download(t, view, 1)
    assert st["error_flags"] == expect_error, st
    assert np.array_equal(got, on.data), f"scatter: {np.count_nonzero(got != on.data)} voxels differ"
    t.integrate()
    O.update_avg(on, oa, mw, tau)
    assert np.array_equal(_download(t, view, 0), oa.data), "integrate"
    for k, (p, po) in enumerate(zip(scans[1:], oracle_scans[1:])):
        t.update_tsdf(torch.from_numpy(p).cuda(), sensor, UP)
        O.update_tsdf(oa, on, po, sensor, UP, tau, mw, res)
        st = t.stats()
        assert st["error_flags"] == expect_error, st
        got = _download(t, view, 0)
        assert np.array_equal(got, oa.data), f"update {k + 1}: {np.count_nonzero(got != oa.data)} voxels differ"
    assert np.all(_download(t, view, 1) == O.pack(tau, 0))


def _pose_error(A, B):
    """translation (m) and rotation (rad) between two row-major poses in mm"""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    dt = np.linalg.norm(A[:3, 3] - B[:3, 3]) / 1000.0
    R = A[:3, :3] @ B[:3, :3].T
    k = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    return dt, np.arctan2(np.linalg.norm(k), (np.trace(R) - 1) / 2)


def check_registration(t, oa, q, res, cloud=False):
    """perform_registration (both flags) on the map the case left behind == O.reg_iterate; register_cloud == O.register_cloud"""
    import warpsense_amd as W
    rc = W.RegistrationCuda()
    try:
        rc.prepare_registration(q)
        for flags in (0, 1):
            rc.flags = flags
            for T in (np.eye(4, dtype=np.float32), S.perturbation(0.4 * res, -0.3 * res, 0.1 * res, 1.5)):
                h, g, e, c = rc.perform_registration(t.device_map(), T, res)
                ho, go, eo, co = O.reg_iterate(oa, T, q, res, flags)
                assert (e, c) == (eo, co) and np.array_equal(g, go) and np.array_equal(h, ho), (flags, e, eo, c, co)
        if cloud:
            rc.flags = 0
            Tg, it = rc.register_cloud(t.device_map(), np.eye(4, dtype=np.float32), 200, 0.1, 0.03, res)
            To, ito, _ = O.register_cloud(oa, q, np.eye(4), 200, 0.1, 0.03, res)
            assert it == ito, (it, ito)
            # (the tolerance of test_gpu_registration.py::test_register_cloud_matches_oracle_pose: 1e-4 m, 1e-4 rad)
            dt, ang = _pose_error(Tg, To)
            assert dt < 1e-4 and ang < 1e-4, (dt, ang)
    finally:
        rc.close()


# ---------------------------------------------------------------- 1 / 6 / 7: odd resolutions, free tau and max_weight, every integrate route
ODD = [  # res, tau, max_weight, window, pos, offset, integrate route
    (3, 13, 640, (101, 101, 41), (-20, 35, 4), (50, 7, 40), "SPARSE"),            # tau % res != 0, tau % 10 != 0
    (7, 5, 64, (81, 81, 31), (11, -9, 2), (3, 80, 1), "DENSE"),                   # tau < res
    (25, 333, 65, (121, 101, 41), (-4, 6, 1), (60, 0, 39), "SPARSE_SEPARATE"),
    (51, 1001, 1, (91, 91, 31), (3, 3, -1), (0, 45, 30), "SPARSE"),
    (75, 163, 32767, (71, 81, 25), (0, 0, 0), (35, 40, 12), "DENSE"),
    (333, 1000, 640, (41, 41, 15), (-2, 1, 0), (40, 1, 14), "SPARSE_SEPARATE"),
]


@pytest.mark.parametrize("res,tau,mw,size,pos,offset,route", ODD, ids=[f"res{c[0]}_tau{c[1]}_mw{c[2]}_{c[6]}" for c in ODD])
def test_odd_resolution_scans_match_oracle(res, tau, mw, size, pos, offset, route):
    """odd res (half = res / 2 truncates; div_res_b's res - 1 bias on negative numerators), tau not a multiple of res or of 10,
    tau < res, max_weight at 1 / 64 / 65 / 32767, odd windows away from the origin with a ring offset, each integrate route;
    registration of the map left behind, one perform_registration per flag and a whole register_cloud"""
    import warpsense_amd as W
    view, t, oa, on = _pair_at(size, tau, res, mw, pos, offset)
    t.set_integrate(getattr(W, "WS_INTEGRATE_" + route))
    sensor = tuple(int(p) + k for p, k in zip(pos, (1, -2, 0)))
    rng = np.random.default_rng(res * 1000 + tau)
    scans = []
    for k in range(3):
        p = np.concatenate([scan_in_window(sensor, res, pos, view.size_, 40 + k), boundary_points(sensor, res, pos, view.size_, rng)])
        scans.append(np.ascontiguousarray(p[rng.permutation(len(p))]))
    pr = ray_predicates(np.concatenate(scans), sensor, res, tau, view.size_, pos)
    assert pr["ok"].sum() > 1000
    both_sides(pr["simple"], pr["ok"], "RAY_SIMPLE (rays that leave the window)")
    assert res % 2 == 1 and biased_ok(res, view.size_, pos)
    run_case(view, t, oa, on, scans, sensor, res, tau, mw)
    q = scans[-1][pr["ok"][-len(scans[-1]):]]
    check_registration(t, oa, S.transform_points_mm(q, S.perturbation(0.3 * res, 0.2 * res, 0, 1.0)), res, cloud=True)


def test_weights_across_int16_from_the_map_side():
    """a non-default first update whose maps hold weights up to +-32767 (and -32768): integrate_entry across its domain from the
    stored side, max_weight 32767, odd res"""
    import warpsense_amd as W
    tau, res, mw = 777, 25, 32767
    size, pos, offset = (81, 81, 31), (2, -3, 1), (10, 70, 5)
    n = int(np.prod(size))
    rng = np.random.default_rng(77)
    vals = rng.integers(-tau, tau + 1, n).astype(np.int16)
    wts = rng.choice(np.array([0, 0, 1, -1, 64, -64, 32767, -32767, -32768, 20000, 32703], dtype=np.int16), n)
    data = O.pack(vals, wts).astype(np.uint32)
    for route in ("SPARSE", "DENSE"):
        view, t, oa, on = _pair_at(size, tau, res, mw, pos, offset, data=data)
        t.set_integrate(getattr(W, "WS_INTEGRATE_" + route))
        sensor = (pos[0], pos[1], pos[2])
        scans = [scan_in_window(sensor, res, pos, size, 90 + k) for k in range(2)]
        # the first update sees the pre-filled entries in new_map too (update_tsdf.cu:135-136): update_tsdf, not scatter
        import torch
        for p in scans:
            t.update_tsdf(torch.from_numpy(p).cuda(), sensor, UP)
            O.update_tsdf(oa, on, p, sensor, UP, tau, mw, res)
            assert t.stats()["error_flags"] == 0
            assert np.array_equal(_download(t, view, 0), oa.data), route
        w = (oa.data >> 16).astype(np.int16)
        assert (w == 32767).sum() > 100 and (w == -32767).sum() > 100
        check_registration(t, oa, S.transform_points_mm(scans[-1], S.perturbation(0.3 * res, 0.2 * res, 0, 1.0)), res)


# ---------------------------------------------------------------- 2: both sides of every term of `fast`
FAST = [  # res, tau, window, what the scan reaches
    (1001, 3001, (121, 121, 21), "long rays: distance wraps past 46 m, dmax * len and (len + 2 res)^2 beyond 2^31"),
    (100003, 32767, (11, 11, 5), "voxels of 100 m: res * distance beyond 2^32, the fan product beyond 2^31"),
]


@pytest.mark.parametrize("res,tau,size,what", FAST, ids=["long_rays", "huge_voxels"])
def test_rays_on_both_sides_of_the_fast_predicate(res, tau, size, what):
    """rays on both sides of each term of the fast predicate (march_steps_fast / the compacting walk against march_steps_direct), fast
    rays that leave the window (fast but not RAY_SIMPLE), shuffled so that waves mix the routes"""
    mw = 640
    pos, offset = (0, 0, 0), (size[0] // 3, 2, size[2] - 1)
    view, t, oa, on = _pair_at(size, tau, res, mw, pos, offset)
    sensor = (1, -1, 0)
    rng = np.random.default_rng(res)
    he = np.asarray(view.size_) // 2 * res
    # rays of every length out to the corners of the window, in every direction
    m = 6000
    dirs = rng.normal(size=(m, 3))
    dirs[:, 2] *= 0.15
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rng_len = rng.uniform(1e-4, 1.0, m) ** 0.5 * float(np.linalg.norm(he[:2]))
    p = np.asarray(sensor) * res + dirs * rng_len[:, None]
    p = np.clip(p, -he, he).astype(np.int64)
    p = np.concatenate([p, boundary_points(sensor, res, pos, view.size_, rng, n_rand=200)]).astype(np.int32)
    p = np.ascontiguousarray(p[rng.permutation(len(p))])
    pr = ray_predicates(p, sensor, res, tau, view.size_, pos)
    ok = pr["ok"]
    assert ok.sum() > 3000
    # (len + 2 res)^2 < 2^31 bounds res below 23 170 and the distance below 46 341: res * distance < 2^32 and the fan product
    # < 2^31 follow from it, so those two terms only ever fail on rays that are not fast anyway -- the huge voxels show them
    want = {"dmax<=dist", "dmax*len", "len^2"} if res < 2000 else {"res*dist", "fan*iv", "dmax<=dist"}
    for name in want:
        both_sides(pr["terms"][name], ok, name)
    implied = pr["terms"]["len^2"] & ~(pr["terms"]["res*dist"] & pr["terms"]["fan*iv"])
    assert not implied[ok & pr["terms"]["dmax<=dist"]].any()
    if res < 2000:
        both_sides(pr["fast"], ok, "fast")
        both_sides(pr["simple"][pr["fast"]], ok[pr["fast"]], "RAY_SIMPLE among fast rays")
        # waves of 64 consecutive rays that mix the routes
        wave_mix = [pr["fast"][i:i + 64][ok[i:i + 64]] for i in range(0, len(p), 64)]
        assert sum(1 for w in wave_mix if w.any() and (~w).any()) > 10
    scans = [p, np.ascontiguousarray(p[::-1])]
    run_case(view, t, oa, on, scans, sensor, res, tau, mw)
    check_registration(t, oa, p[ok][:4000], res)


# ---------------------------------------------------------------- 3: windows the biased route cannot take
FAR = [  # res, tau, window, map position (voxels), why biased_ok is false
    (2, 41, (65, 65, 33), (1 << 22, -17, 3), "reach >= 2^22 voxels"),
    (1000, 1000, (101, 101, 21), ((1 << 30) // 1000 - 23, 5, -2), "reach * res >= 2^30 mm, and pmax + dmax + 2 res + tau near 2^30"),
]


@pytest.mark.parametrize("res,tau,size,pos,why", FAR, ids=["reach_2^22", "reach_res_2^30"])
def test_windows_beyond_the_biased_route(res, tau, size, pos, why):
    """MarchFrame::biased_ok == false: no ray is RAY_SIMPLE, fast rays take march_steps_fast with in_bounds per candidate; the
    second window also splits its rays on the pmax term of fast.  Registration there, too"""
    mw = 640
    offset = (7, size[1] - 1, 0)
    view, t, oa, on = _pair_at(size, tau, res, mw, pos, offset)
    assert not biased_ok(res, view.size_, pos)
    sensor = (pos[0] - 3, pos[1] + 2, pos[2])
    rng = np.random.default_rng(pos[0] % 1000)
    scans = []
    for k in range(2):
        p = np.concatenate([scan_in_window(sensor, res, pos, view.size_, 60 + k), boundary_points(sensor, res, pos, view.size_, rng)])
        scans.append(np.ascontiguousarray(p[rng.permutation(len(p))]))
    pr = ray_predicates(scans[0], sensor, res, tau, view.size_, pos)
    ok = pr["ok"]
    assert ok.sum() > 1000 and not pr["simple"][ok].any() and pr["fast"][ok].any()
    if res == 1000:
        both_sides(pr["terms"]["pmax"], ok, "pmax + dmax + 2 res + tau < 2^30")
    run_case(view, t, oa, on, scans, sensor, res, tau, mw)
    q = scans[-1][ray_predicates(scans[-1], sensor, res, tau, view.size_, pos)["ok"]]
    check_registration(t, oa, S.transform_points_mm(q, S.perturbation(0.3 * res, 0.2 * res, 0, 0.5)) if res > 2 else q, res,
                       cloud=True)


# ---------------------------------------------------------------- 4: the record key's step and fan fields at every split
def _fan_edge_len(F):
    """largest len_end whose fan (res 2: 100 len / 32768 + 1) still fits F bits, i.e. iter_steps == 2^F - 1"""
    return (((1 << F) - 1) * MR - 1) // 100


def _axis_point(L, tau, res, y=1, z=1):
    """a point on the x axis of a sensor at voxel (0, 0, 0) whose ray has len_end == L exactly (distance through float32 sqrt)"""
    for d in range(L - tau - 3, L - tau + 4):
        p = np.array([[res // 2 + d, y, z]], dtype=np.int32)
        if int(ray_predicates(p, (0, 0, 0), res, tau, (3, 3, 3), (0, 0, 0))["dist"][0]) + tau == L:
            return p[0].astype(np.int64)
    raise AssertionError(f"no axis point with len_end {L}")


KEYS = [  # points in the scan, tau: both sides of every threshold of rec_format -- 16 384 | 32 768 | 65 536 | 131 072 | 262 144
    (16384, 20000), (16385, 20000), (32768, 20000), (32769, 20000), (65536, 20000), (65537, 40), (131072, 40), (131073, 40),
    (262144, 40), (262145, 40)]


@pytest.mark.parametrize("n,tau", KEYS, ids=[f"n{k[0]}" for k in KEYS])
def test_key_fields_at_their_last_admitted_value(n, tau):
    """rays at steps == 2^S and 2^S + 1, and at fan width rec_max_fan(F) and one more, for a scan on each side of the rec_format
    thresholds (padded to n with points that fail in_bounds_with_buffer_pos): the admitted ones are exact as they are, the others
    take the piecewise route and are exact, or -- beyond the widest split -- are dropped with WS_ERR_RANGE"""
    res, mw = 2, 640
    Sb, F = rec_format(n)
    sensor = (0, 0, 0)
    sx = res // 2
    lens = [1 << Sb, (1 << Sb) + 1]  # len_end == steps at res 2
    if F < 8:
        lens += [_fan_edge_len(F), _fan_edge_len(F) + 1]
    dists = [L - tau for L in lens]
    assert all(0 < d < 46341 for d in dists)
    lo, hi = min(dists) // res - 8, max(dists) // res + 8
    size = (hi - lo + 1, 5, 5)
    pos = ((lo + hi) // 2, 0, 0)
    view, t, oa, on = _pair_at(size, tau, res, mw, pos, (size[0] // 2 - 5, 1, 4))
    rays = np.array([_axis_point(L, tau, res) for L in lens], dtype=np.int64)  # (sensor at (1, 1, 1) mm: zero y / z components)
    near = np.array([[sx + d - 7, 2, 0] for d in dists], dtype=np.int64)
    pad = np.tile(np.array([[0, 10 ** 8, 0]], dtype=np.int64), (n - len(rays) - len(near), 1))
    pts = np.concatenate([rays, near, pad]).astype(np.int32)
    assert pts.shape[0] == n
    pr = ray_predicates(pts, sensor, res, tau, view.size_, pos)
    assert pr["ok"].sum() == len(rays) + len(near)
    st, fn = pr["steps"], pr["fan"]
    assert st[0] == 1 << Sb and st[1] == (1 << Sb) + 1
    if fn[0] <= (1 << F) - 1:
        assert pr["in_key"][0] and not pr["in_key"][1]
    else:
        # (a ray of 2^S steps carries a fan of about 2^S / 328 + 1 whatever res is: below the widest split the fan field is
        # full first, and the step edge is only ever reached by rays the fan edge has already sent down the piecewise route)
        assert Sb < 16 or F < 8
        assert not pr["in_key"][0] and not pr["in_key"][1]
    if F < 8:
        assert fn[2] == (1 << F) - 1 and fn[3] == 1 << F and st[2] <= 1 << Sb and st[3] <= 1 << Sb
        assert pr["in_key"][2] and not pr["in_key"][3]
    dropped = pr["ok"] & ~pr["in_widest"]
    expect = dropped.any()
    assert dropped.any() == (Sb == 16)  # beyond 2^16 steps only the error is left
    oracle_pts = np.ascontiguousarray(pts[~dropped])
    # (a dropped ray: one scan, its error taken by the stats; an exact one: a second update on top)
    scans = [pts] if expect else [pts, pts]
    run_case(view, t, oa, on, scans, sensor, res, tau, mw, expect_error=ERR_RANGE_BIT if expect else 0,
             oracle_scans=[oracle_pts] * len(scans))
    check_registration(t, oa, np.ascontiguousarray(pts[pr["ok"] & ~dropped]), res)


ERR_RANGE_BIT = 2  # the device's error bit for a ray outside the key range (tsdf_scatter.h: ERR_RANGE)


# ---------------------------------------------------------------- 5: key-range rays at the set-up's workgroup edges
@pytest.mark.parametrize("where", [1, 63, 64, 255, 10_000, 19_999])
def test_key_range_ray_in_any_setup_block_is_repeated(where):
    """one ray beyond the key split of a 20 000-point scan (fan 128 > 127: S 16, F 7) at ray index 1, 63, 64, 255 -- workgroup 0 of
    the set-up pass, which used to clear the abort word while the other workgroups set it --, a middle and the last workgroup:
    the scan is repeated in pieces every time and comes out exact"""
    res, tau, mw, n = 2, 40, 640, 20_000
    Sb, F = rec_format(n)
    assert (Sb, F) == (16, 7)
    sensor = (0, 0, 0)
    L = _fan_edge_len(F) + 1
    far = _axis_point(L, tau, res)
    d = int(far[0])
    size, pos = (d // res + 31, 9, 9), (d // res // 2, 0, 0)
    view, t, oa, on = _pair_at(size, tau, res, mw, pos, (3, 4, 5))
    rng = np.random.default_rng(where)
    pts = np.tile(np.array([[0, 10 ** 8, 0]], dtype=np.int64), (n, 1))
    # ordinary rays a few hundred millimetres long everywhere else, so that every workgroup has work
    idx = rng.choice(n, 3000, replace=False)
    pts[idx] = np.stack([rng.integers(20, 300, 3000), rng.integers(-7, 8, 3000), rng.integers(-7, 8, 3000)], axis=1)
    pts[where] = far
    pts = pts.astype(np.int32)
    pr = ray_predicates(pts, sensor, res, tau, view.size_, pos)
    assert pr["ok"][where] and not pr["in_key"][where] and pr["in_widest"][where]
    assert pr["ok"].sum() > 2500 and (~pr["in_key"][pr["ok"]]).sum() == 1  # that ray alone is beyond the split
    run_case(view, t, oa, on, [pts], sensor, res, tau, mw)
    assert np.count_nonzero(oa.data != O.pack(tau, 0)) > 100
    check_registration(t, oa, np.ascontiguousarray(pts[pr["ok"]]), res)
