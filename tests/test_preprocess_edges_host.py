"""Scan pre-processing at the edges of its float arithmetic and of its hash table, the parts that need no GPU: the C oracle is pinned to
the numpy restatement (test_preprocess.numpy_preprocess) on the inputs that tests/test_gpu_preprocess_scale.py then feeds to the device,
and the premises of the probe-adversarial clouds are checked."""
import numpy as np
import pytest

import oracle_lib as O
from test_preprocess import POSES, numpy_preprocess

EDGE_RES = [1, 25, 33, 1000, 4096]
F03 = np.float32(0.3)                               # 0.300000011920929: above the double 0.3, so it alone keeps a point
BELOW_F03 = np.nextafter(F03, np.float32(0))        # 0.2999999821186066: below the double 0.3
DENORMAL = np.float32(1e-40)


def edge_values(res):
    """float32 coordinates in metres that exercise every branch of floor(x * 1000 / res) * res + res / 2 for this res"""
    f = np.float32
    rng = np.random.default_rng(1000 + res)
    v = [f(0.0), f(-0.0), DENORMAL, -DENORMAL, f(1e-45), f(-1e-45), F03, BELOW_F03, -F03, f(0.1), f(1.0), f(-1.0)]
    # exact negative (and positive) multiples of res: -j * res metres is -1000 j res mm without a rounding (res <= 4096, j <= 5)
    v += [f(s * j * res) for j in range(1, 6) for s in (-1, 1)]
    # -j * res mm, where float32(j res / 1000) * 1000 lands back on the integer (test_edge_cloud_holds_what_it_promises counts them),
    # and its float32 neighbours, which fall into the voxels on either side of the border
    for j in (1, 2, 3, 7, 10, 40, 333):
        x = f(-j * res / 1000.0)
        v += [x, np.nextafter(x, f(0)), np.nextafter(x, f(-np.inf)), -x]
    # beyond 2^24 mm: x * 1000, the quotient, the product and the sum each round; up to 2.0e9 mm (2^31 is 2.147e9)
    big = np.exp(rng.uniform(np.log(16778.0), np.log(2.0e6), size=60)).astype(f)
    v += list(big) + list(-big) + [f(16777.216), f(16777.218), f(2.0e6), f(-2.0e6), f(1.9999e6), f(65.0), f(-65.5)]
    return np.array(v, dtype=f)


def edge_cloud(res, stride=3):
    """At most 2000 points: every edge value on every axis beside two ordinary coordinates, random triples of edge values, and the
    points that decide the near test.  Every |x * 1000| stays below 2^31."""
    f = np.float32
    v = edge_values(res)
    rng = np.random.default_rng(2000 + res)
    pts = []
    for x in v:
        pts += [(x, f(1.0), f(2.0)), (f(1.0), x, f(2.0)), (f(2.0), f(-1.0), x), (x, x, x)]
    pts += [tuple(t) for t in v[rng.integers(0, len(v), size=(1100, 3))]]
    pts += [(F03, f(0.0), f(0.0)), (f(0.0), F03, f(-3.0)), (f(-1e6), f(-0.0), F03),        # kept by one coordinate
            (BELOW_F03, BELOW_F03, BELOW_F03), (BELOW_F03, f(0.1), f(-0.0)),                 # dropped
            (BELOW_F03, BELOW_F03, F03), (f(-0.0), f(-0.0), f(-0.0)), (DENORMAL, -DENORMAL, DENORMAL)]
    a = np.zeros((len(pts), stride), dtype=f)
    a[:, :3] = np.array(pts, dtype=f)
    a = a[rng.permutation(len(a))]
    a = np.concatenate([a, a[:150]])  # and some exact duplicates, later in the cloud
    assert len(a) <= 2000
    return a


@pytest.mark.parametrize("res", EDGE_RES)
def test_edge_cloud_holds_what_it_promises(res):
    f = np.float32
    a = edge_cloud(res)[:, :3]
    mm = a * f(1000.0)
    assert np.all(np.isfinite(a)) and np.abs(mm.astype(np.float64)).max() < 2.0 ** 31 - 2 * 4096
    on_border = (mm < 0) & (np.fmod(mm.astype(np.float64), res) == 0)
    assert on_border.sum() >= 20                                                   # exact negative multiples of res
    assert (np.signbit(a) & (a == 0)).any() and ((a != 0) & (np.abs(a) < np.finfo(f).tiny)).any()   # -0.0, denormals
    assert float(F03) > 0.3 > float(BELOW_F03) and (a == F03).any() and (a == BELOW_F03).any()
    assert ((np.abs(mm) > 2.0 ** 24) & (np.abs(mm) <= 2.0e9)).sum() >= 300         # beyond 2^24 mm
    assert np.abs(mm).max() >= 1.99e9


@pytest.mark.parametrize("res", EDGE_RES)
def test_oracle_matches_numpy_restatement_at_the_float_edges(res):
    """res 1, 25 and 33 are odd (res / 2 truncates), 1000 and 4096 are the large even ones; the coordinates are those of
    edge_values.  Every |x * 1000| is kept below 2^31: beyond it the reference's float -> int conversion is undefined behaviour,
    and a GPU (which saturates) and the host CPU (which returns 0x80000000) legitimately differ, so nothing there can be pinned."""
    cloud = edge_cloud(res)
    for pose in POSES:
        got = O.preprocess(cloud, pose, res)
        want = numpy_preprocess(cloud, pose, res)
        assert np.array_equal(got, want)
        assert 300 < len(got) < len(cloud)
    # under the identity a kept point is its voxel centre j res + res / 2 (integer division) -- where the fixed-point product does
    # not wrap, i.e. within +-65 m
    small = O.preprocess(cloud[(np.abs(cloud[:, :3]) < 60.0).all(axis=1)], np.eye(4), res)
    assert len(small) > 50 and np.all((small.astype(np.int64) - res // 2) % res == 0)


def test_the_near_test_is_on_the_double_literal():
    f = np.float32
    pts = np.array([[F03, 0, 0], [BELOW_F03, BELOW_F03, BELOW_F03], [BELOW_F03, BELOW_F03, F03], [-0.0, -0.0, -0.0], [-1.0, F03, -1.0],
                    [DENORMAL, 0.31, -DENORMAL]], dtype=f)
    got = O.preprocess(pts, np.eye(4), 50)
    assert got.tolist() == [[325, 25, 25], [275, 275, 325], [-975, 325, -975], [25, 325, -25]]
    assert np.array_equal(got, numpy_preprocess(pts, np.eye(4), 50))


# ---------------------------------------------------------------------------------------------------------------- the hash table
PRE_COORD_LIMIT = 1 << 20
_M64 = (1 << 64) - 1


def pre_mix(x):
    """pre_mix of warpsense_amd/csrc/scan_preprocess.hip on a uint64 array"""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def pre_key(q):
    """the 63-bit key of an (n, 3) integer point: three coordinates plus 2^20, shifted by 42 and 21"""
    u = (np.asarray(q, dtype=np.int64) + PRE_COORD_LIMIT).astype(np.uint64)
    return (u[:, 0] << np.uint64(42)) | (u[:, 1] << np.uint64(21)) | u[:, 2]


def _candidate_voxels():
    ix, iy, iz = np.meshgrid(np.arange(8, 136), np.arange(8, 136), np.arange(8, 24), indexing="ij")
    return np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(np.int64)


def probe_adversarial_points(slots, n, last):
    """n distinct points in metres, (n, 3) float32, whose hash keys all have their home slot in the last `last` slots of a table of
    `slots` entries -- under the identity pose and a map resolution of 50.  The points are the centres of the voxels 8..135 x
    8..135 x 8..23 (in x-major order, so none is dropped as near: 425 mm and more on every axis).

    THIS HELPER MIRRORS THE KERNEL'S HASH: pre_mix and the key packing above restate pre_mix and pre_transform_insert of
    warpsense_amd/csrc/scan_preprocess.hip (home slot = low bits of pre_mix(key)).  Nothing on the device can tell a test that they
    have drifted apart -- the output of the pre-processor does not depend on where a key sits -- so if the hash or the key changes,
    this helper has to change with it, or the clouds built from it quietly stop being adversarial."""
    assert slots & (slots - 1) == 0 and 0 < last <= slots
    vox = _candidate_voxels()
    q = vox * 50 + 25                                   # the integer point of a voxel centre under the identity
    home = pre_mix(pre_key(q)) & np.uint64(slots - 1)
    sel = np.nonzero(home >= np.uint64(slots - last))[0]
    if len(sel) < n:
        raise ValueError(f"only {len(sel)} candidate voxels are homed in the last {last} of {slots} slots, {n} wanted")
    return (q[sel[:n]].astype(np.float64) / 1000.0).astype(np.float32)


def test_mix_restatement_on_known_values():
    """the 64-bit finaliser in python integers, step by step, against the numpy form"""
    def mix(x):
        x ^= x >> 33
        x = (x * 0xff51afd7ed558ccd) & _M64
        x ^= x >> 33
        x = (x * 0xc4ceb9fe1a85ec53) & _M64
        return x ^ (x >> 33)
    xs = [0, 1, 2 ** 63 - 1, (1048576 + 425) << 42 | (1048576 + 425) << 21 | (1048576 + 425), 0x0123456789abcdef]
    assert pre_mix(np.array(xs, dtype=np.uint64)).tolist() == [mix(x) for x in xs]
    assert mix(0) == 0 and mix(1) == 0xb456bcfc34c2cb2c
    assert pre_key(np.array([[-PRE_COORD_LIMIT + 1, 0, PRE_COORD_LIMIT - 1]])).tolist() == [(1 << 42) | (PRE_COORD_LIMIT << 21) | (2 * PRE_COORD_LIMIT - 1)]


def test_probe_adversarial_premises():
    """enough candidates exist for the clouds of test_gpu_preprocess_scale.py, and the oracle keeps all of them in input order"""
    q = _candidate_voxels() * 50 + 25
    home = (pre_mix(pre_key(q)) & np.uint64(1023)).astype(np.int64)
    assert (home >= 1016).sum() == 2030 and (home == 1023).sum() == 209
    for n, last in [(512, 8), (200, 1)]:
        pts = probe_adversarial_points(1024, n, last)
        assert pts.shape == (n, 3) and pts.dtype == np.float32 and pts.min() >= np.float32(0.425)
        got = O.preprocess(pts, np.eye(4), 50)
        assert len(got) == n == len({tuple(p) for p in got.tolist()})
        assert np.array_equal(got, np.round(pts.astype(np.float64) * 1000.0).astype(np.int32))  # all n, input order, the voxel centres
        assert np.array_equal(got, numpy_preprocess(pts, np.eye(4), 50))
        h = (pre_mix(pre_key(got)) & np.uint64(1023)).astype(np.int64)
        assert h.min() >= 1024 - last
    with pytest.raises(ValueError):
        probe_adversarial_points(1024, 210, 1)
