"""Scan pre-processing at the edges of its float arithmetic and of its hash table, the parts that need no GPU: the C oracle is pinned to
the numpy restatement (test_preprocess.numpy_preprocess) on the inputs that tests/test_gpu_preprocess_scale.py then feeds to the device,
and the premises of the probe-adversarial clouds are checked."""
import numpy as np
import pytest

import oracle_lib as O
from scan_clouds import POSES, numpy_preprocess
from scan_clouds import BELOW_F03, DENORMAL, EDGE_RES, F03, PRE_COORD_LIMIT, _M64, _candidate_voxels, edge_cloud, pre_key, pre_mix, probe_adversarial_points


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
