"""ws_scan_preprocess* where the small clouds of test_preprocess.py and test_gpu_sweep.py do not reach: more workgroup counts than the
scan kernel has threads (per >= 2 from 262 145 points), probe chains that wrap past the end of the hash table, a table at load 0.5,
one voxel fought over by hundreds of workgroups, buffers left dirty by a larger call, and the float arithmetic of the snap at odd
resolutions and beyond 2^24 mm.

Every expectation is the C oracle's (oracle_lib.preprocess); for sweeps it is the host model preprocess_sweep_host, which
test_sweep_host.py pins to the oracle.  Full arrays, order included, no tolerance; every cloud goes in from the host and as a device
tensor."""
import numpy as np
import pytest

import oracle_lib as O
from scan_clouds import both_routes as both_routes_sweep
from scan_clouds import POSES, make_cloud
from scan_clouds import EDGE_RES, edge_cloud, probe_adversarial_points
from scan_clouds import rigid

pytestmark = pytest.mark.gpu

BIG = 1_000_000
SCAN_SIZES = [262_144, 262_145, 524_289, 1_000_000]  # 1024, 1025, 2049, 3907 workgroups: per = 1, 2, 3, 4 in pre_scan_kernel
N_SWEEP, SWEEP_COLUMNS, SWEEP_ROWS = 262_400, 1025, 256  # 1025 workgroups


@pytest.fixture(scope="module")
def pre():
    import warpsense_amd as W
    p = W.ScanPreprocessor(BIG)
    yield p
    p.close()


def both_routes(pre, cloud, pose, res):
    """the plain call with the cloud on the host and on the device; the two must agree, the first is returned"""
    import torch
    host = pre.preprocess(cloud, pose, res)
    n_host, got = len(host), host.to_host()
    dev = pre.preprocess(torch.from_numpy(np.array(cloud)).cuda(), pose, res)  # (a contiguous, writable copy)
    assert len(dev) == n_host == len(got) and np.array_equal(dev.to_host(), got)
    assert got.shape == (n_host, 3) and got.dtype == np.int32
    return got


# ------------------------------------------------------------------------------------------------------------------------ clouds
def distinct_points(n, seed):
    """n distinct points, none of them near: centres of 50 mm voxels within +-30 m, in shuffled order.  Two centres are at least
    50 mm apart and a rigid pose moves each by less than 2 mm from its exact image (fixed-point matrix, truncating division), so the
    n transformed integer points are distinct too."""
    rng = np.random.default_rng(seed)
    code = np.unique(rng.integers(0, 1200 ** 3, size=n + n // 4 + 64))  # (x, y, z) voxel index + 600, as one number
    idx = np.stack([code // 1200 ** 2, code // 1200 % 1200, code % 1200], axis=1) - 600
    idx = idx[~((idx < 6).all(axis=1))]  # index 6 is the voxel from 300 mm: below it a coordinate is under 0.3
    assert len(idx) >= n
    idx = idx[rng.permutation(len(idx))[:n]]
    return ((idx * 50 + 25).astype(np.float64) / 1000.0).astype(np.float32)


def count_distinct(cloud):
    idx = np.floor(cloud.astype(np.float64) * 20.0).astype(np.int64) + 600  # voxel centres: the index is exact
    assert idx.min() >= 0 and idx.max() < 1200
    return len(np.unique((idx[:, 0] * 1200 + idx[:, 1]) * 1200 + idx[:, 2]))


def repeated_points(n, seed, distinct=5000):
    rng = np.random.default_rng(seed)
    base = distinct_points(distinct, seed + 1)
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=n - distinct)])
    return base[pick[rng.permutation(n)]]


def dropped_run(blocks):
    """the long run of dropped workgroups: 1100 wherever block_cloud can place it -- a kept workgroup on either side and the kept
    last one need 1104 workgroups, so 524 289 and 1 000 000 points get it -- and half the cloud at 1024 and 1025 workgroups"""
    return 1100 if blocks >= 1104 else blocks // 2


def block_cloud(n, seed):
    """make_cloud with whole 256-point workgroups made near (dropped) in runs of 1..24 that alternate with kept runs, one dropped run
    of dropped_run(blocks) workgroups, and the last workgroup (partial where 256 does not divide n) kept.  Returns the cloud and the
    per-workgroup dropped flags."""
    rng = np.random.default_rng(seed)
    blocks = (n + 255) // 256
    dropped = np.zeros(blocks, dtype=bool)
    b, state = 0, False
    while b < blocks:
        run = int(rng.integers(1, 25))
        dropped[b:b + run] = state
        b, state = b + run, not state
    long_run = dropped_run(blocks)
    start = int(rng.integers(1, blocks - long_run - 1))
    dropped[start:start + long_run] = True
    dropped[start - 1] = dropped[start + long_run] = False
    dropped[-1] = False
    cloud = make_cloud(n, seed)
    near = np.repeat(dropped, 256)[:n]
    cloud[near, :3] = rng.uniform(-5.0, 0.29, size=(int(near.sum()), 3)).astype(np.float32)
    return cloud, dropped


_CLOUDS, _DROPPED = {}, {}


def scale_case(kind, n):
    """(cloud, the oracle's points at POSES[1] and res 50), computed once per module run and never written to"""
    if (kind, n) not in _CLOUDS:
        if kind == "blocks":
            cloud, _DROPPED[n] = block_cloud(n, n + 11)
        else:
            cloud = distinct_points(n, n) if kind == "distinct" else repeated_points(n, n + 7)
        cloud.setflags(write=False)
        want = O.preprocess(cloud, POSES[1], 50)
        want.setflags(write=False)
        _CLOUDS[kind, n] = (cloud, want)
    return _CLOUDS[kind, n]


# ------------------------------------------------------------------------------------------------------- a. past one scan pass
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_all_points_distinct_and_kept(pre, n):
    """every workgroup keeps 256 points: the offsets are multiples of 256 up to n -- the hand-over between the counts of one scan
    thread (per >= 2 from 262 145 points on) and the bound of the last thread show in every output row"""
    cloud, want = scale_case("distinct", n)
    assert len(want) == n
    got = both_routes(pre, cloud, POSES[1], 50)
    assert len(got) == n and np.array_equal(got, want)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_five_thousand_voxels_repeated(pre, n):
    """most workgroups keep nothing or a point or two, and every kept point has copies in hundreds of workgroups"""
    cloud, want = scale_case("repeated", n)
    assert len(want) == count_distinct(cloud) == 5000 and len(want) < 0.02 * n
    assert np.array_equal(both_routes(pre, cloud, POSES[1], 50), want)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_runs_of_dropped_workgroups(pre, n):
    """runs of workgroups that keep nothing, one of them 1100 long at 524 289 and 1 000 000 points (per 3 and 4: over 270 scan
    threads in a row sum zero) and half the cloud at 262 144 and 262 145, which have only 1024 and 1025 workgroups (per 1 and 2: 512
    and 256 such threads); the last workgroup kept"""
    cloud, want = scale_case("blocks", n)
    dropped = _DROPPED[n]
    runs = np.diff(np.nonzero(np.diff(np.concatenate([[0], dropped.astype(np.int8), [0]])))[0])[::2]
    assert runs.max() >= dropped_run(len(dropped)) and len(runs) > 10 and not dropped[-1]
    assert 0.1 * n < len(want) < 0.9 * n
    assert np.array_equal(both_routes(pre, cloud, POSES[1], 50), want)


# --------------------------------------------------------------------------------------- b. first occurrence under contention
def test_mirrored_cloud_keeps_the_first_half(pre):
    """concat(A, A[::-1]): point j of A meets its copy at index 2 n - 1 - j, so for the early points the two copies sit in
    workgroups far apart and for the middle ones in neighbouring workgroups"""
    A = distinct_points(150_000, 5)
    want_A = O.preprocess(A, POSES[1], 50)
    assert len(want_A) == len(A)
    cloud = np.concatenate([A, A[::-1]])
    want = O.preprocess(cloud, POSES[1], 50)
    assert np.array_equal(want, want_A)
    assert np.array_equal(both_routes(pre, cloud, POSES[1], 50), want_A)


def test_one_voxel_three_hundred_thousand_times(pre):
    cloud = np.tile(np.array([[2.0, -3.0, 1.0]], dtype=np.float32), (300_000, 1))
    want = O.preprocess(cloud, POSES[1], 50)
    assert len(want) == 1
    got = both_routes(pre, cloud, POSES[1], 50)
    assert got.shape == (1, 3) and np.array_equal(got, want)


def test_first_copy_at_index_zero_among_a_thousand_distinct_points(pre):
    """index 0 holds the first copy of a point that fills all but 2000 of the other places; 1000 distinct points sit at two random
    places each, so their first copies are anywhere in launch order while 1172 workgroups hammer the one word of the common point"""
    rng = np.random.default_rng(17)
    n = 300_000
    cloud = np.tile(np.array([[2.0, -3.0, 1.0]], dtype=np.float32), (n, 1))
    others = distinct_points(1000, 23)
    places = 1 + rng.permutation(n - 1)[:2000]
    cloud[places[:1000]] = others
    cloud[places[1000:]] = others[rng.permutation(1000)]
    want = O.preprocess(cloud, POSES[1], 50)
    assert len(want) == 1001 and np.array_equal(want[0], O.preprocess(cloud[:1], POSES[1], 50)[0])
    assert np.array_equal(both_routes(pre, cloud, POSES[1], 50), want)


# ------------------------------------------------------------------------------------------------------- c. capacity and load
@pytest.mark.parametrize("cap", [1, 255, 256, 257, 512, 4096])
def test_full_preprocessor(cap):
    """n == cap, all points distinct; the table has max(1024, 2 cap) slots, so 512 and 4096 fill it to exactly one half"""
    import warpsense_amd as W
    p = W.ScanPreprocessor(cap)
    try:
        cloud = distinct_points(cap, 100 + cap)
        want = O.preprocess(cloud, POSES[1], 50)
        assert len(want) == cap
        assert np.array_equal(both_routes(p, cloud, POSES[1], 50), want)
        with pytest.raises(W.WsError):
            p.preprocess(np.ones((cap + 1, 3), dtype=np.float32), POSES[1], 50)
        assert np.array_equal(both_routes(p, cloud[::-1], POSES[1], 50), want[::-1])
    finally:
        p.close()


@pytest.mark.parametrize("n,last", [(512, 8), (200, 1)])
def test_probe_chains_wrap_past_the_end_of_the_table(n, last):
    """a 512-point preprocessor has 1024 slots.  512 keys homed in slots 1016..1023: all but the first few probe on through slot 0,
    the last of them some 500 slots far, at load 0.5.  200 keys homed in slot 1023 itself: every one but the first wraps at its first
    step.  (Which slots the keys are homed in is test_preprocess_edges_host.probe_adversarial_points' restatement of the hash.)"""
    import warpsense_amd as W
    p = W.ScanPreprocessor(512)
    try:
        cloud = probe_adversarial_points(1024, n, last)
        want = O.preprocess(cloud, np.eye(4), 50)
        assert len(want) == n
        assert np.array_equal(both_routes(p, cloud, np.eye(4), 50), want)
        # the other way round the keys settle in other slots of the same chains; with 200 points there is room for a copy of each,
        # which probes its key's chain again and has to find it
        twice = np.concatenate([cloud[::-1], cloud])[:512]
        assert np.array_equal(both_routes(p, twice, np.eye(4), 50), O.preprocess(twice, np.eye(4), 50))
    finally:
        p.close()


def test_default_capacity():
    import torch
    import warpsense_amd as W
    p = W.ScanPreprocessor(0)
    try:
        cloud = make_cloud(131_073, seed=9)
        want = O.preprocess(cloud[:131_072], POSES[1], 50)
        assert np.array_equal(both_routes(p, cloud[:131_072], POSES[1], 50), want)
        with pytest.raises(W.WsError):
            p.preprocess(cloud, POSES[1], 50)
        with pytest.raises(W.WsError):
            p.preprocess(torch.from_numpy(cloud).cuda(), POSES[1], 50)
        assert np.array_equal(both_routes(p, cloud[1:], POSES[1], 50), O.preprocess(cloud[1:], POSES[1], 50))
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------------------------------- d. reuse
def sweep_case(rule):
    """the sweep cloud (5 floats per point, a time in the last), its 1025 poses and the host model's points"""
    import warpsense_amd as W
    key = ("sweep", tuple(sorted(rule.items())))
    if key not in _CLOUDS:
        cloud = make_cloud(N_SWEEP, seed=31, stride=5)
        rng = np.random.default_rng(32)
        cloud[:, 4] = rng.uniform(-0.02, 1.02, size=N_SWEEP).astype(np.float32)
        # (left writable: test_gpu_sweep.both_routes hands the array itself to torch.from_numpy, which warns of a read-only one)
        poses = W.sweep_poses(POSES[1], rigid(300.0 * np.cos(0.4), 300.0 * np.sin(0.4), 0.0, 8.0), SWEEP_COLUMNS)
        want = W.preprocess_sweep_host(cloud, poses, 50, **rule)
        want.setflags(write=False)
        _CLOUDS[key] = (cloud, poses, want)
    return _CLOUDS[key]


@pytest.mark.parametrize("route", ["host", "device"])
def test_one_preprocessor_large_small_empty_large(pre, route):
    """slot_of, tmp, wg_count, wg_off and out are not cleared between calls: after 1 000 000 points they hold 3907 workgroups' worth
    of another cloud, and every reader has to stop at the n of its own call.  The whole sequence runs with the clouds on the host
    (ws_scan_preprocess, ws_scan_preprocess_sweep) and again with them on the device (the _dev entry points)."""
    import torch
    import warpsense_amd as W

    def fresh(call, cloud):
        p = W.ScanPreprocessor(BIG)
        try:
            out = call(p, cloud)
            return len(out), out.to_host()
        finally:
            p.close()

    def plain(p, cloud):
        return p.preprocess(cloud, POSES[1], 50)

    big, want_big = scale_case("blocks", BIG)
    mid, want_mid = scale_case("distinct", 262_145)
    sweep, poses, want_sweep = sweep_case({"columns": SWEEP_COLUMNS, "ring_major": True})
    steps = [("1 000 000", plain, big, want_big),
             ("5", plain, mid[:5], want_mid[:5]),
             ("0", plain, mid[:0], want_mid[:0]),
             ("262 145", plain, mid, want_mid),
             ("257", plain, big[:257], O.preprocess(big[:257], POSES[1], 50)),
             ("sweep", lambda p, cloud: p.preprocess_sweep(cloud, poses, 50, columns=SWEEP_COLUMNS, ring_major=True), sweep, want_sweep),
             ("1 000 000 again", plain, big, want_big)]
    for name, call, cloud, want in steps:
        if route == "device":
            cloud = torch.from_numpy(np.array(cloud)).cuda()  # (a contiguous, writable copy)
        out = call(pre, cloud)
        n_got, got = len(out), out.to_host()
        n_fresh, got_fresh = fresh(call, cloud)
        assert n_got == n_fresh == len(want), name
        assert got.shape == (len(want), 3) and np.array_equal(got, got_fresh) and np.array_equal(got, want), name
        if name == "0":
            assert n_got == 0 and got.shape == (0, 3)


# ------------------------------------------------------------------------------------------- e. the sweep form past one scan pass
@pytest.mark.parametrize("ring_major", [True, False])
def test_sweep_by_index_past_one_scan_pass(pre, ring_major):
    """262 400 points = 1025 columns x 256 rows = 1025 workgroups (per == 2), one pose per column.  Column-major, a workgroup is a
    column and takes one row of the pose table; ring-major, its lanes take 256 different rows."""
    cloud, poses, want = sweep_case({"columns": SWEEP_COLUMNS, "ring_major": ring_major})
    assert N_SWEEP == SWEEP_COLUMNS * SWEEP_ROWS and len(poses) == 1025 and 0.5 * N_SWEEP < len(want) < N_SWEEP
    got = both_routes_sweep(pre, cloud, poses, 50, columns=SWEEP_COLUMNS, ring_major=ring_major)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, pre.preprocess(cloud, poses[-1], 50).to_host())  # (the bins matter)


def test_sweep_by_time_past_one_scan_pass(pre):
    cloud, poses, want = sweep_case({"time_field": 4})
    assert 0.5 * N_SWEEP < len(want) < N_SWEEP
    assert np.array_equal(both_routes_sweep(pre, cloud, poses, 50, time_field=4), want)


# ---------------------------------------------------------------------------------------------------- f. snapping on the device
@pytest.mark.parametrize("res", EDGE_RES)
def test_snap_at_the_float_edges(pre, res):
    """the clouds of test_preprocess_edges_host.py: odd res (res / 2 truncates), -0.0, denormals (the case pins that the kernel
    keeps float32 denormals, as the host does: flushed to zero, -1e-40 would move from the voxel below zero to the one above and
    miss the oracle), the two floats around 0.3, and coordinates beyond 2^24 mm, where floor(p / res) * res + half rounds at every
    step -- a contracted multiply-add would round once and land elsewhere"""
    for stride in (3, 4):
        cloud = edge_cloud(res, stride=stride)
        for pose in (np.eye(4, dtype=np.float32), POSES[2]):
            want = O.preprocess(cloud, pose, res)
            assert len(want) > 300
            assert np.array_equal(both_routes(pre, cloud, pose, res), want)
