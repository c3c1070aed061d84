"""Every device route to the registration sums h, g, e, c on every case of tests/reg_cases.py: windows that are shifted, wrapped
and tiny, clouds with a named edge set, poses whose int32 transform wraps -- against the CPU oracle, bit for bit.

Routes with one evaluation: the pass kernel (perform_registration, both flags), the resident server (asked twice: the second
answer comes from cached voxels; then at other poses: the cache is invalid), the shard ranges (ws_reg_accumulate_dev, first > 0)
and the batch kernel with max_iterations = 0.  Loops: register_cloud as one resident launch and as one launch per iteration, the
shard `iterate` route, and register_cloud_batch with both kernel variants (WS_REG_BATCH_VARIANT, read when the handle is created).

tests/test_reg_cases_host.py proves on the oracle alone that the cases exercise what they claim.

Measured on an MI355X, oracle included: the whole file takes 3.1 s; the slowest case is test_single_evaluation_routes[A_shifted-1]
with 0.20 s (it builds the first map), test_loops[A_shifted-1] takes 0.12 s, test_third_stage_of_accumulate_points[262145] 0.10 s.
"""
import numpy as np
import pytest

import oracle_lib as O
import reg_cases as RC
from reg_scenes import check_batch_equals_single
from reg_scenes import _server, pose_error
from reg_scenes import _OracleLoop

pytestmark = pytest.mark.gpu

ARGS = (RC.IT_WEIGHT_GRADIENT, RC.EPSILON)
WINDOW_COUNTS = [(cid, n) for cid in RC.IDS for n in RC.COUNTS_ALL]
LOOP_COUNTS = WINDOW_COUNTS + [RC.LOOP_THAT_EMPTIES]
_ids = lambda v: f"{v[0]}_{RC.WINDOWS[v[0]]['name']}-{v[1]}"


class _Scene:
    """what check_batch_equals_single asks of a TSDFRegistration: .reg_ and .tsdf()"""

    def __init__(self, tsdf, reg_cuda):
        self.tsdf_, self.reg_ = tsdf, reg_cuda

    def tsdf(self):
        return self.tsdf_


def _window_e_on_the_device(c):
    """LocalMap + TSDFRegistration, one update with the scan, three shift_map calls; both downloads equal the host mirror"""
    import torch
    import warpsense_amd as W
    size, res = RC.WINDOWS["E"]["size"], c.res
    lm = W.LocalMap(*size, RC.E_TAU, 0)
    params = W.Params(W.MapParams(resolution=res, max_distance=RC.E_TAU / 1000.0, max_weight=RC.E_MAX_WEIGHT // 64,
                                  size=tuple(s * res / 1000.0 for s in size)))
    reg = W.TSDFRegistration(params, lm)
    reg.update_tsdf(torch.from_numpy(RC.e_scan()).cuda(), pose=np.eye(4, dtype=np.float32))
    for new_pos in RC.e_positions():
        reg.shift_map(tuple(int(v) for v in new_pos))
    for which, want in ((reg.tsdf().avg_map(), c.om.data), (reg.tsdf().new_map(), None)):
        host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
        which.to_host(host)
        assert list(host.pos_) == list(c.om.pos) and list(host.offset_) == list(c.om.offset) and list(host.size_) == list(c.om.size)
        if want is not None:
            assert np.array_equal(host.data_, want)
        else:  # new_map is the default entry everywhere: only its window moves
            assert (host.data_ == W.pack_entry(RC.E_TAU, 0)).all()
    return reg, reg.tsdf(), reg.reg_


class _Windows:
    """one map and one RegistrationCuda per window, and three more handles for the ranks of the shard routes"""

    def __init__(self):
        self.made, self.ranks, self.keep = {}, [], []

    def get(self, cid):
        import warpsense_amd as W
        if cid not in self.made:
            c = RC.case(cid)
            if cid == "E":
                owner, tsdf, rc = _window_e_on_the_device(c)
                self.keep.append(owner)
            else:
                view = W.DeviceMap(c.om.size.copy(), c.om.offset.copy(), c.om.data.copy(), c.om.pos.copy())
                tsdf = W.TSDFCuda(view, 1000, 640, c.map_resolution)
                rc = W.RegistrationCuda(None, tsdf.ctx)
            self.made[cid] = (c, tsdf, rc)
        return self.made[cid]

    def rank_handles(self, tsdf, world):
        import warpsense_amd as W
        while len(self.ranks) < world:
            self.ranks.append(W.RegistrationCuda(None, tsdf.ctx))
        return self.ranks[:world]

    def close(self):
        for c, tsdf, rc in self.made.values():
            _server(rc, enable=0)
            rc.close()
        for rc in self.ranks:
            rc.close()
        for c, tsdf, rc in self.made.values():
            tsdf.close()
        ctxs = {id(t.ctx): t.ctx for _, t, _ in self.made.values()}
        for ctx in ctxs.values():
            ctx.restore_torch_stream()  # (HipGnBackend moved torch to a stream of its own)


@pytest.fixture(scope="module")
def windows():
    w = _Windows()
    yield w
    w.close()


def _same(got, want, what):
    h, g, e, c = got
    ho, go, eo, co = want
    assert (int(e), int(c)) == (int(eo), int(co)), (what, e, eo, c, co)
    assert np.array_equal(g, go), (what, g, go)
    assert np.array_equal(h, ho), (what, np.argwhere(h != ho)[:4])


def _flat(want):
    h, g, e, c = want
    return np.concatenate([h.T.reshape(-1), g, [e, c]]).astype(np.int64)


def _pass_kernel(c, tsdf, rc, q):
    for flags in (0, 1):
        rc.flags = flags
        try:
            for pi, T in enumerate(c.poses):
                _same(rc.perform_registration(tsdf.device_map(), T, c.res), O.reg_iterate(c.om, T, q, c.res, flags), ("pass", flags, pi))
        finally:
            rc.flags = 0


def _served(c, tsdf, rc, q, want):
    """the resident server: pose 0 twice (the second answer from the cached voxels), then the others (the cache is invalid), then
    pose 0 again; the same sums with the server switched off again"""
    _server(rc, enable=1, idle_us=200000)
    try:
        for pi in (0, 0, 1, 2, 0):
            _same(rc.perform_registration(tsdf.device_map(), c.poses[pi], c.res), want[pi], ("server", pi))
    finally:
        _server(rc, enable=0)


def _shard_ranges(c, tsdf, rc, q, want):
    """ws_reg_accumulate_dev over the ranges of 2 and of 3 ranks (ragged), summed"""
    from warpsense_amd.dist import HipGnBackend, shard_range
    b = HipGnBackend(rc, tsdf, c.res)
    n = len(q)
    for world in (2, 3):
        for pi, T in enumerate(c.poses):
            b.begin(T, 6, *ARGS)
            total = np.zeros(44, dtype=np.int64)
            covered = 0
            for r in range(world):
                first, count = shard_range(n, r, world)
                assert first == covered
                covered += count
                with np.errstate(over="ignore"):
                    total = total + b.accumulate(first, count).cpu().numpy()
            assert covered == n
            assert np.array_equal(total, _flat(want[pi])), ("accumulate", world, pi, np.nonzero(total != _flat(want[pi]))[0])


def _oracle_loop(c, q, max_it):
    T_o, it_o, trace = O.register_cloud(c.om, q, c.poses[1], max_it, *ARGS, c.res, trace_cap=max_it)
    assert it_o >= 1
    last = trace[it_o - 1]
    return T_o, it_o, (last[:36].reshape(6, 6).T, last[36:42], int(last[42]), int(last[43]))


def _loop_modes(c, tsdf, rc, q, limits):
    """register_cloud from the perturbed pose as one resident launch and as one launch per iteration"""
    import warpsense_amd as W
    try:
        for max_it in limits:
            T_o, it_o, sums_o = _oracle_loop(c, q, max_it)
            for mode in (W.WS_REG_LOOP_RESIDENT, W.WS_REG_LOOP_LAUNCHES):
                rc.set_loop(mode)
                T, it = rc.register_cloud(tsdf.device_map(), c.poses[1], max_it, *ARGS, c.res)
                assert it == it_o, (mode, max_it, it, it_o)
                _same(rc.last_sums(), sums_o, ("loop", mode, max_it))
                dt, ang = pose_error(T, T_o)
                assert dt < 1e-4 and ang < 1e-4, (mode, max_it, dt, ang)
                # at most 6 iterations: bit for bit (and so between the two routes)
                assert np.array_equal(T.view(np.uint32), T_o.astype(np.float32).view(np.uint32)), (mode, max_it, np.abs(T - T_o).max())
    finally:
        rc.set_loop(W.WS_REG_LOOP_RESIDENT)


def _shard_iterate_loop(c, tsdf, handles, q, limits):
    """the `iterate` route over the ranges of len(handles) ranks, looped as test_hip_shard_ranges_sum_to_the_whole does"""
    import torch
    from warpsense_amd.dist import HipGnBackend, shard_range
    world, n = len(handles), len(q)
    ranks = []
    for rc in handles:
        rc.prepare_registration(q)
        ranks.append(HipGnBackend(rc, tsdf, c.res))
    spans = [shard_range(n, r, world) for r in range(world)]
    for max_it in limits:
        for b in ranks:
            b.begin(c.poses[1], max_it, *ARGS)
        oracle = _OracleLoop(c.om, q, c.res, c.poses[1], max_it, *ARGS)
        its = 0
        while not oracle.finished():
            want = oracle.sums()
            parts = [b.iterate(first, count).cpu().numpy().copy() for b, (first, count) in zip(ranks, spans)]
            with np.errstate(over="ignore"):
                total = np.sum(parts, axis=0, dtype=np.int64)
            assert np.array_equal(total, want), ("iterate", max_it, its, np.nonzero(total != want)[0])
            tt = torch.from_numpy(total)
            for b in ranks:
                b.sums.copy_(tt)  # the all-reduce
            oracle.update(total)
            its += 1
        for b in ranks:
            b.solve(b.sums)
        fin_o, it_o, T_o = oracle.result()
        assert fin_o and it_o == its
        for b in ranks:
            fin, it, T = b.poll()
            assert fin and it == it_o
            assert np.array_equal(T.view(np.uint32), T_o.view(np.uint32)), ("iterate", max_it, np.abs(T - T_o).max())


@pytest.mark.parametrize("cid,n", WINDOW_COUNTS, ids=[_ids(v) for v in WINDOW_COUNTS])
def test_single_evaluation_routes(windows, cid, n):
    c, tsdf, rc = windows.get(cid)
    q = c.cloud(n)
    rc.prepare_registration(q)
    want = [O.reg_iterate(c.om, T, q, c.res, 0) for T in c.poses]
    assert want[0][3] > 0  # (tests/test_reg_cases_host.py holds the cases to much more)
    _pass_kernel(c, tsdf, rc, q)
    _served(c, tsdf, rc, q, want)
    _shard_ranges(c, tsdf, rc, q, want)
    # the batch kernel with no iteration: e and c are the score at the start pose
    T, it, e, cnt = rc.register_cloud_batch(tsdf.device_map(), np.stack(c.poses), 0, *ARGS, c.res)
    assert np.array_equal(T, np.stack(c.poses)) and not it.any()
    assert [(int(a), int(b)) for a, b in zip(e, cnt)] == [(w[2], w[3]) for w in want]


@pytest.mark.parametrize("cid,n", LOOP_COUNTS, ids=[_ids(v) for v in LOOP_COUNTS])
def test_loops(windows, cid, n):
    c, tsdf, rc = windows.get(cid)
    q = c.cloud(n)
    rc.prepare_registration(q)
    _loop_modes(c, tsdf, rc, q, RC.LOOP_LIMITS)
    _shard_iterate_loop(c, tsdf, windows.rank_handles(tsdf, 3 if n % 2 else 2), q, RC.LOOP_LIMITS)
    if (cid, n) == RC.LOOP_THAT_EMPTIES:
        T, it = rc.register_cloud(tsdf.device_map(), c.poses[1], 6, *ARGS, c.res)
        assert 2 <= it < 6 and rc.last_sums()[3] == 0  # the loop ended because no point was counted


@pytest.mark.parametrize("cid,n", WINDOW_COUNTS, ids=[_ids(v) for v in WINDOW_COUNTS])
def test_batch_kernel_variants(windows, monkeypatch, cid, n):
    """k = 7 start poses through reg_batch_kernel<512, 0> (every point streamed) and <512, 2> (two cached points per lane): each
    equal to the single routes (check_batch_equals_single), both to each other and their scores to the oracle"""
    import warpsense_amd as W
    c, tsdf, rc0 = windows.get(cid)
    q = c.cloud(n)
    poses = c.batch_poses()
    assert len(poses) == 7
    got = {}
    for variant in (0, 1):
        monkeypatch.setenv("WS_REG_BATCH_VARIANT", str(variant))  # read by ws_reg_create
        rc = W.RegistrationCuda(None, tsdf.ctx)
        try:
            rc.prepare_registration(q)
            scene = _Scene(tsdf, rc)
            got[variant] = [check_batch_equals_single(scene, poses, max_it, c.res) for max_it in RC.LOOP_LIMITS]
        finally:
            rc.close()
    for a, b in zip(got[0], got[1]):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    for (T, it, e, cnt), max_it in zip(got[1], RC.LOOP_LIMITS):
        assert (it >= 1).all() and (it <= max_it).all()
        for k in range(len(poses)):
            assert (int(e[k]), int(cnt[k])) == O.reg_iterate(c.om, T[k], q, c.res, 0)[2:], (max_it, k)
            # and the oracle's own loop from that start pose (the host test keeps these loops inside the range of (int)(T * 32768))
            T_o, it_o, _ = O.register_cloud(c.om, q, poses[k], max_it, *ARGS, c.res)
            assert it[k] == it_o and np.array_equal(T[k].view(np.uint32), T_o.astype(np.float32).view(np.uint32)), (max_it, k)


@pytest.mark.parametrize("n", RC.COUNTS_SWITCH)
def test_switch_between_matrix_cores_and_mad_i64(windows, n):
    """131 072 points are one per lane of the resident grid (matrix cores), 131 073 are not (v_mad_i64_i32): loop modes, server
    and shard routes on window A"""
    c, tsdf, rc = windows.get("A")
    q = c.cloud(n)
    rc.prepare_registration(q)
    want = [O.reg_iterate(c.om, T, q, c.res, 0) for T in c.poses]
    assert all(w[3] > 0 for w in want) and want[0][3] > n // 4
    _loop_modes(c, tsdf, rc, q, RC.LOOP_LIMITS_LARGE)
    _served(c, tsdf, rc, q, want)
    _shard_ranges(c, tsdf, rc, q, want)
    _shard_iterate_loop(c, tsdf, windows.rank_handles(tsdf, 3), q, RC.LOOP_LIMITS_LARGE[:1])


@pytest.mark.parametrize("n", RC.COUNTS_THIRD_STAGE)
def test_third_stage_of_accumulate_points(windows, n):
    """beyond two passes of the grid (2 * 256 * 512 = 262 144 points) accumulate_points loops idx += REG_STRIDE: 262 145 points
    have exactly one point there, and it is the cloud's last (so the sums differ from those of 262 144 points)"""
    c, tsdf, rc = windows.get("A")
    q = c.cloud(n)
    rc.prepare_registration(q)  # (ws_reg_prepare grows the point buffer: no limit at this size)
    if n == 262145:
        # the one point of the third stage is counted under the identity: a route that skipped it would be found out
        q[-1] = c.edge[0]
        rc.prepare_registration(q)
        assert O.reg_iterate(c.om, c.poses[0], q, c.res)[3] == O.reg_iterate(c.om, c.poses[0], q[:-1], c.res)[3] + 1
    _pass_kernel(c, tsdf, rc, q)
    _loop_modes(c, tsdf, rc, q, RC.LOOP_LIMITS_LARGE)
