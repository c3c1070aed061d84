"""The world model of tests/window_model.py proved on the CPU: its walks through LocalMap.shift (pinned to the reference by
test_oracle_pins.py::test_kat_ring_buffer_shift), and the walks themselves counted for what they are meant to contain.
tests/test_gpu_map_window.py runs the same walks (same shapes, same seeds) through the device routes."""
import numpy as np
import pytest

from window_host_routes import HostRoute, TAU
from window_model import WALKS
import window_model as M
WS_ERR_INVALID = -1


@pytest.mark.parametrize("size,seed", WALKS)
def test_model_matches_local_map_shift(size, seed):
    import warpsense_amd as W
    walk = M.make_walk(size, seed)
    w = M.run_walk(size, walk, seed, HostRoute(size), W.pack_entry(TAU, 0))
    assert np.all(w.pos == 0)
    assert np.count_nonzero(w.world != w.default_raw) > 0 and np.count_nonzero(w.store != w.default_raw) > 0


@pytest.mark.parametrize("size,seed", WALKS)
def test_walks_contain_what_they_are_meant_to(size, seed):
    """conditions on the INPUTS, counted from the walk itself"""
    walk = M.make_walk(size, seed)
    assert walk == M.make_walk(size, seed)  # deterministic
    pos = np.asarray([(0, 0, 0)] + walk)
    assert np.all(np.abs(np.diff(pos, axis=0)) <= np.asarray(size))  # every step is one the library admits
    cov = M.walk_coverage(size, walk, seed)
    for axis in range(3):
        want = {d for d in (1, size[axis] // 2, size[axis] // 2 + 1, size[axis] - 1, size[axis]) if d >= 1}
        assert want == {d for (a, d) in cov["steps"] if a == axis}
    # each |d| out and back along its axis alone: at least twice
    assert all(n >= 2 for n in cov["steps"].values()), cov["steps"]
    assert cov["diagonal"] >= 3, cov       # three-axis steps
    assert cov["corner"] >= 3, cov         # a corner enters with an earlier axis and leaves with a later one in the same shift
    assert cov["revisit"] >= 5, cov        # the entering slab holds voxels written before they left
    assert cov["origin"] >= 1, cov         # back at the origin: every voxel written on the way is in the window or the store
    assert tuple(walk[-1]) == (0, 0, 0)
    assert cov["seam_boxes"] >= 3, cov     # written boxes that lie across the ring seam of every axis
    if max(size) > 64:
        assert cov["chunk_borders"] >= 10 and cov["negative_chunks"] >= 10, cov


def test_expected_slabs_partition_the_move():
    """the slab boxes the GPU tests expect, against the model's own move: together the leaving boxes hold every voxel of the old
    window that the new one lacks (and, for a corner, voxels that were in neither), and no box is wider than the ring"""
    rng = np.random.default_rng(5)
    for size in [(21, 17, 13), (16, 18, 20), (3, 19, 5), (4, 4, 4)]:
        size = np.asarray(size)
        for _ in range(40):
            pos = rng.integers(-30, 31, 3)
            new_pos = pos + np.array([rng.integers(-int(s), int(s) + 1) for s in size])
            olo, ohi = M.window(size, pos)
            nlo, nhi = M.window(size, new_pos)
            blo, bhi = np.minimum(olo, nlo) - 1, np.maximum(ohi, nhi) + 1
            shape = tuple(int(v) for v in bhi - blo + 1)
            sl = lambda lo, hi: tuple(slice(int(lo[k] - blo[k]), int(hi[k] - blo[k]) + 1) for k in range(3))
            inside = np.zeros(shape, dtype=bool)
            inside[sl(olo, ohi)] = True
            slabs = M.expected_slabs(size, pos, new_pos)
            assert len(slabs) == int(np.count_nonzero(new_pos != pos))
            for s in slabs:  # replay: what leaves was inside, what enters was not
                for lo, hi in (s["leave"], s["enter"]):
                    assert np.all(hi - lo + 1 <= size) and np.all(hi >= lo)
                assert inside[sl(*s["leave"])].all()
                inside[sl(*s["leave"])] = False
                assert not inside[sl(*s["enter"])].any()
                inside[sl(*s["enter"])] = True
            want = np.zeros(shape, dtype=bool)
            want[sl(nlo, nhi)] = True
            assert np.array_equal(inside, want)


def test_shift_plan_is_the_models_slabs():
    """ws_shift_plan (no map, no GPU) against the model over the shapes of test_expected_slabs_partition_the_move: the steps, every
    leaving and entering box, and the window's final pos / offset; no move, the largest step and the first one refused"""
    import ctypes as C
    from warpsense_amd import _lib
    L = _lib.load()
    i3 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def plan_of(size, pos, new_pos):
        plan = _lib.ShiftPlan()
        size, pos, off, new_pos = i3(size), i3(pos), i3(M.model_offset(size, pos)), i3(new_pos)
        return L.ws_shift_plan(p(size), p(pos), p(off), p(new_pos), C.byref(plan)), plan

    rng = np.random.default_rng(5)
    for size in [(21, 17, 13), (16, 18, 20), (3, 19, 5), (4, 4, 4)]:
        size = np.asarray(size)
        for _ in range(40):
            pos = rng.integers(-30, 31, 3)
            new_pos = pos + np.array([rng.integers(-int(s), int(s) + 1) for s in size])
            rc, plan = plan_of(size, pos, new_pos)
            want = M.expected_slabs(size, pos, new_pos)
            assert rc == 0 and plan.n == len(want)
            for i, s in enumerate(want):
                assert plan.axis[i] == s["axis"] and plan.d[i] == new_pos[s["axis"]] - pos[s["axis"]]
                assert np.array_equal(plan.leave_lo[i], s["leave"][0]) and np.array_equal(plan.leave_hi[i], s["leave"][1])
                assert np.array_equal(plan.enter_lo[i], s["enter"][0]) and np.array_equal(plan.enter_hi[i], s["enter"][1])
            assert np.array_equal(plan.pos, new_pos) and np.array_equal(plan.offset, M.model_offset(size, new_pos))
        pos = rng.integers(-30, 31, 3)
        rc, plan = plan_of(size, pos, pos)
        assert rc == 0 and plan.n == 0 and np.array_equal(plan.pos, pos) and np.array_equal(plan.offset, M.model_offset(size, pos))
        for axis in range(3):
            for sign in (1, -1):
                step = np.zeros(3, dtype=np.int64)
                step[axis] = sign * size[axis]
                rc, plan = plan_of(size, pos, pos + step)
                assert rc == 0 and plan.n == 1 and plan.axis[0] == axis and plan.d[0] == step[axis]
                step[axis] += sign
                assert plan_of(size, pos, pos + step)[0] == WS_ERR_INVALID
    a, plan = i3((0, 0, 0)), _lib.ShiftPlan()
    for k in range(5):
        args = [p(i3((5, 5, 5))), p(a), p(a), p(a), C.byref(plan)]
        args[k] = None
        assert L.ws_shift_plan(*args) == WS_ERR_INVALID
