"""The sliding window far from the origin, on the CPU: the world model of tests/window_model.py against LocalMap.shift with windows
that touch both ends of int32, ws_shift_plan against the model there -- what it plans and what it refuses -- and the chunk keys
of boxes that end at INT32_MAX and begin at INT32_MIN.  tests/test_gpu_window_domain.py runs the device routes from the same
bases.

The rule (include/warpsense_hip.h): every window of a plan, pos - size/2 .. pos - size/2 + size - 1, lies in int32 on
every axis, else WS_ERR_RANGE."""
import ctypes as C

import numpy as np
import pytest

from window_host_routes import HostRoute, TAU
from window_model import I32_MAX, I32_MIN, WALKS
import window_model as M

WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
SIZES = [(21, 17, 13), (16, 18, 20), (3, 19, 5), (4, 4, 4)]
BASES = ["aligned+-+", "aligned-+-", "touching"]


def _i3(v):
    v = np.asarray(v, dtype=np.int64)
    assert np.all(v >= I32_MIN) and np.all(v <= I32_MAX), v  # the argument itself fits: only the window may not
    return np.ascontiguousarray(v.astype(np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def plan_of(size, pos, new_pos):
    from warpsense_amd import _lib
    L = _lib.load()
    plan = _lib.ShiftPlan()
    size, off, pos, new_pos = _i3(size), _i3(M.model_offset(size, pos)), _i3(pos), _i3(new_pos)
    rc = L.ws_shift_plan(_p(size), _p(pos), _p(off), _p(new_pos), C.byref(plan))
    return rc, plan, (L.ws_last_error() or b"").decode() if rc else ""


def assert_planned(size, pos, new_pos):
    """accepted, and exactly the model's: steps, every leaving and entering box, the final pos / offset"""
    rc, plan, text = plan_of(size, pos, new_pos)
    assert rc == 0, (size, pos, new_pos, text)
    want = M.expected_slabs(size, pos, new_pos)
    assert plan.n == len(want)
    for i, s in enumerate(want):
        assert plan.axis[i] == s["axis"] and plan.d[i] == int(new_pos[s["axis"]]) - int(pos[s["axis"]])
        assert np.array_equal(plan.leave_lo[i], s["leave"][0]) and np.array_equal(plan.leave_hi[i], s["leave"][1]), (size, pos, new_pos, i)
        assert np.array_equal(plan.enter_lo[i], s["enter"][0]) and np.array_equal(plan.enter_hi[i], s["enter"][1]), (size, pos, new_pos, i)
        for lo, hi in (s["leave"], s["enter"]):
            assert M.fits_int32(lo, hi) and np.all(hi >= lo)
    assert np.array_equal(plan.pos, new_pos) and np.array_equal(plan.offset, M.model_offset(size, new_pos))


def assert_refused(size, pos, new_pos, code):
    rc, _, text = plan_of(size, pos, new_pos)
    assert rc == code, (size, pos, new_pos, rc, text)
    assert text.startswith("ws_shift_plan"), text  # the entry point's name, as the queries' refusals have it


def plan_windows(size, pos, new_pos):
    """every window of the plan: at pos, and behind each axis step in the order x, y, z"""
    p = np.asarray(pos, dtype=np.int64).copy()
    out = [M.window(size, p)]
    for axis in range(3):
        if int(new_pos[axis]) != int(p[axis]):
            p[axis] = new_pos[axis]
            out.append(M.window(size, p))
    return out


# ------------------------------------------------------------------------------------------------ the model, far out
@pytest.fixture(scope="module")
def near_walks():
    """the walks from the origin through LocalMap.shift, once: the final ring and the chunks"""
    import warpsense_amd as W
    out = {}
    for size, seed in WALKS:
        r = HostRoute(size)
        M.run_walk(size, M.make_walk(size, seed), seed, r, W.pack_entry(TAU, 0), check_every=False)
        out[(size, seed)] = (r.lm.data.copy(), {k: v.copy() for k, v in r.lm.map_.chunks.items()})
    return out


@pytest.mark.parametrize("name", BASES)
@pytest.mark.parametrize("size,seed", WALKS)
def test_model_matches_local_map_shift_from_far_bases(size, seed, name, near_walks):
    """both work in int64: this pins them there before the device is held to them"""
    import warpsense_amd as W
    base = M.far_bases(size, seed)[name]
    walk = M.make_walk(size, seed, base=base)
    near = M.make_walk(size, seed)
    assert [tuple(np.asarray(p) - np.asarray(base)) for p in walk] == near and walk[-1] == base
    lo, hi = M.walk_bounds(size, walk, base)
    assert M.fits_int32(lo, hi)
    if name == "touching":
        assert hi[0] == I32_MAX and lo[1] == I32_MIN and base[2] == 2 ** 30 + 37
        wins = [M.window(size, p) for p in walk]
        assert any(w[1][0] == I32_MAX for w in wins) and any(w[0][1] == I32_MIN for w in wins)  # some window holds either voxel
    else:
        unit = 64 * np.asarray(size, dtype=np.int64)
        assert np.all(np.asarray(base) % unit == 0) and np.all(np.asarray(base) != 0)
        out = np.where(np.asarray(base) > 0, hi + unit > I32_MAX, lo - unit < I32_MIN)
        assert np.all(out)  # one multiple further and the walk's bounding box leaves int32
    r = HostRoute(size)
    r.lm.pos[:] = base
    r.lm.offset[:] = M.model_offset(size, base)
    w = M.run_walk(size, walk, seed, r, W.pack_entry(TAU, 0), base=base)
    assert np.array_equal(w.pos, base) and np.count_nonzero(w.store != w.default_raw) > 0
    assert M.walk_coverage(size, walk, seed, base=base)["origin"] == M.walk_coverage(size, near, seed)["origin"] >= 1
    keys = set(r.lm.map_.chunks)
    if name == "touching":
        assert max(k[0] for k in keys) == 2 ** 25 - 1 and min(k[1] for k in keys) == -2 ** 25
    else:  # the walk from the origin, moved: the same ring bytes, the same chunks under keys moved by base / 64
        ring, chunks = near_walks[(size, seed)]
        assert np.array_equal(r.lm.data, ring)
        shift = np.asarray(base) // 64
        assert keys == {tuple(int(v) for v in np.asarray(k) + shift) for k in chunks}
        for k, c in chunks.items():
            assert np.array_equal(r.lm.map_.chunks[tuple(int(v) for v in np.asarray(k) + shift)], c), k


# ------------------------------------------------------------------------------------------------ ws_shift_plan at the edges
def edge_positions(size):
    """positions whose window ends `gap` voxels short of INT32_MAX (side +1) or begins `gap` voxels after INT32_MIN (side -1), per
    axis: gaps 0 (the window's last voxel is INT32_MAX / its first INT32_MIN exactly), 1, size - 1 and size, every mix of sides"""
    size = np.asarray(size, dtype=np.int64)
    rng = np.random.default_rng(int(size.sum()))
    out = []
    for sides in [(1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1), (1, 1, -1), (-1, 1, 1)]:
        for gaps in [(0, 0, 0), (1, 1, 1), tuple(size - 1), tuple(size), tuple(int(rng.integers(0, s + 1)) for s in size), (0, 1, 2)]:
            pos = [I32_MAX - g - (s - 1 - s // 2) if side > 0 else I32_MIN + g + s // 2 for side, g, s in zip(sides, gaps, size)]
            lo, hi = M.window(size, pos)
            assert all((I32_MAX - hi[k] if sides[k] > 0 else lo[k] - I32_MIN) == gaps[k] for k in range(3))
            out.append((np.asarray(pos, dtype=np.int64), np.asarray(sides), np.asarray(gaps, dtype=np.int64)))
    return out


@pytest.mark.parametrize("size", SIZES)
def test_shift_plan_at_the_edges_of_int32(size):
    """Accepted: the largest outward step that keeps the window inside, per axis and on all three at once, planned as the model
    has it; a step of `size` back towards the origin.  Refused: one voxel further.  Which refusal: per axis in the order x, y, z
    the step's size is tested first (WS_ERR_INVALID), the window behind it second (WS_ERR_RANGE) -- so a step that is too large
    AND out of range on one axis is WS_ERR_INVALID, and across axes the first offending axis decides."""
    size = np.asarray(size, dtype=np.int64)
    seen = {"exact_max": 0, "exact_min": 0, "range": 0, "invalid": 0, "both": 0, "across": 0}
    for pos, sides, gaps in edge_positions(size):
        lo, hi = M.window(size, pos)
        seen["exact_max"] += int(np.any(hi == I32_MAX))
        seen["exact_min"] += int(np.any(lo == I32_MIN))
        assert_planned(size, pos, pos)
        best = np.minimum(size, gaps) * sides  # the largest outward step per axis
        for axis in range(3):
            step = np.zeros(3, dtype=np.int64)
            step[axis] = best[axis]
            assert_planned(size, pos, pos + step)
            step[axis] += sides[axis]  # one voxel further
            if abs(step[axis]) > size[axis]:
                assert_refused(size, pos, pos + step, WS_ERR_INVALID)
                seen["invalid"] += 1
            else:
                assert_refused(size, pos, pos + step, WS_ERR_RANGE)
                seen["range"] += 1
            # too large and out of range at once, on this axis alone: the size of the step comes first
            both = np.zeros(3, dtype=np.int64)
            both[axis] = sides[axis] * (size[axis] + 1)
            if gaps[axis] <= size[axis] and M.fits_int32(pos + both, pos + both):  # (new_pos itself has to be an int32)
                assert not M.fits_int32(*M.window(size, pos + both))
                assert_refused(size, pos, pos + both, WS_ERR_INVALID)
                seen["both"] += 1
            # back towards the origin by the whole size
            back = np.zeros(3, dtype=np.int64)
            back[axis] = -sides[axis] * size[axis]
            assert_planned(size, pos, pos + back)
        assert_planned(size, pos, pos + best)          # all three at once
        assert_planned(size, pos, pos - sides * size)  # and all three back
        # across axes: x out of range and y too large is x's refusal, x too large and y out of range is x's too
        if gaps[0] < size[0] and gaps[1] < size[1]:
            out_of_range, too_large = best + sides, sides * (size + 1)
            for step, code in [(np.array([out_of_range[0], too_large[1], 0]), WS_ERR_RANGE), (np.array([too_large[0], out_of_range[1], 0]), WS_ERR_INVALID)]:
                if M.fits_int32(pos + step, pos + step):
                    assert_refused(size, pos, pos + step, code)
                    seen["across"] += 1
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("size", SIZES)
def test_shift_plan_accepts_exactly_the_plans_whose_windows_fit(size):
    """Three-axis steps drawn around the corners of int32: accepted if and only if every window of the plan -- at pos, behind the
    x step, behind the y step, behind the z step -- fits.  (An axis moves once, so a window between two steps is per axis the first
    window's range or the last one's: none can leave int32 unless the first or the last does, which the test asserts from the
    model's windows.  So the rule needs no more than the window behind every step; the draw holds plans whose first refused window
    is the one behind x, behind y and behind z.)"""
    size = np.asarray(size, dtype=np.int64)
    rng = np.random.default_rng(7)
    n_ok = n_range = 0
    first_bad = set()
    for sides in [(1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1)]:
        sides = np.asarray(sides)
        for _ in range(60):
            gaps = np.array([rng.integers(0, 3) for _ in range(3)])
            pos = np.where(sides > 0, I32_MAX - gaps - (size - 1 - size // 2), I32_MIN + gaps + size // 2)
            step = np.array([rng.integers(-int(s), int(s) + 1) for s in size])
            step = np.where(rng.integers(0, 2, 3) == 1, np.clip(step, -3, 3), step)  # small steps too: near the limit either way
            new_pos = pos + step
            if not (np.all(new_pos >= I32_MIN) and np.all(new_pos <= I32_MAX)):
                continue
            wins = plan_windows(size, pos, new_pos)
            fits = [M.fits_int32(*w) for w in wins]
            assert fits[0] and (all(fits) or not fits[-1])
            if all(fits):
                assert_planned(size, pos, new_pos)
                n_ok += 1
            else:
                assert_refused(size, pos, new_pos, WS_ERR_RANGE)
                n_range += 1
                moved = [k for k in range(3) if step[k]]
                first_bad.add(moved[fits.index(False) - 1])
    assert n_ok > 20 and n_range > 20 and first_bad == {0, 1, 2}


def test_shift_plan_refuses_a_window_that_is_outside_to_begin_with():
    """pos itself is an int32, its window is not: no plan, not even for new_pos == pos or for the step back in"""
    for size in SIZES:
        s = np.asarray(size, dtype=np.int64)
        for pos in [(I32_MAX, 0, 0), (0, I32_MIN, 0), (0, 0, I32_MAX - (int(s[2]) - 1 - int(s[2]) // 2) + 1), (I32_MIN + int(s[0]) // 2 - 1, 0, 0)]:
            pos = np.asarray(pos, dtype=np.int64)
            assert not M.fits_int32(*M.window(s, pos))
            assert_refused(s, pos, pos, WS_ERR_RANGE)
            assert_refused(s, pos, np.where(np.abs(pos) > 2 ** 30, pos - np.sign(pos) * s, pos), WS_ERR_RANGE)  # the step back in


# ------------------------------------------------------------------------------------------------ chunk keys at the edges
def test_chunks_of_box_at_the_ends_of_int32():
    import warpsense_amd as W
    from window_host_routes import expected_keys
    top, bottom = 2 ** 25 - 1, -2 ** 25
    boxes = [((I32_MAX, I32_MAX, I32_MAX), (I32_MAX, I32_MAX, I32_MAX)),
             ((I32_MIN, I32_MIN, I32_MIN), (I32_MIN, I32_MIN, I32_MIN)),
             ((I32_MAX - 64, I32_MIN, 2 ** 30 + 37), (I32_MAX, I32_MIN + 64, 2 ** 30 + 37 + 64)),  # two chunks per axis, mixed signs
             ((I32_MIN, I32_MAX - 63, -1), (I32_MIN + 63, I32_MAX, 0)),                            # exactly the first and the last chunk
             ((I32_MAX - 200, I32_MAX - 2, I32_MIN), (I32_MAX, I32_MAX, I32_MIN + 130))]
    for lo, hi in boxes:
        got = W.chunks_of_box(lo, hi)
        assert np.array_equal(got, expected_keys(lo, hi)), (lo, hi)
        assert got.min() >= bottom and got.max() <= top
    assert np.array_equal(W.chunks_of_box(*boxes[0]), [[top, top, top]])
    assert np.array_equal(W.chunks_of_box(*boxes[1]), [[bottom, bottom, bottom]])
    assert np.array_equal(W.chunks_of_box(*boxes[3]), [[bottom, top, -1], [bottom, top, 0]])
    got = W.chunks_of_box(*boxes[2])
    assert len(got) == 8 and tuple(got[0]) == (top - 1, bottom, 2 ** 24) and tuple(got[-1]) == (top, bottom + 1, 2 ** 24 + 1)
