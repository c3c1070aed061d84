"""ws_store_coarsen and MapPyramid at the ends of their domain: chunk keys at INT32_MIN and INT32_MAX and parents whose children lie
beyond int32, refresh() over boxes at negative and odd keys, absent chunks and empty space, a base chunk that was dropped, and a
plan of 700 rows (8400 words: more than the 8192 a slot table holds from the start) followed by a trip round the ring of eight
tables.  Every comparison is bit for bit against coarsen_model.py.

Measured on an MI355X (pytest's durations): the eleven tests take 8 s together, the slowest 2.1 s (the first refresh box, which also
computes the shared model); test_a_plan_beyond_one_table_then_the_ring takes 0.52 s with its 700 puts and 50 chunks read back."""
import numpy as np
import pytest

import coarsen_model as CM
import fuse_scenes as S
import two_store_scenes as T
from fuse_scenes import FILL, RES
from two_store_scenes import IMAX, IMIN, observed

pytestmark = pytest.mark.gpu


def read_levels(p):
    return [S.read(p.store(l)) for l in range(p.levels + 1)]


# ------------------------------------------------------------------------------------------------ 1. the ends of the keys
def test_parents_at_the_ends_of_int32():
    import warpsense_amd as W
    src_chunks = T.key_end_source()
    want, want_stats = CM.coarsen({}, src_chunks, None, 8, FILL)
    src, dst = S.make_store(src_chunks, segment_chunks=1), S.make_store({}, segment_chunks=0)
    st = src.coarsen(dst)
    got = S.read(dst)
    assert st.as_tuple() == tuple(want_stats) == (4, 4, 5 * 32 ** 3, 0)
    assert sorted(got) == sorted([(2 ** 30 - 1, -2 ** 30, 0), (-2 ** 30, 2 ** 30 - 1, -1), (-1, -1, -1), (0, 0, 0)]) and CM.same(got, want)
    both = got[(2 ** 30 - 1, -2 ** 30, 0)].reshape(64, 64, 64)  # the children x = INT32_MAX - 1 and INT32_MAX, y = INT32_MIN, z = 0
    assert np.all(both[:, :32, :32] != FILL) and np.all(both[:, 32:, :] == FILL) and np.all(both[:, :, 32:] == FILL)
    one = got[(-2 ** 30, 2 ** 30 - 1, -1)].reshape(64, 64, 64)  # the child x = INT32_MIN (cx 0), y = INT32_MAX (cy 1), z = -1 (cz 1)
    assert np.all(one[:32, 32:, 32:] != FILL) and np.count_nonzero(one != FILL) == 32 ** 3
    assert CM.same(S.read(src), src_chunks)
    assert np.array_equal(W.parents_of(T.KEY_END_KEYS), CM.parents_of(T.KEY_END_KEYS)) and W.parents_of(T.KEY_END_KEYS).dtype == np.int32


def test_listed_parents_whose_children_lie_beyond_int32():
    """absent in DST: nothing is created; present: every word becomes fill, and the key counts as processed with no voxel valued.
    Two of the keys are such that children cast to int32 without the range check would be chunks of SRC"""
    src_chunks = T.key_end_source()
    src = S.make_store(src_chunks, segment_chunks=1)
    empty = S.make_store({}, segment_chunks=4)
    st = src.coarsen(empty, T.KEY_END_LISTED)
    assert st.as_tuple() == (0, 0, 0, 0) and empty.count() == 0
    dst_chunks = {key: S.draw(90 + i, False) for i, key in enumerate(T.KEY_END_LISTED)}
    dst_chunks[(7, 7, 7)] = S.draw(99, False)  # not listed
    want, want_stats = CM.coarsen(dst_chunks, src_chunks, T.KEY_END_LISTED, 8, FILL)
    dst = S.make_store(dst_chunks, segment_chunks=4)
    st = src.coarsen(dst, T.KEY_END_LISTED)
    got = S.read(dst)
    assert st.as_tuple() == tuple(want_stats) == (4, 0, 0, 0) and CM.same(got, want)
    assert all(np.all(got[key] == FILL) for key in T.KEY_END_LISTED) and np.array_equal(got[(7, 7, 7)], dst_chunks[(7, 7, 7)])
    assert CM.same(S.read(src), src_chunks)


def test_pyramid_over_the_ends_of_int32():
    import warpsense_amd as W
    src_chunks = T.key_end_source()
    levels = CM.pyramid(src_chunks, 3, 8, FILL)
    p = W.MapPyramid(S.make_store(src_chunks, segment_chunks=1), 3, RES, segment_chunks=2)
    p.rebuild()
    got = read_levels(p)
    for l in range(4):
        assert CM.same(got[l], levels[l]), l
    for l, far in ((1, 2 ** 30), (2, 2 ** 29), (3, 2 ** 28)):
        assert (-1, -1, -1) in got[l] and (-far, far - 1, -1) in got[l] and (far - 1, -far, 0) in got[l] and len(got[l]) == 4
        assert np.any(got[l][(-1, -1, -1)] != FILL) and np.any(got[l][(-far, far - 1, -1)] != FILL)
    p.close(), p.base.close()


# ------------------------------------------------------------------------------------------------ 2. refresh boxes
_BASE = {}


def refresh_base():
    if not _BASE:
        base = dict(T.pyramid_case()["base"])
        base.update({(-1, 0, -1): observed(101), (-2, 0, -1): observed(102), (-3, -1, -2): observed(103)})
        _BASE.update(base=base, levels=CM.pyramid(base, 3, 8, FILL))
    return _BASE


# (lo, hi, the chunks to put inside the box)
BOXES = {
    "one voxel at -1": ((-1, -1, -1), (-1, -1, -1), [(-1, -1, -1)]),
    "one voxel at (-65, 0, -129)": ((-65, 0, -129), (-65, 0, -129), [(-2, 0, -3)]),  # a chunk the base does not hold yet
    "across the origin": ((-10, -10, -10), (10, 10, 10), [(0, 0, 0), (-1, -1, 0), (-1, 0, -1)]),
    "ends at voxel -129": ((-140, -10, -70), (-129, -1, -65), [(-3, -1, -2)]),  # key -3 -> -2 -> -1: odd on the first and the third level
    "four chunks, two absent": ((-128, 0, -128), (-1, 63, -1), [(-2, 0, -1), (-1, 0, -1)]),  # (-2, 0, -2) and (-1, 0, -2) are absent
    "far from every chunk": ((6400, 6400, 6400), (6500, 6500, 6500), []),
}


@pytest.mark.parametrize("name", list(BOXES))
def test_refresh_of_a_box(name):
    import warpsense_amd as W
    lo, hi, puts = BOXES[name]
    g = refresh_base()
    p = W.MapPyramid(S.make_store(g["base"], segment_chunks=1), 3, RES)
    p.rebuild()
    before = read_levels(p)
    for l in range(4):
        assert CM.same(before[l], g["levels"][l]), l
    box_keys = [tuple(int(v) for v in k) for k in W.chunks_of_box(lo, hi)]
    changed = dict(g["base"])
    for i, key in enumerate(puts):
        assert key in box_keys
        changed[key] = observed(200 + i)
        p.base.put_chunk(key, changed[key])
    if name == "four chunks, two absent":
        assert len(box_keys) == 4 and sum(k in changed for k in box_keys) == 2
    stats = p.refresh(lo, hi)
    after = read_levels(p)
    full = W.MapPyramid(S.make_store(changed, segment_chunks=2), 3, RES, segment_chunks=2)
    full.rebuild()
    model = CM.pyramid(changed, 3, 8, FILL) if puts else g["levels"]
    for l, (got, want) in enumerate(zip(after, read_levels(full))):
        assert CM.same(got, want) and CM.same(got, model[l]), l
    # outside the parents of the box every level keeps its keys and bytes
    keys = np.asarray(box_keys)
    for l in range(1, 4):
        keys = CM.parents_of(keys)
        inside = {tuple(int(v) for v in k) for k in keys}
        assert set(after[l]) - set(before[l]) <= inside and set(before[l]) <= set(after[l])
        assert all(np.array_equal(after[l][k], before[l][k]) for k in before[l] if k not in inside), l
        assert stats[l - 1].chunks == len(inside & set(after[l]))
    if not puts:
        assert all(s.as_tuple() == (0, 0, 0, 0) for s in stats) and all(CM.same(a, b) for a, b in zip(after, before))
    else:
        assert any(not CM.same(a, b) for a, b in zip(after[1:], before[1:]))
    p.close(), full.close(), p.base.close(), full.base.close()


# ------------------------------------------------------------------------------------------------ 3. a dropped base chunk
def test_a_dropped_base_chunk_needs_refresh_of_its_box():
    """(5, -3, 2) is alone under (2, -2, 1) and (1, -1, 0), and has company under (0, -1, 0) of level 3.  refresh() over its box turns
    the first two to fill and recomputes the third; rebuild() covers the parents of the chunks a level HAS, so it leaves them stale"""
    import warpsense_amd as W
    g = refresh_base()
    gone = (5, -3, 2)
    left = {k: v for k, v in g["base"].items() if k != gone}
    model = CM.pyramid(left, 3, 8, FILL)
    ancestors = [(2, -2, 1), (1, -1, 0), (0, -1, 0)]
    pyramids = []
    for _ in range(2):
        p = W.MapPyramid(S.make_store(g["base"], segment_chunks=1), 3, RES, segment_chunks=2)
        p.rebuild()
        p.base.drop_chunk(gone)
        pyramids.append(p)
    fresh = W.MapPyramid(S.make_store(left, segment_chunks=1), 3, RES, segment_chunks=2)
    fresh.rebuild()
    p, stale = pyramids
    before = read_levels(p)
    p.refresh(tuple(64 * k for k in gone), tuple(64 * k + 63 for k in gone))
    after = read_levels(p)
    assert np.all(after[1][ancestors[0]] == FILL) and np.all(after[2][ancestors[1]] == FILL) and ancestors[0] not in model[1] and ancestors[1] not in model[2]
    assert CM.same(after[3], model[3]) and not np.array_equal(after[3][ancestors[2]], before[3][ancestors[2]])
    for l in (1, 2):  # but for the chunk of fill the level is the model's
        assert CM.same({k: v for k, v in after[l].items() if k != ancestors[l - 1]}, model[l]), l
    for l in (1, 2, 3):
        a, b = p.store(l).mesh(p.resolution(l)), fresh.store(l).mesh(fresh.resolution(l))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (l > 1 or len(a[0]) > 100), l
    # rebuild() alone: the ancestors keep what the dropped chunk gave them
    stale.rebuild()
    old = read_levels(stale)
    for l in (1, 2, 3):
        assert np.array_equal(old[l][ancestors[l - 1]], before[l][ancestors[l - 1]]) and np.any(old[l][ancestors[l - 1]] != FILL), l
    assert not CM.same(old[3], model[3])
    for q in (p, stale, fresh):
        q.close(), q.base.close()


# ------------------------------------------------------------------------------------------------ 4. a plan beyond one slot table
def test_a_plan_beyond_one_table_then_the_ring():
    """700 listed keys are 8400 words of plan: the slot table grows inside the call.  Rows 0, 681, 682 (which holds word 8192), 683,
    699 and three drawn rows have a child; all others turn to fill.  Then eight single-row calls without a wait take the ring of
    eight tables once round, the eighth onto the grown table, and a ninth goes past it"""
    import time
    import warpsense_amd as W
    t0 = time.perf_counter()
    rows, n = T.plan_rows(), T.PLAN_ROWS
    keys = [(i, 0, 0) for i in range(n)]
    shared = S.draw(300, False)
    dst = W.DeviceGlobalMap(S.TAU, 0)
    for key in keys:
        dst.put_chunk(key, shared)
    assert dst.capacity() == 3 * 256
    src_chunks = {T.plan_child(row, j): observed(310 + j) for j, row in enumerate(rows)}
    src = S.make_store(src_chunks, segment_chunks=1)
    # the model on the rows with a child; a present row without one is processed, values nothing and turns to fill (test_two_store_host.py)
    want, want_stats = CM.coarsen({(row, 0, 0): shared for row in rows}, src_chunks, [(row, 0, 0) for row in rows], 8, FILL)
    st = src.coarsen(dst, keys)
    assert st.as_tuple() == (n, 0, want_stats[2], want_stats[3]) and want_stats[:2] == [8, 0] and st.valued == 8 * 32 ** 3
    for row in rows:
        assert np.array_equal(dst.chunk((row, 0, 0)), want[(row, 0, 0)]), row
    rng = np.random.default_rng(700)
    beside = sorted({r + d for r in rows for d in (-1, 1)} - set(rows) - {-1, n})
    others = [i for i in range(n) if i not in rows and i not in beside]
    drawn = sorted(int(v) for v in rng.choice(others, 16, replace=False))
    for row in beside + drawn:
        assert np.all(dst.chunk((row, 0, 0)) == FILL), row
    assert dst.count() == n and CM.same(S.read(src), src_chunks)
    # the ring: SRC changes first (a put waits for the stream), then nine calls back to back
    ninth = drawn[7]
    changed = {T.plan_child(row, j + 3): observed(330 + j) for j, row in enumerate(rows)}
    changed[T.plan_child(ninth, 5)] = observed(340)
    for key in src_chunks:
        src.drop_chunk(key)
    for key, data in changed.items():
        src.put_chunk(key, data)
    for row in rows + [ninth]:
        assert src.coarsen(dst, [(row, 0, 0)], stats=False) is None
    dst.ctx.sync()
    want, want_stats = CM.coarsen({(row, 0, 0): shared for row in rows + [ninth]}, changed, [(row, 0, 0) for row in rows + [ninth]], 8, FILL)
    assert want_stats == [9, 0, 9 * 32 ** 3, 0]
    for row in rows + [ninth]:
        assert np.array_equal(dst.chunk((row, 0, 0)), want[(row, 0, 0)]), row
    assert np.all(dst.chunk((drawn[0], 0, 0)) == FILL)
    print("seconds", time.perf_counter() - t0)
    src.close(), dst.close()
