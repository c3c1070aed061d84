"""CPU tests of the scenes of test_gpu_two_store_geometry.py and test_gpu_coarsen_domain.py: what the aged stores are built to show is
asserted here on a pure-Python replay of the directory rules of api_store.hip (two_store_scenes.Directory) and on the numpy models
alone -- that the slots are out of key order, reused and spread over segments, that a lookup with the other store's shift would land in
other bytes or outside every allocation (no wrong kernel is ever run for that), that every scene compares a thousand voxels or more,
and the row and word arithmetic of the coarsen plan that outgrows a slot table.  No GPU."""
import numpy as np
import pytest

import coarsen_model as CM
import two_store_scenes as T
from fuse_scenes import FILL

ALL_CASES = [(pair, name) for pair in T.PAIRS for name in T.SCENES if 0 not in pair or name in T.DEFAULT_POOL_SCENES]


def test_the_replay_follows_the_directory_rules():
    """slots count up, a dropped slot is the next one taken (a stack), an overwrite keeps its slot, and the capacity is whole segments"""
    d = T.Directory(2)
    for key in "abcde":
        d.put(key)
    assert [d.dir[k] for k in "abcde"] == [0, 1, 2, 3, 4] and d.nseg == 3 and d.capacity() == 6
    d.drop("b"), d.drop("d")
    d.put("a")  # an overwrite
    assert d.dir["a"] == 0 and d.free == [1, 3]
    d.put("f"), d.put("g"), d.put("h")
    assert (d.dir["f"], d.dir["g"], d.dir["h"]) == (3, 1, 5) and d.recycled == {"f", "g"} and d.nseg == 3
    d.put("i")
    assert d.dir["i"] == 6 and d.nseg == 4
    # a call that creates several chunks asks for all the room first, then takes the slots in key order
    d.drop("a")
    d.create(["z", "x", "y", "c"])
    assert (d.dir["x"], d.dir["y"], d.dir["z"]) == (0, 7, 8) and d.nseg == 5
    assert [T.shift_of(n) for n in (0, 1, 2, 3, 4, 256, 257)] == [8, 0, 1, 2, 2, 8, 9]
    # the default pool: everything in one segment of 256
    d = T.Directory(0)
    for i in range(256):
        d.put(i)
    assert d.nseg == 1
    d.put(256)
    assert d.nseg == 2 and d.capacity() == 512


def test_a_history_ends_with_exactly_the_scene():
    keys = [(i, -i, 2 * i) for i in range(7)]
    ops = T.history(keys, 5)
    d = T.Directory(2).run(ops)
    assert sorted(d.dir) == sorted(keys)
    assert sum(1 for op, k, what in ops if what == "other") >= 2 and sum(1 for op, k, what in ops if what == "decoy" and op == "put") == 16
    assert all(k[0] >= 1 << 20 for op, k, what in ops if what == "decoy")  # outside every scene
    # every "other" put is followed by a "real" put of the same key; the last operation on every key is a real put
    last = {}
    for op, key, what in ops:
        last[key] = (op, what)
    assert all(last[k] == ("put", "real") for k in keys) and all(v == ("drop", "decoy") for k, v in last.items() if k not in keys)
    assert T.history([], 3) and sorted(T.Directory(1).run(T.history([], 3)).dir) == []


@pytest.mark.parametrize("pair,name", ALL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_aged_stores_are_out_of_order_reused_and_spread(pair, name):
    s = T.scene(name)
    for which, geometry, seed in (("first", pair[0], T.seeds(name)[0]), ("second", pair[1], T.seeds(name)[1])):
        keys = sorted(s[which])
        if len(keys) < 3:
            continue
        d = T.replay(keys, geometry, seed)
        mixed, reused, spans = T.claims(d, keys)
        print(name, which, geometry, "slots", [d.dir[k] for k in keys], "reused", reused, "segments", d.nseg, "spans", spans)
        assert T.hold(d, keys, geometry), (which, geometry)
    assert len(s[T.read_store(name)[0]]) >= 3  # the store a wrong shift is seen on always makes the claims


@pytest.mark.parametrize("pair,name", ALL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_a_swapped_shift_would_be_seen(pair, name):
    """SRC's (changes: REF's) slots addressed with the shift of the other store: at least one chunk of the scene would be read from
    another chunk whose bytes differ, or from outside every allocation.  With equal shifts (the control) nothing moves."""
    s = T.scene(name)
    which, other = T.read_store(name)
    geometry = dict(first=pair[0], second=pair[1])
    seed = T.seeds(name)[0 if which == "first" else 1]
    d = T.replay(sorted(s[which]), geometry[which], seed)
    outside, elsewhere = T.seen(d, T.shift_of(geometry[other]), s[which])
    print(name, pair, which, "outside", outside, "in another chunk", elsewhere)
    if T.shift_of(pair[0]) == T.shift_of(pair[1]):
        assert set(T.astray(d, d.shift).values()) == {"same"} and not outside and not elsewhere
    else:
        assert outside or elsewhere
    # and the other way round, for the store that is written or sampled on its own lattice
    back = T.replay(sorted(s[other]), geometry[other], T.seeds(name)[1 if which == "first" else 0])
    if s[other] and T.shift_of(pair[0]) != T.shift_of(pair[1]) and len(s[other]) >= 3:
        assert any(w != "same" for w in T.astray(back, T.shift_of(geometry[which])).values())


@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_every_scene_compares_a_thousand_voxels(name):
    print(name, T.volume(name))
    assert T.volume(name) >= 1000


def test_listed_scene_has_every_kind_of_row():
    s, (out, stats) = T.scene("coarsen_listed"), T.want("coarsen_listed")
    dst = s["second"]
    assert stats == [3, 1, 3 * 32 ** 3, 0] and sorted(out) == sorted(list(dst) + [(2, 2, 2)])
    assert np.all(out[(7, 7, 7)] == FILL) and not np.array_equal(out[(0, 0, 0)], dst[(0, 0, 0)])
    assert np.array_equal(out[(1, 0, 0)], dst[(1, 0, 0)]) and np.array_equal(out[(-1, 0, 0)], dst[(-1, 0, 0)]) and (9, 9, 9) not in out


def test_key_ends_on_the_model():
    """the parents at the ends of int32, and what a cast without the range check would do to the listed keys"""
    src = T.key_end_source()
    parents = [tuple(int(v) for v in k) for k in CM.parents_of(list(src))]
    assert sorted(parents) == sorted([(2 ** 30 - 1, -2 ** 30, 0), (-2 ** 30, 2 ** 30 - 1, -1), (-1, -1, -1), (0, 0, 0)])
    for key, n_children in (((2 ** 30 - 1, -2 ** 30, 0), 2), ((-2 ** 30, 2 ** 30 - 1, -1), 1)):
        data, n, any_child = CM.coarsen_chunk(src, key, 8, FILL)
        assert any_child and np.count_nonzero(n == 8) == n_children * 32 ** 3
    for key in T.KEY_END_LISTED:
        assert all(not T.IMIN <= 2 * key[0] + c <= T.IMAX for c in (0, 1))  # both x children beyond int32
        assert not CM.coarsen_chunk(src, key, 8, FILL)[2]
    # without the check the last two would find chunks of SRC: the scene sees that mutant
    hits = [sum(c in src for c in T.wrapped_children(key)) for key in T.KEY_END_LISTED]
    assert hits == [0, 0, 2, 1], hits
    # -1 stays -1, INT32_MIN halves, through three levels
    k = np.array([[-1, T.IMIN, T.IMAX]])
    for want in ([-1, -2 ** 30, 2 ** 30 - 1], [-1, -2 ** 29, 2 ** 29 - 1], [-1, -2 ** 28, 2 ** 28 - 1]):
        k = CM.parents_of(k)
        assert k.tolist() == [want]


def test_plan_rows_and_words():
    """a plan row is 12 words and a table holds 8192: 682 rows fit, 683 do not, word 8192 lies in row 682, 700 rows are 8400 words"""
    R, W = T.ROW_WORDS, T.TABLE_WORDS
    assert 682 * R <= W < 683 * R and 682 * R <= 8192 < 683 * R and W // R == 682
    assert T.PLAN_ROWS * R == 8400 > W and T.PLAN_ROWS <= 3 * 256  # three segments of the default pool
    rows = T.plan_rows()
    assert len(rows) == 8 == len(set(rows)) and set(T.PLAN_FIXED_ROWS) <= set(rows) and rows == sorted(rows)
    assert all(b - a > 2 or (a, b) in ((681, 682), (682, 683)) for a, b in zip(rows, rows[1:]))  # the drawn rows have fill either side
    children = [T.plan_child(row, j) for j, row in enumerate(rows)]
    assert sorted({(c[0] & 1, c[1], c[2]) for c in children}) == sorted((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1))
    assert [tuple(int(v) for v in CM.parents_of([c])[0]) for c in children] == [(row, 0, 0) for row in rows]
    # a present parent without a child counts as processed with no voxel valued, and turns to fill
    out, stats = CM.coarsen({(5, 0, 0): np.zeros(CM.CW, dtype=np.uint32)}, {children[0]: T.observed(1)}, [(5, 0, 0)], 8, FILL)
    assert stats == [1, 0, 0, 0] and np.all(out[(5, 0, 0)] == FILL)
