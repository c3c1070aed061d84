"""The numpy models of frontier, reach, distance and sample and the fixtures of tests/edge_domain_scenes.py where
tests/test_gpu_edge_domain.py leans on them, without a GPU: every model gives at the far, top, bottom and mixed bases exactly its
near result moved by whole voxels (a model that wrapped in int32 would not), and every fixture exercises its edge in the model
alone: the conditions (a) to (f) of the frontier scene, the kept and dropped seeds, the classes and gradients on the two sides of
the 2^30 plane, and the teeth of the adversarial chunk pairs."""
import numpy as np
import pytest

import distance_model as DM
import edge_domain_scenes as E
import frontier_model as FM
import query_model as QM
import reach_model as RM
import sample_model as H
import store_scenes as SM
import store_surface_scenes as SS

FAR = [b for b in E.BASES if b != "near"]


# ------------------------------------------------------------------------------------------------ frontier
@pytest.mark.parametrize("size", E.FRONTIER_SIZES, ids=str)
def test_bases_touch_the_ends_of_int32(size):
    ends = {name: QM.window(size, E.base_pos(size, name)) for name in E.BASES}
    assert np.all(ends["top"][1] == E.I32_MAX) and np.all(ends["bottom"][0] == E.I32_MIN)
    assert ends["mixed"][1][0] == E.I32_MAX and ends["mixed"][0][1] == E.I32_MIN and ends["mixed"][1][2] == E.I32_MAX
    if size[0] % 2 == 0:
        pos = E.base_pos(size, "top")
        assert int(pos[0]) + size[0] // 2 - 1 == E.I32_MAX  # an even window ends at pos + size/2 - 1


@pytest.mark.parametrize("name", E.BASES)
@pytest.mark.parametrize("size", E.FRONTIER_SIZES, ids=str)
def test_frontier_scene_meets_its_conditions_at_every_base(size, name):
    seen = E.check_frontier_scene(size, name)
    print(size, name, seen)


@pytest.mark.parametrize("name", FAR)
@pytest.mark.parametrize("size", E.FRONTIER_SIZES, ids=str)
def test_frontier_model_moves_with_the_window(size, name):
    import warpsense_amd as W
    s = E.shift(size, name)
    near, far = E.frontier_boxes(size, "near"), E.frontier_boxes(size, name)
    for (_, _, _, a0, b0), (box, _, _, a1, b1) in zip(near, far):
        assert np.array_equal(a1 - a0, s) and np.array_equal(b1 - b0, s)
        for min_value, any_weight in ((0, False), (E.TAU, False), (0, True), (E.TAU, True)):
            want = E.moved_frontier(E.frontier_model(size, "near", a0, b0, min_value, any_weight), s)
            got = E.frontier_model(size, name, a1, b1, min_value, any_weight)
            assert all(QM.same(g, w) for g, w in zip(got, want)), (box, min_value, any_weight)
            if box == "inner":
                assert len(got[0]) >= 200 and len(got[2]) >= 5
        mine, theirs = FM.goals(got[2], E.RES, 3), W.frontier_goals(got[2], E.RES, 3)
        assert len(mine[0]) >= 2 and all(np.array_equal(m, t) and m.dtype == t.dtype for m, t in zip(mine, theirs))
        assert np.all(np.abs(mine[0][:, 0] * 1000.0 / E.RES - (a1[0] + b1[0]) / 2.0) <= (b1[0] - a1[0]))  # centroids lie in the box, at every base


# ------------------------------------------------------------------------------------------------ reach and distance
REACH_CASES = [(kind, columns) for kind in E.REACH_SHAPES for columns in (False, True) if not (kind == "rooms" and columns)]


@pytest.mark.parametrize("name", E.BASES)
@pytest.mark.parametrize("kind,columns", REACH_CASES)
def test_reach_model_moves_and_seeds_are_kept_and_dropped_as_built(kind, columns, name):
    s = E.shift(E.REACH_SHAPES[kind], name)
    box, lo0, hi0, rec0, kept0, dropped0 = E.reach_scene(kind, "near", columns)
    box, lo, hi, rec, kept, dropped = E.reach_scene(kind, name, columns)
    assert np.array_equal(lo - lo0, s) and np.all(kept - kept0 == s) and QM.same(rec, rec0)
    n_faces = sum(1 for k in range(2 if columns else 3) for v in (lo[k] - 1, hi[k] + 1) if E.I32_MIN <= v <= E.I32_MAX)
    assert len(dropped) == 1 + n_faces + 2 and len(kept) == (1 if kind == "rooms" else 3)
    if name in E.EDGES:
        assert n_faces == (3 if not columns else 2 if name != "mixed" else 2)  # one face per axis has nothing beyond it
        assert np.abs(dropped[-2:] - lo).max() >= 2 ** 32 - 64                 # seed - lo needs 33 bits
    for clear_d2, unknown_free in ((0, False), (2, False), (0, True), (2, True)):
        seeds = np.concatenate([dropped[:3], kept, dropped[3:]])
        want, n_kept, reached = RM.field(rec, lo, seeds, clear_d2, unknown_free)
        near, _, _ = RM.field(rec0, lo0, seeds - s, clear_d2, unknown_free)
        assert n_kept == len(kept) and QM.same(want, near) and reached > 100
        assert RM.field(rec, lo, dropped, clear_d2, unknown_free)[1:] == (0, 0)
        assert np.all(RM.lookup(want, lo, dropped) == RM.INF) and np.all(RM.lookup(want, lo, kept) == 0)
        trav = RM.traversable(rec, clear_d2, unknown_free)
        goals = E.reach_goals(want, lo, hi, trav, columns)
        hdr, steps = RM.paths(want, lo, goals, 12)
        h0, s0 = RM.paths(near, lo0, goals - s * (np.array([1, 1, 0]) if columns else 1), 12)
        assert QM.same(hdr, h0)
        if kind != "rooms" or clear_d2 == 0:
            assert {0, 2} <= set(hdr["status"].tolist()) and np.any(hdr["steps"] + 1 > hdr["written"]), (clear_d2, unknown_free)
        if kind != "rooms" and not unknown_free:
            assert 1 in hdr["status"]  # the sealed corner
        written = np.arange(12)[None, :] < hdr["written"][:, None]
        at_end = []
        for k, n in enumerate("xy" if columns else "xyz"):
            assert np.array_equal(steps[n][written].astype(np.int64), s0[n][written].astype(np.int64) + s[k])
            end = E.I32_MAX if (name == "top" or (name == "mixed" and k != 1)) else E.I32_MIN
            at_end.append(bool(np.any(steps[n][written] == end)))
        if name in E.EDGES:  # record coordinates at the end of int32: on x or y always, on every axis where free space reaches that plane
            assert any(at_end[:2]) and (kind == "rooms" or all(at_end[:2])), at_end
        assert np.array_equal(steps["cost"], s0["cost"])
        if columns and name in ("top", "mixed"):
            assert goals[0][2] == E.I32_MIN and hdr["status"][0] == 0 and steps["z"][0, 0] == E.I32_MIN


def test_distance_model_does_not_know_where_the_box_is():
    """distance_model.model_box takes entries alone: the records of a box are those of the same entries anywhere.  Through a ring at an
    edge base (distance_model.model) they are the same bytes"""
    size = E.REACH_SHAPES["random_odd"]
    box = E.reach_box("random_odd")
    for name in E.BASES:
        pos = E.base_pos(size, name)
        lo, hi = QM.window(size, pos)
        ax = [(np.arange(lo[k], hi[k] + 1, dtype=np.int64) - pos[k] + E.OFFSET[k] + size[k]) % size[k] for k in range(3)]
        data = np.zeros(size, dtype=np.uint32)
        data[np.ix_(*ax)] = box
        view = type("V", (), dict(data_=data.reshape(-1), size_=np.asarray(size), pos_=pos, offset_=np.asarray(E.OFFSET)))
        for kw in ({}, dict(unknown_occupied=True), dict(columns=True)):
            assert DM.same(DM.model(view, 4, **kw)[0], DM.model_box(box, 4, **kw)[0]), (name, kw)


# ------------------------------------------------------------------------------------------------ sample
@pytest.mark.parametrize("case", E.SAMPLE_CASES, ids=E.sample_id)
def test_sample_fixture_and_model_on_both_sides_of_the_plane(case):
    """Per case and weight rule: at least 16 points of every class; at least 16 non-zero gradients among the live points within two
    voxels of the plane and 16 among the other live points; beyond the plane every point is dead: class 0, record and gradient zero,
    although the voxel of each 2^30 point is valid and inside the window; every 2^30 - 1 point is classed from a valid cell.  The same
    entries in a near window, the points moved by s res: the points live in both have the same records and gradients."""
    res, sign, axes = case
    pos, ring, pts, live, dead = E.sample_case(case)
    near_ring, near_pts, s = E.sample_near(case)
    both = E.live_in_both(case)
    is_dead = np.any(np.abs(pts) >= E.LIMIT, axis=1)
    close = np.zeros(len(pts), dtype=bool)
    for k in axes:
        close |= np.abs(np.abs(pts[:, k]) - E.LIMIT) <= 2 * res
    assert len(live) == len(dead) == 8 * len(axes)
    for any_weight in (False, True):
        rec, counts, grad, sel = H.model(ring, res, pts, E.BAND, any_weight, select=(H.FREE, H.SURFACE))
        nz = np.any(grad != 0, axis=1)
        print(E.sample_id(case), any_weight, counts.tolist(), int((nz & close).sum()), int((nz & ~close).sum()), int(is_dead.sum()), int(both.sum()))
        assert counts.min() >= 16 and (nz & close & ~is_dead).sum() >= 16 and (nz & ~close & ~is_dead).sum() >= 16
        assert is_dead.sum() >= 256 and not rec[is_dead].tobytes().strip(b"\0") and not grad[is_dead].any()
        assert np.all(rec["cls"][live] != H.UNKNOWN) and np.all(rec["weight"][live] > 0)
        raw, inside = H.raws(ring, pts[dead] // res)
        assert np.all(inside) and np.all(QM.unpack(raw)[1] > 0)  # dead although the voxel is valid and in the window
        assert not np.any(np.any(np.abs(sel.astype(np.int64)) >= E.LIMIT, axis=1)) and len(sel) == int(counts[H.FREE] + counts[H.SURFACE])
        near = H.model(near_ring, res, near_pts, E.BAND, any_weight)
        assert both.sum() >= 1000 and rec[both].tobytes() == near[0][both].tobytes() and np.array_equal(grad[both], near[2][both])
    for k in axes:
        assert np.any(np.abs(pts[live][:, k]) == E.LIMIT - 1) and np.any(np.abs(pts[dead][:, k]) == E.LIMIT)


# ------------------------------------------------------------------------------------------------ the store
@pytest.mark.parametrize("where", ("top", "bottom"))
def test_block_fixture_has_records_at_the_end_of_int32(where):
    chunks, near = E.block_chunks(where), E.block_chunks("near")
    end = E.I32_MAX if where == "top" else E.I32_MIN
    for i, (_, _, lo, hi) in enumerate(E.block_boxes(where)):
        want = E.store_frontier_model(chunks, lo, hi)
        assert len(want[0]) >= 200 and len(want[2]) >= 5
        for n in "xyz":
            assert np.count_nonzero(want[0][n] == end) >= 8, (where, n)
        if i == 0:  # the default box is the near block's box moved (the grown box is cut at the end of int32)
            lo0, hi0 = SM.bounding_box(near)
            assert np.array_equal(hi - lo, hi0 - lo0)
            assert all(QM.same(g, w) for g, w in zip(want, E.moved_frontier(E.store_frontier_model(near, lo0, hi0), lo - lo0)))
        else:
            assert np.count_nonzero((lo == E.I32_MIN) | (hi == E.I32_MAX)) == 3 and np.all(hi - lo == 2 * E.CS)
        rec, _ = SS.model_store(chunks, E.TAU, E.RES, lo, hi)
        assert len(rec) > 100 and any(np.any(rec[n] == end) for n in "xyz")
    heavy = np.all((1 if where == "top" else -1) * want[2]["sum"] > 2 ** 33, axis=1)
    assert heavy.any()


def test_adversarial_pairs_have_teeth():
    """x pair: in the box of all int32 the model sets neither the +x bit at INT32_MAX nor the -x bit at INT32_MIN; a model whose
    neighbour arithmetic wraps sets at least 64 of each.  y pair: two clusters; records whose y is turned so that INT32_MAX and
    INT32_MIN are neighbours, as a column search that wraps sees them, are one cluster fewer"""
    rec, labels, table = E.pair_model()
    top, bottom = rec["x"] == E.I32_MAX, rec["x"] == E.I32_MIN
    a = E.pair_pattern()
    assert top.sum() == a.sum() >= 64 and bottom.sum() == (~a).sum() >= 64
    assert not np.any(rec["mask"][top] & 2) and not np.any(rec["mask"][bottom] & 1)
    wrap = E.pair_records(wrap=True)
    assert np.count_nonzero(wrap["mask"][wrap["x"] == E.I32_MAX] & 2) >= 64 and np.count_nonzero(wrap["mask"][wrap["x"] == E.I32_MIN] & 1) >= 64
    in_y = (rec["y"] == E.I32_MAX) | (rec["y"] == E.I32_MIN)
    assert in_y.sum() == 800 and len(np.unique(labels[in_y])) == 2
    assert np.any(rec["y"][:-1].astype(np.int64) > rec["y"][1:].astype(np.int64))  # the two plates interleave in the record order
    assert len(FM.clusters(E.wrapped_y(rec))[1]) == len(table) - 1
    for key in E.pair_chunks():
        assert E.BOTTOM_KEY <= min(key) and max(key) <= E.TOP_KEY


def test_corner_box_of_the_top_block_is_the_near_corner_moved():
    a, b = E.corner_box("top")
    a0, b0 = E.corner_box("near")
    assert np.all(b == E.I32_MAX) and np.array_equal(SM.assemble(E.block_chunks("top"), a, b), SM.assemble(E.block_chunks("near"), a0, b0))
    rec, _ = DM.model_box(SM.assemble(E.block_chunks("top"), a, b), 4)
    assert np.count_nonzero(RM.traversable(rec, 1)) > 1000
