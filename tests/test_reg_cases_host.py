"""The case table of tests/reg_cases.py proved on the CPU oracle alone: every window, cloud and pose exercises what it claims.
These are conditions on the INPUTS of tests/test_gpu_reg_routes.py: if one fails, the table changes, never the condition."""
import numpy as np
import pytest

import oracle_lib as O
import reg_cases as RC

CROSS_LIMIT = 0x7F7F7F80  # beyond it a signed-limb split without a bias fails (test_loop_sums_on_a_map_of_arbitrary_entries)


def _sides(k):
    return ((-1, f"{k}lo"), (1, f"{k}hi"))


def test_windows_are_the_table():
    """sizes, positions and offsets as the table states them; E is what three LocalMap.shift calls leave of a scanned map"""
    for cid in "ABCD":
        c, spec = RC.case(cid), RC.WINDOWS[cid]
        assert list(c.om.size) == list(spec["size"]) and list(c.om.pos) == list(spec["pos"]) and list(c.om.offset) == list(spec["offset"])
        v, w = O.unpack(c.om.data)
        if cid != "B":
            assert v.min() == -32768 and v.max() == 32767 and (w < 0).any() and 0.15 < np.mean(w == 0) < 0.25
    e = RC.case("E")
    assert list(e.om.pos) == list(RC.e_positions()[-1]) == [-2, 6, -1]
    assert list(e.om.offset) == [(32 + p) % 65 for p in (-2, 6, -1)] and all(o != 32 for o in e.om.offset)
    assert np.count_nonzero(O.unpack(e.om.data)[1]) > e.om.n_vox // 8  # the scan is still in the window
    assert RC.case("B").half.tolist() == [1, 1, 1]  # lim = size/2 - 1 = 0
    d = RC.case("D")
    assert (np.abs(d.om.pos[:2]) + d.half[:2] < RC.REACH_MM).all() and (np.abs(d.om.pos[:2]) + d.half[:2] > RC.REACH_MM - 8).all()


@pytest.mark.parametrize("cid", RC.IDS)
def test_every_named_edge_class_is_there_under_the_identity(cid):
    c = RC.case(cid)
    om, res, T = c.om, c.res, c.poses[0]
    assert np.array_equal(T, np.eye(4))
    q, exact = RC.transform_exact(T, c.edge)
    plain = np.abs(c.edge.astype(np.int64)).max(axis=1) < RC.REACH_MM
    assert np.array_equal(q[plain], c.edge[plain])  # q == p exactly for |p| < 65 536
    b = RC.voxel_of(q, res)
    admitted = np.asarray(O.calc_jacobis(c.all_observed(), T, c.edge, res)[2]).astype(bool)  # in_bounds_with_buffer_neg(1) alone
    counted = np.asarray(O.calc_jacobis(om, T, c.edge, res)[2]).astype(bool)
    in_window = np.array([om.in_bounds(*(int(v) for v in bi)) for bi in b])
    pos, half, size = om.pos.astype(np.int64), c.half, om.size.astype(np.int64)
    assert counted[0] and c.classes["centre"][0] == 0  # a cloud of one point is not an empty sum
    for k in range(3):
        for side, tag in _sides(k):
            i = c.classes[f"last_{tag}"]   # the last admitted voxel pos +- (size/2 - 1)
            assert (b[i, k] == pos[k] + side * (half[k] - 1)).all() and admitted[i].all(), (cid, tag)
            if cid != "E":  # (the slabs that entered E with the shifts are unobserved)
                assert counted[i].any(), (cid, tag)
            i = c.classes[f"refused_{tag}"]  # the first refused voxel pos +- size/2: inside the window, not admitted
            assert (b[i, k] == pos[k] + side * half[k]).all() and in_window[i].all() and not admitted[i].any(), (cid, tag)
        for ring, tag in ((0, "ring0"), (size[k] - 1, "ringmax")):
            i = c.classes[f"{tag}_{k}"]
            assert in_window[i].all() and all(c.ring_coordinate(b[j])[k] == ring for j in i), (cid, tag, k)
            # where the window's geometry lets a point's own voxel have that ring coordinate, one does and is admitted
            d = (ring - int(om.offset[k])) % size[k]
            d = d - size[k] if d > half[k] else d
            assert admitted[i].all() == (abs(d) <= half[k] - 1), (cid, tag, k)
        i = c.classes[f"wrap_identity_{k}"]
        assert (q[i] != exact[i]).any(axis=1).all() and admitted[i].all(), (cid, k)
        if cid == "C":
            for v in (0, 1, -1, res - 1, -(res - 1), res, -res, res + 1, -(res + 1)):
                i = c.classes[f"q{v:+d}_{k}"]
                assert (q[i, k] == v).all() and admitted[i].all() and (b[i, k] == (0 if abs(v) < res else np.sign(v))).all(), (v, k)
    if cid == "C":  # truncation toward zero: voxel 0 is 2 res - 1 wide
        assert RC.voxel_of([-(res - 1), res - 1, -res, res], res).tolist() == [0, 0, -1, 1]
    # ring wraps among the neighbours that are READ: the voxels next to ring coordinate 0 / size - 1 are admitted somewhere
    ring = np.array([c.ring_coordinate(bi) for bi in b[admitted]])
    for k in range(3):
        assert ((ring[:, k] == 0) | (ring[:, k] == size[k] - 1) | (ring[:, k] == 1) | (ring[:, k] == size[k] - 2)).any(), (cid, k)


@pytest.mark.parametrize("cid", RC.IDS)
def test_every_pose_of_every_case_counts_points(cid):
    c = RC.case(cid)
    assert len(c.edge) <= 513  # every count from 513 up holds the whole edge set
    for n in RC.COUNTS_HOST:
        q = c.cloud(n)
        assert q.shape == (n, 3) and np.array_equal(q[:min(n, len(c.edge))], c.edge[:n])
        for pi, T in enumerate(c.poses):
            count = O.reg_iterate(c.om, T, q, c.res)[3]
            assert 0 <= count <= n
            if pi == 0 or n >= 65:
                assert count > 0, (cid, n, pi)
    # both other poses: points that arrive plainly and points for which the int32 transform wraps, some of each counted
    for pi in (1, 2):
        q, exact = RC.transform_exact(c.poses[pi], c.edge)
        counted = np.asarray(O.calc_jacobis(c.om, c.poses[pi], c.edge, c.res)[2]).astype(bool)
        wrapped = (q != exact).any(axis=1)
        assert wrapped[c.classes[f"pose{pi}_wrapped"]].all() and counted[c.classes[f"pose{pi}_wrapped"]].any(), (cid, pi)
        assert not wrapped[c.classes[f"pose{pi}_plain"]].any() and counted[c.classes[f"pose{pi}_plain"]].any(), (cid, pi)


@pytest.mark.parametrize("cid", ["A", "C", "E"])
def test_a_quarter_of_the_body_is_counted(cid):
    c = RC.case(cid)
    assert O.reg_iterate(c.om, c.poses[0], c.body, c.res)[3] >= len(c.body) / 4
    q = c.cloud(3075)
    assert O.reg_iterate(c.om, c.poses[0], q, c.res)[3] >= len(q) / 4


def test_window_a_uses_the_whole_width_of_the_arithmetic():
    c = RC.case("A")
    q = c.cloud(513)
    J = np.asarray(O.calc_jacobis(c.om, c.poses[2], q, c.res)[0]).astype(np.int64)
    assert (J[:, :3] > CROSS_LIMIT).any() and (J[:, :3] < -CROSS_LIMIT).any()
    for n in (513, 3075):
        for T in c.poses:
            assert np.abs(O.reg_iterate(c.om, T, c.cloud(n), c.res)[0]).max() > 2 ** 50, n


def test_window_b_admits_one_voxel():
    c = RC.case("B")
    for n in RC.COUNTS_HOST:
        q = c.cloud(n)
        for T in c.poses:
            counted = np.asarray(O.calc_jacobis(c.om, T, q, c.res)[2]).astype(bool)
            assert counted.sum() <= n
            b = RC.voxel_of(RC.transform_exact(T, q)[0], c.res)
            assert (b[counted] == c.om.pos).all()
    # and the sums there are not trivially zero: the neighbours, every one a ring wrap, give a gradient
    h = O.reg_iterate(c.om, c.poses[0], c.cloud(65), c.res)[0]
    assert np.abs(h).max() > 0
    assert sorted(c.ring_coordinate(c.om.pos).tolist()) == [0, 1, 2]  # the voxel's own ring coordinates: first, interior, last


def test_window_d_counts_points_whose_transform_wrapped():
    c = RC.case("D")
    q3075 = c.cloud(3075)
    for T in c.poses:
        q, exact = RC.transform_exact(T, q3075)
        wrapped = (q != exact).any(axis=1)
        counted = np.asarray(O.calc_jacobis(c.om, T, q3075, c.res)[2]).astype(bool)
        assert wrapped.any() and (wrapped & counted).any()
        assert np.abs(q).max() <= RC.REACH_MM


def test_loops_run_and_end_on_different_causes():
    causes = {}
    for cid, n in [("A", 3075), ("C", 3075), ("E", 3075), RC.LOOP_THAT_EMPTIES]:
        c = RC.case(cid)
        T, it, cause, trace = RC.loop_end(c.om, c.cloud(n), c.poses[1], 6, c.res)
        assert it >= 2 and int(trace[0][43]) > 0, (cid, n, it)
        causes[cid, n] = cause
    assert causes["A", 3075] == causes["E", 3075] == "cut" and causes[RC.LOOP_THAT_EMPTIES] == "empty", causes
    assert RC.LOOP_THAT_EMPTIES[0] in "ACE" and RC.LOOP_THAT_EMPTIES[0] != "A"  # two cases between them, two causes


@pytest.mark.parametrize("cid", RC.IDS)
def test_loop_poses_stay_inside_the_float_to_int_conversion(cid):
    """(int)(T * 32768) is defined for |translation| < 65 536 mm only: beyond it the oracle (x86) and a GPU convert differently, and
    a comparison of the two would test the C standard's undefined behaviour, not a kernel"""
    c = RC.case(cid)
    for n in RC.COUNTS_ALL + ([RC.LOOP_THAT_EMPTIES[1]] if cid == RC.LOOP_THAT_EMPTIES[0] else []):
        for max_it in range(1, max(RC.LOOP_LIMITS) + 1):  # every pose a loop of at most 6 iterations passes through
            for k, P in enumerate(c.batch_poses()):  # (pose 1 starts the loops, all seven the batch)
                T, it, cause, trace = RC.loop_end(c.om, c.cloud(n), P, max_it, c.res)
                assert np.isfinite(T).all() and np.abs(T[:3, 3]).max() < RC.REACH_MM - 1 and np.abs(T[:3, :3]).max() < 2, (cid, n, max_it, k)
