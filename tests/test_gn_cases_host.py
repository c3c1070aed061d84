"""The case table of tests/gn_cases.py proved on the CPU oracle alone: every class occurs and does what it claims.  These are
conditions on the INPUTS of tests/test_gpu_gn_units.py: if one fails, the table changes, never the condition.  What an update does
is read from the oracle's own solve of its sums (Update.xi / theta / pivots), not from the target the sums were built from."""
import collections

import numpy as np

import gn_cases as G

DROP_CAP = 0.01  # share of the generated sequences that may be dropped for a non-finite expected pose


def _updates(cls=None, tag=None):
    for s in G.sequences():
        if cls is None or s.cls == cls:
            for k, u in enumerate(s.updates):
                if tag is None or tag in u.tags:
                    yield s, k, u


def _pose_unchanged(u):
    return np.array_equal(u.before[:16], u.after[:16])


def test_every_class_occurs_and_few_sequences_are_dropped():
    kept = collections.Counter(s.cls for s in G.sequences())
    dropped = G.dropped()
    assert sorted(kept) == sorted(G.CLASSES), set(G.CLASSES) ^ set(kept)  # no class is left out, whatever was dropped
    assert sum(dropped.values()) <= DROP_CAP * G.generated(), dropped
    assert len(G.sequences()) + sum(dropped.values()) == G.generated() and 2000 <= len(G.sequences()) <= 5000
    for s in G.sequences():
        assert 1 <= len(s.updates) <= G.MAX_UPDATES
    # the subset the C ABI routes run holds every class as well
    assert sorted({s.cls for s in G.subset()}) == sorted(G.CLASSES) and 100 <= len(G.subset()) <= 400


def test_no_expected_state_holds_a_non_finite_pose():
    for s, k, u in _updates():
        assert np.isfinite(u.after[:16].view(np.float32)).all(), (s.cls, k)
        assert np.isfinite(u.after[16:21].view(np.float32)).all(), (s.cls, k)  # alpha and the error history


def test_slots_and_words_are_those_of_the_reduction():
    """29 slots -> 44 words: h column-major from the upper triangle, g, and the low words of e and c"""
    assert [G.word_slot(k) for k in (0, 1, 6, 7, 35, 36, 41, 42, 43)] == [0, 1, 1, 6, 20, 21, 26, 27, 28]
    assert sorted(set(G.word_slot(k) for k in range(44))) == list(range(29))
    for s, k, u in _updates():
        h = u.words[:36].reshape(6, 6)
        assert np.array_equal(h, h.T)
        assert int(u.words[42]) == u.e and int(u.words[43]) == u.c and -2 ** 31 <= u.e < 2 ** 31 and -2 ** 31 <= u.c < 2 ** 31


def test_theta_of_every_targeted_update_lies_in_its_interval():
    seen = collections.Counter()
    for s, k, u in _updates():
        if not u.stepped:
            continue
        th = u.theta()
        for tag in u.tags:
            if tag in G.THETA_INTERVALS:
                assert G._in(th, tag), (s.cls, k, tag, th)
                seen[tag] += 1
    assert set(seen) == set(G.THETA_INTERVALS), seen
    # each side of the branch, the branch point and its neighbours in numbers
    assert seen["small"] > 1000 and seen["large"] > 800 and seen["tiny"] >= 100 and seen["quarter_exact"] >= 24
    assert seen["quarter_below"] >= 48 and seen["quarter_above"] >= 100 and seen["huge"] >= 30 and seen["zero"] >= 40
    # theta == 0: a pure translation
    for s, k, u in _updates(tag="zero"):
        xi = u.xi()
        assert (xi[:3] == 0).all() and (xi[3:] != 0).any() and u.stepped
        R = u.after[:16].view(np.float32).reshape(4, 4).T[:3, :3]
        assert np.array_equal(R, u.before[:16].view(np.float32).reshape(4, 4).T[:3, :3])
    # the neighbours of 0.25 below it, ulp by ulp
    below = sorted({round((0.25 - u.theta()) / G.QUARTER_ULP) for s, k, u in _updates(tag="quarter_below")})
    assert below == list(range(1, 9)), below
    # and the first doubles above it
    above = {round((u.theta() - 0.25) / (2 * G.QUARTER_ULP)) for s, k, u in _updates(tag="quarter_above")}
    assert {1, 2, 3, 4, 5} <= above, sorted(above)[:8]


def test_axes_and_sign_patterns():
    for s, k, u in _updates("axis_aligned"):
        if u.stepped:
            assert np.count_nonzero(u.xi()[:3]) == 1, (k, u.xi())
    axes = {(int(np.argmax(np.abs(u.xi()[:3]))), float(np.sign(u.xi()[:3].sum()))) for s, k, u in _updates("axis_aligned") if u.stepped}
    assert len(axes) == 6
    for branch in ("small", "large"):
        patterns = {tuple(np.signbit(u.xi()).tolist()) for s, k, u in _updates("sign_patterns", branch)}
        assert len(patterns) == 64, (branch, len(patterns))
    general = sum(1 for s, k, u in _updates("large_theta") if u.stepped and np.count_nonzero(u.xi()[:3]) == 3)
    assert general > 400


def test_pose_history():
    far = [s for s in G.sequences() if s.cls == "far_pose"]
    assert all(20000 <= np.abs(s.T0[12:15]).max() <= 60000 for s in far)
    for s in G.sequences():
        assert np.abs(s.T0[12:15]).max() <= 60000
    # sequences that carry T, alpha and prev forward: eight stepped updates, alpha grown, the history full
    full = [s for s in G.sequences() if s.cls == "history"]
    assert len(full) >= 200
    for s in full:
        assert len(s.updates) == 8 and all(u.stepped for u in s.updates)
        last = s.updates[-1]
        assert last.alpha_before > 0 and (last.after[17:21].view(np.float32) != 0).all() and int(last.after[21]) == 8
        for a, b in zip(s.updates, s.updates[1:]):
            assert np.array_equal(a.after, b.before) and not _pose_unchanged(b)


def test_e_and_c_cases():
    for cls in ("c_zero_first", "c_zero_later"):
        n = 0
        for s, k, u in _updates(cls, "c_zero"):
            assert u.c == 0 and u.live and (k == 0) == (cls == "c_zero_first")
            assert int(u.after[22]) == 1 and int(u.after[21]) == int(u.before[21]) + 1  # finished, and counted as an iteration
            assert np.array_equal(u.before[:21], u.after[:21])  # pose, alpha and history bit-unchanged
            n += 1
        assert n >= 20
        assert any(int(u.slots[28]) != 0 for s, k, u in _updates(cls, "c_zero"))  # c == 0 as the low word of a larger total
    cs = collections.Counter((u.c, u.alpha_before > 0) for s, k, u in _updates("c_values") if u.stepped)
    for c in (1, 2 ** 24 + 1, 2 ** 31 - 1):
        assert cs[c, False] >= 10 and cs[c, True] >= 20, cs
    # (float)c is not c at the two large values, and the damping they make is part of the matrix
    assert float(np.float32(2 ** 24 + 1)) != 2 ** 24 + 1 and float(np.float32(2 ** 31 - 1)) != 2 ** 31 - 1
    n = 0
    for s, k, u in _updates("c_high_word"):
        assert int(u.slots[28]) >> 32 >= 1 and u.c == int(u.slots[28]) & 0xffffffff and u.c > 0 and u.stepped
        n += 1
    assert n >= 40
    n = 0
    for s, k, u in _updates("e_high_word"):
        total = int(u.slots[27])
        assert u.e < 0 and total > 0 and (total >> 32) != -1 and u.stepped
        assert u.after[20].view(np.float32) == np.float32(u.e) / np.float32(u.c) < 0  # the error the history took is the low word's
        n += 1
    assert n >= 40


def test_singular_systems_finish_with_the_pose_untouched():
    for cls in ("singular_zero", "singular_rank"):
        first = later = 0
        for s, k, u in _updates(cls, "singular"):
            rc, _ = u.solve()
            assert rc != 0 and u.live and u.c != 0 and u.alpha_before == 0
            assert int(u.after[22]) == 1 and int(u.after[21]) == int(u.before[21]) + 1
            assert np.array_equal(u.before[:21], u.after[:21])
            if cls == "singular_zero":
                assert not u.words[:36].any()
            else:
                assert u.words[:36].any() and np.linalg.matrix_rank(u.words[:36].reshape(6, 6).astype(np.float64)) < 6
            first += k == 0
            later += k > 0
        assert first >= 8 and later >= 8, (cls, first, later)


def test_zero_h_with_damping_is_not_singular():
    n = 0
    for s, k, u in _updates("zero_h_damped", "zero_h"):
        assert not u.words[:36].any() and u.alpha_before > 0 and u.c > 0 and u.stepped and not _pose_unchanged(u)
        n += 1
    assert n >= 40


def test_both_pivot_outcomes_occur():
    """the Python restatement of the solve gives the oracle's x bit for bit, so its pivot rows are the oracle's"""
    for s, k, u in _updates():
        if u.live and u.c != 0:
            A, b = G.system(u.words, u.alpha_before)
            rc, x, piv = G.solve6_trace(A, b)
            rc_o, x_o = G.oracle_solve(A, b)
            assert rc == rc_o and (rc != 0 or np.array_equal(x.view(np.uint64), x_o.view(np.uint64))), (s.cls, k)
    kept = sum(1 for s, k, u in _updates() if u.stepped and u.pivots() == list(range(6)))
    assert kept > 5000  # the diagonal keeps its place in every step: one side of the ballot six times
    at = collections.Counter()
    for kind in ("first", "later", "tie"):
        for s, k, u in _updates("pivot_" + kind, "pivot_" + kind):
            piv = u.pivots()
            moved = [j for j in range(6) if piv[j] != j]
            if kind == "first":
                assert moved == [0], piv
            elif kind == "later":
                assert len(moved) == 1 and moved[0] >= 1, piv  # both sides of the ballot within one update
                at[moved[0]] += 1
            else:
                assert moved == [], piv
                j = int([t for t in u.tags if t.startswith("at")][0][2:])
                A, _ = G.system(u.words, u.alpha_before)
                assert abs(A[j + 1][j]) == abs(A[j][j])  # an exact tie (the block is reached unchanged: uncoupled from the rows above)
            assert u.stepped and u.alpha_before == 0
    assert sorted(at) == [1, 2, 3, 4], at


def test_large_sums_pass_2_to_the_53():
    n = 0
    for s, k, u in _updates("large_sums"):
        h, g = np.abs(u.words[:36].astype(object)), np.abs(u.words[36:42].astype(object))
        assert max(h) >= 2 ** 60 and max(h) < 2 ** 62 and max(g) > 2 ** 53 and u.stepped
        n += max(h) >= 2 ** 61
        # values that (double) has to round
        assert any(int(v) != int(float(int(v))) for v in u.words[:42])
    assert n >= 100


def test_convergence_at_and_next_to_epsilon():
    for kind in ("equal", "below", "one_fails"):
        seqs = [s for s in G.sequences() if s.cls == "converge_" + kind]
        assert len(seqs) >= 30
        orders = set()
        for s in seqs:
            u = s.updates[4]
            err = np.float32(u.e) / np.float32(u.c)
            prev = u.before[17:21].view(np.float32)
            d2, d0 = np.abs(err - prev[2]), np.abs(err - prev[0])
            assert all(int(v.after[22]) == 0 for v in s.updates[:4]) and u.stepped
            if kind == "equal":
                assert max(d2, d0) == s.epsilon and min(d2, d0) < s.epsilon and int(u.after[22]) == 0 and s.finish_at is None
            elif kind == "below":
                assert np.nextafter(max(d2, d0), np.float32(np.inf)) == s.epsilon and int(u.after[22]) == 1 and s.finish_at == 4
                assert np.array_equal(s.updates[5].before, s.updates[5].after)
            else:
                assert min(d2, d0) < s.epsilon <= max(d2, d0) and int(u.after[22]) == 0
            orders.add((bool(d2 > d0), bool(err > prev[2])))
            if kind != "below":
                assert s.updates[5].stepped
        assert len(orders) == 4, (kind, orders)  # either difference the larger one, either sign


def test_iteration_limits():
    limits = collections.Counter()
    for s in G.sequences():
        if s.cls == "max_iterations":
            assert len(s.updates) == 5 > s.max_iterations
            limits[s.max_iterations] += 1
            for k, u in enumerate(s.updates):
                assert u.live == (k < s.max_iterations) and int(u.after[21]) == min(k + 1, s.max_iterations) and int(u.after[22]) == 0
                if not u.live:
                    assert np.array_equal(u.before, u.after)
    assert sorted(limits) == [0, 1, 3] and min(limits.values()) >= 20
    causes = collections.Counter()
    for s in G.sequences():
        if s.cls == "after_finished":
            end = next(k for k, u in enumerate(s.updates) if int(u.after[22]) == 1)
            causes[s.updates[end].tags[0]] += 1
            for u in s.updates[end + 1:]:
                assert not u.live and np.array_equal(u.before, u.after)  # an update sent after `finished` changes nothing
            assert len(s.updates) - 1 - end == 2
    assert set(causes) == {"c_zero", "singular", "converge"} and min(causes.values()) >= 10, causes
