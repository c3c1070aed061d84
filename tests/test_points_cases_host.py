"""The case table of tests/points_cases.py proved on the CPU alone: every class occurs and reaches what it claims.  These are
conditions on the INPUTS of tests/test_gpu_points_units.py: if one fails, the table changes, never the condition."""
import numpy as np

import points_cases as P
import reg_cases as R


def test_gradient_lists_hold_the_edges():
    vals, weights = (set(int(v) for v in a) for a in P.gradient_lists())
    assert {-32768, -32767, -1, 0, 1, 2, 32766, 32767} <= vals and {0, 1, -1, -32768} <= weights
    pairs = [(a, b) for a in vals for b in vals]
    assert any(a > 0 > b for a, b in pairs) and any(a < 0 < b for a, b in pairs)          # strictly opposite signs
    assert any(a == 0 and b != 0 for a, b in pairs) and any(b == 0 and a != 0 for a, b in pairs)  # product 0, signs not opposite
    same = [(a, b) for a, b in pairs if not (a > 0 > b or a < 0 < b)]
    assert any((a - b) % 2 and a - b > 0 for a, b in same) and any((a - b) % 2 and a - b < 0 for a, b in same)  # truncation toward zero
    # the restatement truncates toward zero and refuses opposite signs and unobserved neighbours
    e = P.entry
    assert int(P.central_gradient(e(2, 1), e(-1, 1))) == 0 and int(P.central_gradient(e(0, 1), e(-1, 1))) == 0
    assert int(P.central_gradient(e(-1, 1), e(0, 1))) == 0 and int(P.central_gradient(e(-3, 1), e(0, -1))) == -1
    assert int(P.central_gradient(e(3, 1), e(0, 1))) == 1 and int(P.central_gradient(e(3, 0), e(0, 1))) == 0
    assert int(P.central_gradient(e(-32768, 1), e(-1, 1))) == -16383 and int(P.central_gradient(e(0, 1), e(-32768, 1))) == 16384
    assert P.gradient_cases() == (len(vals) * len(weights)) ** 2


def test_point_terms_cases_hold_the_edges():
    G = P.point_terms_cases().astype(np.int64)
    J, v, used = P.point_terms(G)
    q = P.wrap32(G[:, :3])
    assert len(G) == 7 ** 3 * len(P.V_VALUES) * len(P.GRADIENT_SETS) * len(P.STATES)
    for k in range(3):
        assert {0, 1, -1, 65535, -65535, P.INT32_MIN, P.INT32_MAX} <= set(int(x) for x in np.unique(q[:, k]))
    ok, observed = G[:, 10] != 0, (G[:, 3] >> 16) != 0
    assert (~ok).any() and (ok & ~observed).any() and (ok & observed).any()
    assert not J[~(ok & observed)].any() and not v[~(ok & observed)].any() and not used[~(ok & observed)].any()
    assert {-32768, -1, 0, 32767} <= set(int(x) for x in np.unique(v[used != 0]))
    n_axes = (J[:, 3:6] != 0).sum(axis=1)
    assert (n_axes[used != 0] == 1).any() and (n_axes[used != 0] == 3).any()
    # some product wraps: the cross terms are compared as wrapped
    g = J[:, 3:6]
    assert (np.abs(q[:, 1].astype(object) * g[:, 2].astype(object)) >= 2 ** 31).any()


def test_gradient_entries_give_the_gradient():
    for g in (-16383, -2, -1, 0, 1, 2, 12345, 16383, 16384):
        assert int(P.central_gradient(*P.gradient_entries(g))) == g


def test_patterns_hold_every_class_and_value():
    pats = P.patterns()
    by_cls = {c: [p for p in pats if p.cls == c] for c in P.PATTERN_CLASSES}
    assert all(by_cls[c] for c in P.PATTERN_CLASSES) and sum(len(v) for v in by_cls.values()) == len(pats)
    assert P.PASSES == 2 and len({p.G.tobytes() for p in pats}) == len(pats)  # (g): the second pass has other data
    want = {0, 1, -1, P.BIAS, -P.BIAS, 0x7f7f7f7f, 0x7f7f7f80, 0x7f7f7f81, -0x7f7f7f7f, -0x7f7f7f80, -0x7f7f7f81, P.INT32_MAX, P.INT32_MIN}
    want |= {b << s for b in (0x7f, 0x80, 0xff, 0x100) for s in (0, 8, 16)}
    assert want <= set(P.J_VALUES)
    # (a) every listed value in all 64 lanes of a wave, in each of the rows J[0..2], for v = -32768 and 32767
    seen = set()
    for p in by_cls["a_same"]:
        J, v, used = p.terms()
        assert used.all() and len(set(int(x) for x in v)) == 1
        for w in range(P.WAVES):
            Jw = J[64 * w:64 * w + 64]
            assert (Jw == Jw[0]).all()
            for r in range(3):
                seen.add((r, int(Jw[0, r]), int(v[0])))
    assert {(r, val, v) for r in range(3) for val in P.J_VALUES if val for v in (-32768, 32767)} <= seen
    # (b) a single non-zero lane per wave, at every lane position, for each of the six rows
    singles = set()
    for p in by_cls["b_single"]:
        J, v, used = p.terms()
        for w in range(P.WAVES):
            lanes = np.flatnonzero(J[64 * w:64 * w + 64].any(axis=1))
            assert len(lanes) == 1
            for r in np.flatnonzero(J[64 * w + lanes[0]]):
                singles.add((int(lanes[0]), int(r)))
    assert singles == {(lane, r) for lane in range(64) for r in range(6)}
    # (c) neighbouring lanes hold extremes of opposite sign
    for p in by_cls["c_alternate"]:
        J = p.terms()[0]
        rows = J[:, :3]
        assert (np.sign(rows[0::2]) * np.sign(rows[1::2]) <= 0).all() and (np.abs(rows).max(axis=1) >= P.BIAS).all()
    assert any((p.terms()[0] == P.INT32_MIN).any() and (p.terms()[0] == P.INT32_MAX).any() for p in by_cls["c_alternate"])
    # (e) waves of 0, 1, 63, 64 valid points at either end; the lanes without a point hold data all the same
    counts = set()
    for p in by_cls["e_partial"]:
        ok = (p.G[:, 10] != 0).reshape(P.WAVES, 64)
        assert (ok == ok[0]).all() and (ok.all() or p.G[~ok.reshape(-1), :10].any())
        n = int(ok[0].sum())
        counts.add((n, "low" if ok[0, :n].all() else "high"))
        counts.add((n, "high" if ok[0, 64 - n:].all() else "low"))
    assert counts >= {(n, end) for n in (0, 1, 63, 64) for end in ("low", "high")}
    # (f) 1, 2, 4 and 8 waves
    assert sorted(p.waves for p in by_cls["f_waves"]) == [1, 2, 4, 8] and all(p.waves == 8 for p in pats if p.cls != "f_waves")


def test_class_a_reaches_the_largest_limb_product_and_totals_wrap():
    a = [p for p in P.patterns() if p.cls == "a_same"]
    best = 0
    for p in a:
        L = P.limbs(p.terms()[0][:64])  # [lane, row, limb] of wave 0
        L = L.reshape(64, 24)
        best = max(best, int(np.abs(L.T @ L).max()))  # C[a][b] = sum over the wave's 64 points of limb a x limb b
    assert best == 64 * 128 * 128
    assert all(int(np.abs(P.limbs(p.terms()[0])).max()) <= 128 for p in P.patterns())
    assert any(max(abs(t) for t in P.exact_totals(p)) > 2 ** 63 for p in a)
    # the restated terms give the values the lanes were built for
    p = next(p for p in a if p.name.startswith("-0x80000000"))
    assert (p.terms()[0][:64, 1:3] == P.INT32_MIN).all()


def test_gather_sequences_hold_the_four_kinds_of_point():
    assert [w.id for w in P.gather_windows()] == list(R.IDS) and P.STEP_NAMES == ["pose0", "nudged", "pose1", "pose0", "out", "pose0", "pose2"]
    for w in P.gather_windows():
        adm, vox = w.admitted, w.voxel
        assert len(w.points) == P.GATHER_POINTS and len(w.poses) == len(P.STEP_NAMES)
        assert np.array_equal(w.expect[0], w.expect[3]) and np.array_equal(w.expect[0], w.expect[5])
        same = (vox[0] == vox[1]).all(axis=1)
        assert (adm[0] & adm[1] & same).any(), w.id                       # stays in its voxel
        if w.id != "B":                                                  # (B admits one voxel)
            assert (adm[0] & adm[1] & ~same).any(), w.id                  # changes voxel
        assert (adm[3] & ~adm[4] & adm[5]).any(), w.id                    # leaves the window and returns
        assert (adm[1] != adm[2]).any() or w.id == "B", w.id              # enters or leaves between two poses of the case
        assert w.expect[:, :, 7].any(axis=1)[[0, 1, 2, 3, 5, 6]].all(), w.id  # every pose of the case counts points
        # ring coordinates 0 and size - 1 on each axis: at the voxel itself where the window admits that voxel (the margin of one
        # keeps the outermost layer for the neighbours: C's y offset puts both there), and read as a neighbour otherwise
        size, pos, off = (a.astype(np.int64) for a in (w.om.size, w.om.pos, w.om.offset))
        ring = (vox - pos + off + size) % size
        lim = size // 2 - 1
        for k in range(3):
            for r in (0, int(size[k]) - 1):
                d = (r - off[k]) % size[k]
                d = d - size[k] if d > size[k] // 2 else d
                at_voxel = (adm & (ring[:, :, k] == r)).any()
                as_neighbour = (adm & (((ring[:, :, k] + 1) % size[k] == r) | ((ring[:, :, k] - 1) % size[k] == r))).any()
                assert (at_voxel or as_neighbour) and (at_voxel or abs(d) > lim[k]), (w.id, k, r)
        if w.id == "B":
            assert (size == 3).all() and adm.any() and (vox[adm] == w.om.pos).all()
        # the oracle's mask implies admission, and the ring coordinate above is the oracle's index
        assert not (w.expect[:, :, 7].astype(bool) & ~adm).any()
        s, i = np.argwhere(adm)[0]
        assert w.case.ring_coordinate(vox[s, i]).tolist() == ring[s, i].tolist()


def test_counts_and_case_file(tmp_path):
    points, exchange = P.expected_counts()
    assert len(points) == 8 and len(exchange) == 5 and all(v > 0 for v in {**points, **exchange}.values())
    assert len(P.EXCHANGE_PRESETS) == 7 and len(P.EXCHANGE_TOTALS) == 4
    path = tmp_path / "points_cases.bin"
    P.write_case_file(str(path))
    head = np.fromfile(str(path), dtype=np.int32, count=8)
    assert head[0] == P.MAGIC and head[4] == len(P.patterns()) and head[5] == 5
    assert path.stat().st_size < 32 << 20
