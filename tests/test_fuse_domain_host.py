"""CPU tests of the scenes of the fuse's domain tests (fuse_domain_scenes.py), on the model alone: the expectation that does not come
from the plan (fuse_model.fuse_at over fuse_model.receivers) equals the model that goes through it (fuse_model.fuse) in every scene;
the margin of receivers is checked, not assumed; the random poses keep the conditions that make them worth running; and every edge
scene's claim -- which voxels are live, dead, inside or outside -- holds.  test_gpu_fuse_domain.py runs the same scenes on the
device.  No GPU."""
import numpy as np
import pytest

import fuse_model as F
import fuse_domain_scenes as D
from edge_domain_scenes import BOTTOM_KEY, TOP_KEY
from fuse_scenes import FILL

Q30, REACH = F.Q30, F.REACH


def rows(a):
    return {tuple(int(c) for c in r) for r in np.asarray(a).reshape(-1, 3)}


@pytest.mark.parametrize("scene", D.scenes(), ids=lambda s: s["name"])
def test_fuse_at_over_receivers_is_the_models_fuse(scene):
    """chunks and stats[1:6] agree, and no voxel that receives a sample lies on the outermost shell of the margin: all of them are
    within margin - 1 voxels of a mapped SRC voxel"""
    want_at, want = D.expect(scene), D.expect_plan(scene)
    assert F.same_at(want, want_at), (want[1], want_at[1])
    got = rows(F.receiving(scene["src"], scene["pose"], scene["res"], scene["voxels"])[0])
    inner = rows(F.receivers(scene["src"], scene["pose"], scene["res"], margin=2))
    assert got <= inner and (got or scene.get("nothing"))


def test_random_poses_keep_their_conditions():
    cases = D.random_scenes()
    assert len(cases) >= 24 and [c["res"] for c in cases[:4]] == [1, 7, 64, 1000]
    assert sum(c["far"] for c in cases) == len(cases) // 2
    n_set = n_four = n_corner = n_avg = 0
    for c in cases:
        _, st = D.expect(c)
        v = F.receiving(c["src"], c["pose"], c["res"], c["voxels"])[0]
        _, per_chunk = np.unique(v >> 6, axis=0, return_counts=True)
        assert int(st[2]) > 0, c["name"]  # set > 0: no case is quiet
        assert np.all(np.abs(c["pose"][9:12].astype(np.int64)) <= 2 ** 22) and len(c["src"]) == 2 and len(c["dst"]) == 1
        n_set += 1
        n_four += len(per_chunk) >= 4
        n_corner += bool(np.any(per_chunk < 8))
        n_avg += int(st[1]) > 0
    print("set", n_set, "four or more chunks", n_four, "a chunk touched at a corner", n_corner, "averaged", n_avg)
    assert n_set == len(cases) and n_four >= 12 and n_corner >= 6 and n_avg >= 6


@pytest.mark.parametrize("scene", D.edge_scenes(), ids=lambda s: s["name"])
def test_edge_scene_claims(scene):
    """the voxels a scene says must receive do; those it says must not do not, for the stated reason and, where the scene says so,
    for no other: all eight corners of their cells are observed voxels of SRC.  q and p - pivot_dst come from the rule's formula in
    the scene module, not from the model's pull()."""
    D.expect(scene)
    res, pose = scene["res"], scene["pose"]
    v, nv, _ = F.receiving(scene["src"], pose, res, scene["voxels"])
    got = rows(v)
    if len(v):
        q, d = D.pull_exact(pose, res, v)
        assert np.all(np.abs(q) < Q30) and np.all(np.abs(d) < REACH)
        assert BOTTOM_KEY <= int((v >> 6).min()) and int((v >> 6).max()) <= TOP_KEY
    if scene.get("nothing"):
        assert not got and F.same_at((scene["dst"], [0] * 5), scene["want_at"])
    if "must" in scene:
        assert len(scene["must"]) and rows(scene["must"]) <= got
    if "must_not" in scene:
        bad = scene["must_not"]
        assert len(bad) and not (rows(bad) & got)
        q, d = D.pull_exact(pose, res, bad)
        if scene["why"] == "dead":
            assert np.all(np.any(np.abs(q) >= Q30, axis=1)) and np.all(np.abs(d) < REACH)
        else:
            assert np.all(np.any(np.abs(d) >= REACH, axis=1)) and np.all(np.abs(q) < Q30)
        if scene["covered"]:
            b = (q - res // 2) // res
            for c in np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.int64):
                raw, present = F.lookup(scene["src"], b + c)
                assert present.all() and np.all(F.unpack(raw)[1] > 0)
    if scene["name"].startswith("dead_"):
        # both sides of the boundary are there: the last live and the first dead component differ by one voxel
        axis = int(np.argmax(np.ptp(scene["must"], axis=0)))
        edge = {int(scene["must"][:, axis].min()), int(scene["must"][:, axis].max())} & {31, 32}
        assert edge and {int(scene["must_not"][:, axis].min()), int(scene["must_not"][:, axis].max())} & {31, 32}
        q_live = np.abs(D.pull_exact(pose, res, scene["must"])[0]).max()
        q_dead = np.abs(D.pull_exact(pose, res, scene["must_not"])[0]).max(axis=1).min()
        assert (q_live, q_dead) in ((Q30 - 1, Q30 - 1 + res), (Q30 - res, Q30))
    if scene["name"].startswith("pivot_src_beyond"):
        assert abs(int(pose[12])) == Q30 + 2 ** 23
    if scene["name"].startswith("reach_"):
        d = np.abs(scene["must"]).max(axis=1), np.abs(scene["must_not"]).max(axis=1)
        assert d[0].max() == REACH - 1 and d[1].min() == REACH
        for axis in range(3):
            for sign in (1, -1):
                assert np.any(scene["must"][:, axis] == sign * (REACH - 1)) and np.any(scene["must_not"][:, axis] == sign * REACH)
    if "keys_created" in scene:
        for key in scene["keys_created"]:
            assert key not in scene["dst"] and key in scene["want_at"][0]
            cube = scene["want_at"][0][key].reshape(64, 64, 64)
            last = 63 if key[0] == TOP_KEY else 0
            assert np.any(cube[last] != FILL) and (last, 0, 0) in {(x & 63, y, z) for x, y, z in got if x >> 6 == key[0]}
        assert all(BOTTOM_KEY <= k <= TOP_KEY for key in scene["want_at"][0] for k in key)
    if "value" in scene:
        sel = np.array([tuple(r) in rows(scene["must"]) for r in v.tolist()])
        assert np.all(nv[sel] == scene["value"]) and sel.sum() == len(scene["must"])
    if scene["name"].startswith("extremes"):
        before, after = scene["dst"][(0, 0, 0)], scene["want_at"][0][(0, 0, 0)]
        assert int((before != after).sum()) > 0 and int(scene["want_at"][1][1]) == 24 and int(scene["want_at"][1][2]) == 24


def test_a_plan_that_is_too_small_shows_against_fuse_at():
    """The point of an expectation that does not share the plan.  A plan that shrinks every chunk of SRC by two voxels misses a chunk
    of DST that receives a sample in some random-pose scene: the model that goes through such a plan -- and a device that shared it --
    no longer gives fuse_at's result.

    A growth of 0 instead of 2 voxels does not show, and cannot: a valid sample has its base voxel b in a present chunk, so q lies in
    that chunk's box, or above it by less than h on some axes, where f_k > 0 makes the corner b_k + 1 take part, which lies in the
    next chunk, present as well, whose box then holds q.  So q always lies in the box of a present chunk, p within the rounding
    (below 1 mm) of its image, and the 2 mm per side alone make the plan a superset.  The growth is spare generosity."""
    red = []
    for c in D.random_scenes():
        D.expect(c)
        received = rows(F.receiving(c["src"], c["pose"], c["res"], c["voxels"])[0] >> 6)
        assert received <= set(F.candidates(sorted(c["src"]), c["pose"], c["res"], grow=0)), c["name"]
        if received - set(F.candidates(sorted(c["src"]), c["pose"], c["res"], grow=-2)):
            red.append(c)
    print("random-pose scenes in which a plan shrunk by two voxels misses a receiving chunk:", [c["name"] for c in red])
    assert red
    small = F.fuse(red[0]["dst"], red[0]["src"], red[0]["pose"], red[0]["res"], red[0]["mw"], FILL, grow=-2)
    assert not F.same_at(small, D.expect(red[0])) and F.same_at(D.expect_plan(red[0]), D.expect(red[0]))
