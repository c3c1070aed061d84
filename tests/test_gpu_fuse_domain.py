"""ws_store_fuse on the scenes of fuse_domain_scenes.py: random rigid poses, and the edges of the call's domain -- the dead boundary
at |q| = 2^30, pivot_src beyond +-2^30, DST at the ends of int32 voxels, the 2^24 mm reach under a rotation, values and weights at
the ends of int16, WS_FUSE_COUNT_ONLY.  The device's key set, every chunk's bytes and stats[1:6] are compared bit for bit with
fuse_model.fuse_at over fuse_model.receivers, an expectation applied voxel by voxel that shares nothing with the chunk plan;
stats[0] with the length of the model's plan; and the edge scenes also with fuse_model.fuse.  test_fuse_domain_host.py holds every
scene to its claim on the model alone."""
import numpy as np
import pytest

import fuse_model as F
import fuse_domain_scenes as D
import fuse_scenes as S

pytestmark = pytest.mark.gpu


def run(scene):
    """the scene on the device: (DST's chunks after the call, stats)"""
    dst, src = S.make_store(scene["dst"]), S.make_store(scene["src"])
    st = dst.fuse(src, scene["pose"], scene["mw"], count_only=scene.get("count_only", False), resolution=scene["res"])
    got = S.read(dst)
    assert F.same_at((S.read(src), ()), (scene["src"], ()))  # SRC is only read
    dst.close()
    src.close()
    return got, st.as_tuple()


@pytest.mark.parametrize("scene", D.random_scenes(), ids=lambda s: s["name"])
def test_random_rigid_pose(scene):
    got, stats = run(scene)
    print(scene["name"], "res", scene["res"], "stats", stats)
    assert F.same_at((got, stats), D.expect(scene)), (stats, D.expect(scene)[1])
    assert stats[0] == len(F.candidates(sorted(scene["src"]), scene["pose"], scene["res"]))


@pytest.mark.parametrize("scene", D.edge_scenes(), ids=lambda s: s["name"])
def test_domain_edge(scene):
    got, stats = run(scene)
    print(scene["name"], "res", scene["res"], "stats", stats)
    want_at, want = D.expect(scene), D.expect_plan(scene)
    assert stats == tuple(int(v) for v in want[1]) and stats[1:] == tuple(int(v) for v in want_at[1]), (stats, want[1], want_at[1])
    if scene.get("count_only"):
        # the statistics of the real call; no byte and no key of DST changes
        assert F.same_at((got, ()), (scene["dst"], ())) and stats[2] + stats[3] > 0
    else:
        assert F.same_at((got, stats), want_at) and F.same((got, stats), want)
    if scene.get("nothing"):
        assert F.same_at((got, ()), (scene["dst"], ())) and stats[1:] == (0, 0, 0, 0, 0)
    for key in scene.get("keys_created", []) if not scene.get("count_only") else []:
        assert key in got and key not in scene["dst"]
