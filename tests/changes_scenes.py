"""The scenes of the ws_store_changes tests: chunks of random entries on and around every class edge, the maps of the pose cases,
and the sphere-and-floor map of fuse_scenes.py with a box added and a pillar removed."""
import numpy as np

import fuse_model as F
import fuse_scenes as S
from fuse_scenes import RES, TAU

BAND, FREE = RES, TAU
EDGES = np.array([-32768, -TAU, -BAND, -BAND + 1, -1, 0, BAND - 1, BAND, FREE - 1, FREE, 32767])


def draw(seed, weights=(0, 1, 2, 3, 40), unobserved=0.0):
    """a chunk whose values sit on and around every class edge, with weights around min_weight"""
    rng = np.random.default_rng(seed)
    value = np.where(rng.random(F.CW) < 0.5, rng.choice(EDGES, F.CW), rng.integers(-TAU, TAU + 1, F.CW))
    weight = rng.choice(np.array(weights), F.CW)
    return F.pack(value, np.where(rng.random(F.CW) < unobserved, 0, weight))


def pose_maps():
    cur = {(0, 0, 0): draw(21, unobserved=0.2), (0, 1, 0): draw(22), (-1, 0, 0): draw(23)}
    ref = {(0, 0, 0): draw(24, weights=(2, 3, 40), unobserved=0.01), (0, 1, 0): draw(25, weights=(1, 2, 3, 40)), (-1, 0, -1): draw(26, weights=(2, 40))}
    return cur, ref


_SCENE = {}


def scene():
    """the sphere-and-floor map with its free space observed; REF holds a pillar that CUR lacks, CUR a box that REF lacks"""
    if not _SCENE:
        base = {}
        for key, data in S.sphere_and_floor().items():
            value, weight = F.unpack(data)
            base[key] = F.pack(value, np.where(value >= TAU, 20, weight)).reshape(64, 64, 64)

        def put(chunks, lo, hi):
            out = {k: v.copy() for k, v in chunks.items()}
            for x in range(lo[0], hi[0] + 1):
                for y in range(lo[1], hi[1] + 1):
                    for z in range(lo[2], hi[2] + 1):
                        out[(x >> 6, y >> 6, z >> 6)][x & 63, y & 63, z & 63] = F.pack(0, 20)
            return {k: v.reshape(-1) for k, v in out.items()}
        box, pillar = ((40, 40, -20), (47, 47, -13)), ((-50, -50, -30), (-48, -48, 10))
        _SCENE.update(cur=put(base, *box), ref=put(base, *pillar), box=box, pillar=pillar)
    return _SCENE
