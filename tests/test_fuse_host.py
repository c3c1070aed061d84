"""CPU tests of ws_store_fuse's rule: the numpy model (fuse_model.py) under the identity pose against the C oracle's wso_update_avg,
the cell of the model against the model of ws_store_sample, the zero-coefficient rule, fuse_pose, and the declaration of the entry
points.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import fuse_model as F
import query_model as QM
from warpsense_amd import _lib
from warpsense_amd.fuse import FuseStats, fuse_pose, pose_transform

from fuse_scenes import FILL, MW, RES, TAU, identity_case, oracle_route, rot


def test_identity_is_the_oracles_integrate():
    """Under the identity pose q is the voxel's own centre, f = 0 on every axis, so the sample is the src voxel itself and the fuse is
    wso_update_avg voxel by voxel.  The src weights are >= 0 here: the oracle would also copy an entry of negative weight over an
    unobserved one (nw != 0), which the fuse, valid iff weight > 0, does not."""
    dst, src = identity_case()
    out, stats = F.fuse(dst, src, F.identity_pose(), RES, MW, FILL)
    want = oracle_route(dst, src, MW, FILL)
    for key, data in want.items():
        got = out.get(key, np.full(F.CW, FILL, dtype=np.uint32))
        assert got.tobytes() == data.tobytes(), key
    assert sorted(out) == sorted(set(dst) | set(src))  # every src chunk here holds a positive weight
    ev, ew = F.unpack(np.concatenate([dst.get(k, np.full(F.CW, FILL, dtype=np.uint32)) for k in sorted(src)]))
    nv, nw = F.unpack(np.concatenate([src[k] for k in sorted(src)]))
    avg, put = (nw > 0) & (ew > 0), (nw > 0) & (ew <= 0)
    assert [int(v) for v in stats[1:]] == [1, int(avg.sum()), int(put.sum()), int(np.abs(nv - ev)[avg].sum()), int(np.minimum(nw, ew)[avg].sum())]
    assert int(stats[2]) > 100000 and int(stats[3]) > 100000 and np.any((ew + nw)[avg] > MW)


def test_cell_is_the_sample_models():
    """where all eight corners are valid the fuse's nv is d_mm of ws_store_sample's model at the same point, and off the lattice
    (every coefficient positive) nw is its weight"""
    import sample_model as SM
    import store_raycast_scenes as SH
    rng = np.random.default_rng(11)
    chunks = {k: F.pack(rng.integers(-TAU, TAU + 1, F.CW), rng.integers(1, 600, F.CW)) for k in [(0, 0, 0), (0, 0, 1), (-1, 0, 0)]}
    for res in (1, 7, 64, 1024):
        q = np.stack([rng.integers(-66 * res, 66 * res, 4096), rng.integers(-2 * res, 66 * res, 4096), rng.integers(-2 * res, 130 * res, 4096)], axis=1).astype(np.int64)
        q[::3] = (q[::3] // res) * res + res // 2
        valid, nv, nw = F.sample(chunks, res, q)
        rec = SM.model(SH.Chunks({k: v.reshape(64, 64, 64) for k, v in chunks.items()}), res, q, TAU)[0]
        full = rec["cls"] != SM.UNKNOWN
        assert np.count_nonzero(full) > 500 and np.all(valid[full])
        h = res // 2
        on_lattice = np.any((q - h) % res == 0, axis=1)
        off = full & ~on_lattice
        assert np.array_equal(nv[full], rec["d_mm"][full]) and np.array_equal(nw[off], rec["weight"][off]) and (res == 1 or np.count_nonzero(off) > 300)
        assert np.all(nw[full] >= rec["weight"][full])
        # what the zero-coefficient rule adds lies on the lattice only
        assert np.all(on_lattice[valid & ~full])


def test_zero_coefficient_rule():
    """a src voxel whose +x neighbour is invalid is still fused under the identity; it is dropped under a 1 mm shift in x"""
    src = np.full(F.CW, F.pack(TAU, 0), dtype=np.uint32)
    at = lambda x, y, z: x * 4096 + y * 64 + z
    for y in (10, 11):
        for z in (10, 11):
            src[at(10, y, z)] = F.pack(100 + y + z, 5)  # x = 11 stays at weight 0
    out, stats = F.fuse({}, {(0, 0, 0): src}, F.identity_pose(), RES, MW, FILL)
    assert [int(v) for v in stats[1:]] == [1, 0, 4, 0, 0] and out[(0, 0, 0)][at(10, 10, 10)] == F.pack(120, 5)
    shifted = F.identity_pose()
    shifted[12] = 1  # pivot_src x: q = p + (1, 0, 0)
    out, stats = F.fuse({}, {(0, 0, 0): src}, shifted, RES, MW, FILL)
    assert [int(v) for v in stats[1:]] == [0, 0, 0, 0, 0] and out == {}


def test_fuse_pose():
    rng = np.random.default_rng(5)
    for T, pivot in [(rot(17, 3, 0, (13, -7, 4)), None), (rot(-140, 25, 71, (1e6, -2e6, 3e5)), (4000, -9000, 250)), (rot(), None)]:
        pose = fuse_pose(T, pivot)
        assert pose.dtype == np.int32 and pose.shape == (15,) and np.all(np.abs(pose[:9].astype(np.int64)) <= F.Q30)
        # the pull of the inverse pose undoes the pull: within 1 mm over a 2^23 mm cube around the pivot
        back = fuse_pose(np.linalg.inv(pose_transform(pose)), pose[9:12])
        assert np.array_equal(back[12:15], pose[9:12]) and np.array_equal(back[9:12], pose[12:15])
        p = pose[9:12].astype(np.int64) + rng.integers(-2 ** 22, 2 ** 22 + 1, (4096, 3))
        q, inside = F.pull(pose, p)
        p2, inside2 = F.pull(back, q)
        assert inside.all() and inside2.all() and np.abs(p2 - p).max() <= 1
    quarter = fuse_pose(rot(90))
    assert set(np.abs(quarter[:9].astype(np.int64)).tolist()) == {0, F.Q30} and quarter[:9].tolist() == [0, F.Q30, 0, -F.Q30, 0, 0, 0, 0, F.Q30]
    assert fuse_pose(rot(0, 0, 0, (13.4, -7.6, 0.2)))[9:12].tolist() == [13, -8, 0]  # the sub-millimetre remainder is dropped
    for bad in (np.full((4, 4), np.nan), np.eye(3)):
        with pytest.raises(ValueError):
            fuse_pose(bad)
    T = rot()
    T[0, 3] = np.inf
    with pytest.raises(ValueError):
        fuse_pose(T)


@pytest.mark.parametrize("angles,t,pivot,res,key", [((33, -21, 48), (13, -7, 4), (2048, 2048, 2048), RES, (0, 0, 0)),
                                                  ((1, 0.5, -0.7), (63.4, -0.6, 31.5), (0, 0, 0), 1, (-1, 2, 0)),
                                                  ((0, 0, 0), (-RES, 64 * RES - 1, 1), (0, 0, 0), RES, (0, 0, 0))])
def test_candidates_hold_every_receiving_chunk(angles, t, pivot, res, key):
    """the plan is a superset, so the result does not depend on how generous it is: a sparse src chunk creates the same chunks when
    every chunk around is examined -- under a general pose, at res = 1 with a small rotation, and under a translation that puts the
    samples one millimetre from a chunk face"""
    rng = np.random.default_rng(9)
    src = np.full(F.CW, F.pack(TAU, 0), dtype=np.uint32)
    idx = np.stack(np.meshgrid(*(np.array([0, 1, 31, 32, 62, 63]),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)  # 2^3 blocks at corners and centre
    src[idx[:, 0] * 4096 + idx[:, 1] * 64 + idx[:, 2]] = F.pack(rng.integers(-TAU, TAU, len(idx)), 9)
    pose = fuse_pose(rot(*angles, t), pivot)
    out, stats = F.fuse({}, {key: src}, pose, res, MW, FILL)
    cand = F.candidates([key], pose, res)
    assert int(stats[0]) == len(cand) and int(stats[3]) > 0
    lo, hi = np.min(cand, axis=0) - 1, np.max(cand, axis=0) + 1
    receiving = set()
    for k in np.stack(np.meshgrid(*(np.arange(lo[a], hi[a] + 1) for a in range(3)), indexing="ij"), axis=-1).reshape(-1, 3):
        if not F.may_receive(np.asarray([key], dtype=np.int64), pose, k, res):
            continue
        q, inside = F.pull_chunk(pose, k, res)
        if np.any(F.sample({key: src}, res, q)[0] & inside):
            receiving.add(tuple(int(v) for v in k))
    assert receiving == set(out) and receiving <= set(cand)


def test_stats_dataclass():
    s = FuseStats(5, 1, 4, 2, 10, 7)
    assert s.disagreement_mm == 2.5 and s.as_tuple() == (5, 1, 4, 2, 10, 7) and np.isnan(FuseStats(1, 0, 0, 3, 0, 0).disagreement_mm)


def test_symbols_are_declared_bound_and_exported():
    L = _lib.load()
    for name in ("ws_store_fuse", "ws_debug_store_fuse_timing"):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        ret, params = QM._declared(name)
        assert ret == "int" and len(getattr(L, name).argtypes) == len(params), (name, params)
    assert len(QM._declared("ws_store_fuse")[1]) == 7
    header = QM._header()
    assert "#define WS_FUSE_COUNT_ONLY 1u" in header and _lib.WS_FUSE_COUNT_ONLY == 1 and _lib.WS_FUSE_DEFAULT == 0
    assert L.ws_version() == 1
    # refusals that need no device: NULL arguments
    stats = (C.c_uint64 * 6)()
    assert L.ws_store_fuse(None, None, None, 64, 640, 0, stats) == -1
    assert L.ws_last_error().decode().startswith("ws_store_fuse:")
    assert L.ws_debug_store_fuse_timing(None, 0, None) == -1
