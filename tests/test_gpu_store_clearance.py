"""ws_store_clearance: the clearance over the distance records of the chunk store against clearance_model.py on the dense box of the
chunks (store_distance_scenes.model).  Three chunks with negative keys around a corner; the box spans the five absent ones, whose
records are unknown and show as such.  Raw bytes throughout."""
import ctypes as C

import numpy as np
import pytest

import clearance_model as CM
import distance_model as D
import store_distance_scenes as SDS
from store_distance_scenes import RES, make_store, seam_chunks

pytestmark = pytest.mark.gpu
WS_ERR_INVALID, WS_ERR_RANGE = -1, -5
KEYS = [(-1, -1, -1), (0, -1, -1), (-1, 0, -1)]
R, SOFT, RADIUS = 4, 100, 100
LO, HI = np.array([-12, -10, -14]), np.array([9, 11, 9])
# (T, P, K): seed, steps of the walk in voxels -- picked on the CPU so that the model meets the conditions
SCENES = {(3, 5, 64): (9, 0.4), (70, 67, 3): (8, 0.15)}
assert R * RES >= RADIUS + SOFT


def bytes_equal(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def store_and_records():
    chunks = {k: v for k, v in seam_chunks().items() if k in KEYS}
    assert len(chunks) == 3
    store = make_store(chunks)
    yield store, chunks
    store.close()


@pytest.mark.parametrize("columns", [False, True])
@pytest.mark.parametrize("shape", list(SCENES))
def test_store_matches_the_model(store_and_records, shape, columns):
    store, chunks = store_and_records
    rec, _ = SDS.model(chunks, LO, HI, R, any_weight=True, columns=columns)
    absent = np.zeros(tuple(HI - LO + 1), dtype=bool)
    absent[:, :, 14:] = True       # z >= 0: no chunk there
    absent[12:, 10:, :] = True     # x >= 0 and y >= 0: chunk (0, 0, -1) is absent
    if not columns:
        assert np.all((rec[absent] >> 30) == 0)  # what the store does not have is unknown
    T, P, K = shape
    seed, walk = SCENES[shape]
    rng = np.random.default_rng(seed)
    poses, body = CM.draw_poses(rng, T, P, LO, HI - LO + 1, RES, walk), CM.draw_body(rng, K, RES, RADIUS)
    want, want_pp, best = CM.score(rec, LO, columns, RES, poses, body, SOFT)
    _, _, best_ok = CM.score(rec, LO, columns, RES, poses, body, SOFT, outside_ok=True)
    CM.conditions(want, best, T)
    assert D.same(store.distance(lo=LO, hi=HI, max_dist_vox=R, any_weight=True, columns=columns), rec)
    got = store.clearance(RES, poses, body, SOFT, per_pose=True)
    assert bytes_equal(got.records, want.astype(got.records.dtype)) and bytes_equal(got.poses, want_pp.astype(got.poses.dtype)) and got.best == best
    plain = store.clearance(RES, poses, body, SOFT, outside_ok=True)
    assert plain.poses is None and bytes_equal(plain.records, got.records) and plain.best == best_ok
    # another resolution is another voxel grid over the same records: the model follows
    want2, _, best2 = CM.score(rec, LO, columns, 64, poses, body, SOFT)
    got2 = store.clearance(64, poses, body, SOFT)
    assert bytes_equal(got2.records, want2.astype(got2.records.dtype)) and got2.best == best2


def test_store_refusals_and_the_empty_store(store_and_records):
    import warpsense_amd as W
    store, chunks = store_and_records
    store.distance(lo=LO, hi=HI, max_dist_vox=R, any_weight=True)
    rng = np.random.default_rng(3)
    poses, body = CM.draw_poses(rng, 3, 5, LO, HI - LO + 1, RES, 0.4), CM.draw_body(rng, 2, RES, 40)
    before = store.clearance(RES, poses, body, SOFT)
    L, h = store._L, store.handle
    pp, bp, best = poses.ctypes.data_as(C.c_void_p), body.ctypes.data_as(C.c_void_p), C.c_int64(77)
    call = lambda res=RES, flags=0, soft=SOFT: L.ws_store_clearance(h, pp, 3, 5, bp, 2, soft, res, flags, C.byref(best))
    assert [call(res=0), call(res=-1), call(res=1025), call(flags=8), call(soft=R * RES + 1)] == [WS_ERR_INVALID, WS_ERR_INVALID, WS_ERR_RANGE, WS_ERR_INVALID, WS_ERR_RANGE]
    assert call(res=RES // 2) == WS_ERR_RANGE and best.value == 77  # R res shrinks with the resolution
    n = C.c_size_t(0)
    got = np.zeros(3, dtype=before.records.dtype)
    assert L.ws_store_clearance_download(h, got.ctypes.data_as(C.c_void_p), None, 3, 0, C.byref(n), None) == 0 and n.value == 3 and bytes_equal(got, before.records)
    empty = W.DeviceGlobalMap(SDS.TAU, 0)
    try:
        assert L.ws_store_clearance(empty.handle, pp, 3, 5, bp, 2, SOFT, RES, 0, C.byref(best)) == WS_ERR_INVALID and b"no distance result" in L.ws_last_error()
        assert empty.distance(max_dist_vox=R).size == 0  # no chunk: no records, and every sample is outside
        out = empty.clearance(RES, poses, body, SOFT, per_pose=True)
        assert out.best == -1 and np.all(out.records["outside"] == 10) and np.all(out.records["min_margin"] == CM.NONE) and np.all(out.poses["outside"] == 2)
        assert empty.clearance(RES, poses, body, SOFT, outside_ok=True).best == 0
    finally:
        empty.close()
