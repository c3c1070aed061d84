"""The chunk scenes and the store model of the ws_store_surface tests."""
import numpy as np

import query_model as QM
import store_scenes as SM
import surface_model as G


TAU, RES, MW = G.TAU, G.RES, 640
CS, CW = SM.CS, SM.CW
BAND = TAU // 3


# ------------------------------------------------------------------------------------------------ the model on chunks
def model_store(chunks, tau, res, lo=None, hi=None, band=None):
    if lo is None:
        if not chunks:
            return np.empty(0, dtype=G.REC), np.empty((0, 7), dtype=G.F)
        lo, hi = SM.bounding_box(chunks)
    lo = np.asarray(lo, dtype=np.int64)
    return G.model_box(SM.assemble(chunks, lo, hi), lo, tau, res, band)


# ------------------------------------------------------------------------------------------------ the seam store
_SEAM = {}


def seam_chunks():
    """the seven chunks of test_gpu_store_mesh's seam store -- (-1..0)^3 without (0, 0, -1) -- filled with surface_model.draw_entries:
    weights <= 0, |value| >= band and -32768 all occur, in every chunk"""
    if "chunks" not in _SEAM:
        _SEAM["chunks"] = {k: G.draw_entries(CW, seed=640 + i).astype(np.uint32) for i, k in enumerate(SM.SEAM_KEYS) if k != SM.ABSENT}
    return _SEAM["chunks"]


def seam_model(lo=None, hi=None, band=None):
    """the model's cloud of the seam store, computed once per case"""
    key = (None if lo is None else (tuple(lo), tuple(hi)), band)
    if key not in _SEAM:
        _SEAM[key] = model_store(seam_chunks(), TAU, RES, lo, hi, band)
    return _SEAM[key]


def check_seam_inputs():
    """conditions on the INPUTS: the model's cloud is not small, every present chunk has a record on each of its six faces, and both
    branches of the predicate decide somewhere alone"""
    for data in seam_chunks().values():
        G.check_inputs(data)
    rec, _ = seam_model()
    assert len(rec) > 1000, len(rec)
    for key in seam_chunks():
        mine = np.all([rec[n] // CS == key[k] for k, n in enumerate("xyz")], axis=0)
        for n in "xyz":
            local = rec[n][mine] % CS
            assert np.any(local == 0) and np.any(local == CS - 1), (key, n)
    raw = np.concatenate(list(seam_chunks().values()))
    v = (raw & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32)
    w = (raw >> 16).astype(np.uint16).view(np.int16).astype(np.int32)
    for band in (TAU, BAND):
        assert np.any((w <= 0) & (np.abs(v) < band)) and np.any((w > 0) & (np.abs(v) >= band)), band


def same2(got, want):
    return QM.same(got[0], want[0]) and QM.same(got[1], want[1])


# ------------------------------------------------------------------------------------------------ 4. far-apart chunks
FAR_KEYS = [(-15700, 15650, -20), (0, 0, 0), (15700, -15650, 20)]  # a million voxels apart


def far_chunks():
    return {key: G.draw_entries(CW, seed=500 + i).astype(np.uint32) for i, key in enumerate(FAR_KEYS)}


def check_far_inputs():
    """a condition on the INPUTS: neighbours a million voxels apart along x and y, and no dense pass over their bounding box can run"""
    lo, hi = SM.bounding_box(far_chunks())
    assert int((hi - lo)[:2].min()) > 2_000_000 and float(np.prod((hi - lo + 1).astype(np.float64))) > 1e15, (lo, hi)
    assert all(-2 ** 31 <= int(c) < 2 ** 31 for c in list(lo) + list(hi)), (lo, hi)
    return lo, hi
