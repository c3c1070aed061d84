"""The chunk scenes (seam, pillars) and the store model of the ws_store_distance tests."""
import distance_model as D
import store_scenes as SM


TAU, RES, MW = D.TAU, D.RES, 640
CS, CW = SM.CS, SM.CW
FLAGS, RANGES = D.FLAGS, D.RANGES
FLAG_BITS = lambda kw: (1 if kw.get("any_weight") else 0) | (2 if kw.get("unknown_occupied") else 0) | (4 if kw.get("columns") else 0)

# ------------------------------------------------------------------------------------------------ the draws
# one draw of distance_model.draw_entries per chunk; tests/test_store_distance_host.py checks each against D.check_inputs
SEAM_SEED, PILLAR_Z_SEED, PILLAR_Y_SEED, WINDOW_SEED = 7100, 7200, 7300, 7400
SEAM_KEYS, ABSENT = SM.SEAM_KEYS, SM.ABSENT
PILLAR_Z = [(0, 0, k) for k in range(-2, 3)]
PILLAR_Y = [(0, k, 0) for k in range(-2, 3)]
HOLE = 2  # the middle chunk of a pillar is absent
SEEDS = ([((CS,) * 3, SEAM_SEED + i) for i in range(8)] + [((CS,) * 3, PILLAR_Z_SEED + i) for i in range(5)]
         + [((CS,) * 3, PILLAR_Y_SEED + i) for i in range(5)] + [((65,) * 3, WINDOW_SEED)])
_CACHE = {}


def drawn(keys, seed, absent=()):
    return {key: D.draw_entries((CS,) * 3, seed + i) for i, key in enumerate(keys) if key not in absent}


def seam_chunks():
    if "seam" not in _CACHE:
        _CACHE["seam"] = drawn(SEAM_KEYS, SEAM_SEED, (ABSENT,))
    return _CACHE["seam"]


def pillar_chunks(keys, seed):
    if seed not in _CACHE:
        _CACHE[seed] = drawn(keys, seed, (keys[HOLE],))
    return _CACHE[seed]


def model(chunks, lo, hi, R, **kw):
    """(records, sites) of the rules on the dense box [lo, hi] of `chunks`; absent chunks are weight-0 entries"""
    return D.model_box(SM.assemble(chunks, lo, hi), R, **kw)


def seam_model(lo, hi, R, **kw):
    key = ("seam", tuple(lo), tuple(hi), R, FLAG_BITS(kw))
    if key not in _CACHE:
        _CACHE[key] = model(seam_chunks(), lo, hi, R, **kw)
    return _CACHE[key]


def make_store(chunks, segment_chunks=2, shift=(0, 0, 0)):
    import warpsense_amd as W
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=segment_chunks)
    for key in sorted(chunks):
        store.put_chunk(tuple(int(k + s) for k, s in zip(key, shift)), chunks[key])
    return store


# ------------------------------------------------------------------------------------------------ 1. seams
CUT_BOXES = SM.CUT_BOXES  # both contain the common corner of the eight chunks, neither is chunk-aligned
