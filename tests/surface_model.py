"""The numpy model of ws_map_surface: a line-for-line port of publish_local_map (include/warpsense/visualization/map.h:14-121, the
reference lines are cited in it), its record dtype, the arbitrary-entry maps with every edge of the predicate planted, and the
conditions on those inputs.  It is not part of the oracle."""
import numpy as np

from query_model import ring_box, window


REC = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("raw", "<u4")])
F = np.float32


# ------------------------------------------------------------------------------------------------ the numpy model
def model_box(box, lo, tau, res, band=None):
    """publish_local_map on a dense box of raw entries, box[ix, iy, iz] = values.value(lo + (ix, iy, iz)) (map.h:44).
    Returns (records, marker (n, 7) float32)."""
    band = tau if band is None or band <= 0 else band
    value = (box & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32)  # TSDFEntry::value(), promoted to int for abs()
    weight = (box >> 16).astype(np.uint16).view(np.int16).astype(np.int32)
    keep = (weight > 0) & (np.abs(value) < band)       # map.h:45: if (val.weight() <= 0 || abs(val.value()) >= tau) continue;
    ix, iy, iz = np.nonzero(keep)                      # C order == the collapse(3) schedule(static) concatenation, map.h:35-40, 78-104
    rec = np.empty(len(ix), dtype=REC)
    rec["x"], rec["y"], rec["z"] = lo[0] + ix, lo[1] + iy, lo[2] + iz
    rec["raw"] = box[keep]
    val = value[keep]
    mk = np.empty((len(ix), 7), dtype=F)
    for k, name in enumerate("xyz"):
        mk[:, k] = (rec[name].astype(F) * F(res)) / F(1000.0)  # map.h:51-53: (float)x * (float)map_resolution / 1000.f
    pos = val >= 0
    with np.errstate(invalid="ignore"):
        mk[:, 3] = np.where(pos, val.astype(F) / F(tau), F(0))      # map.h:55-58: color.r = val.value() / (float)tau; color.g = 0
        mk[:, 4] = np.where(pos, F(0), (-val).astype(F) / F(tau))   # map.h:60-63: color.r = 0; color.g = -val.value() / (float)tau
    mk[:, 5] = 0                                                    # map.h:33: color.b = 0
    mk[:, 6] = 1                                                    # map.h:32: color.a = 1
    return rec, mk


def model(host, tau, res, lo=None, hi=None, band=None):
    if lo is None:
        lo, hi = window(host.size_, host.pos_)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    return model_box(ring_box(host.data_, host.size_, host.pos_, host.offset_, lo, hi), lo, tau, res, band)


# ------------------------------------------------------------------------------------------------ arbitrary-entry maps
TAU, RES = 1000, 50
SIZES = [(21, 17, 13), (15, 15, 15), (16, 18, 20), (15, 17, 24), (17, 15, 25), (19, 15, 26), (15, 19, 27)]  # one even; size[2] % 4 = 0, 1, 2, 3
PLANTED = [(w, v) for w in (-1, 0, 1) for v in (TAU - 1, -(TAU - 1), TAU, -TAU, -32768, 0)]


def draw_entries(n, seed, tau=TAU):
    """values uniform in [-2 tau, 2 tau] (P(|v| < tau) = 1999/4001), weights uniform in [-640, 640] (P(w > 0) = 640/1281): a quarter
    qualifies and both branches of the predicate are well populated; then every edge of the predicate planted at fixed places"""
    import warpsense_amd as W
    rng = np.random.default_rng(seed)
    value, weight = rng.integers(-2 * tau, 2 * tau + 1, n), rng.integers(-640, 641, n)
    where = rng.permutation(n)[:len(PLANTED)]
    for i, (w, v) in zip(where, PLANTED):
        value[i], weight[i] = v, w
    return W.pack_entry(value, weight)


def check_inputs(raw, tau=TAU):
    """a condition on the INPUTS: every planted category is there and the qualifying share is 0.25 +- 3 sigma inside [0.10, 0.40]"""
    v = (raw & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32)
    w = (raw >> 16).astype(np.uint16).view(np.int16).astype(np.int32)
    for pw, pv in PLANTED:
        assert np.any((w == pw) & (v == pv)), (pw, pv)
    share = np.count_nonzero((w > 0) & (np.abs(v) < tau)) / raw.size
    assert 0.10 <= share <= 0.40, share


# ------------------------------------------------------------------------------------------------ C++ twin
def skeleton_model(size, pos, res):
    """numpy port of publish_local_map_skeleton's arithmetic (map.h:175-227)"""
    scale = F(res) / F(1000.0)                                                        # (float)map_resolution / 1000.f
    br = [int(np.trunc(F(int(pos[k]) - int(size[k]) // 2) * scale)) for k in range(3)]  # map.h:182-183: int *= float truncates
    tl = [int(np.trunc(F(int(pos[k]) + int(size[k]) // 2) * scale)) for k in range(3)]  # map.h:184-185
    d = [tl[k] - br[k] for k in range(3)]                                              # map.h:188
    pts = []

    def rect(zoff):  # draw_rectangle, map.h:150-173
        bbr = [br[0], br[1], br[2] + zoff]
        btr = [bbr[0] + d[0], bbr[1], bbr[2]]
        btl = [btr[0], btr[1] + d[1], btr[2]]
        bbl = [btl[0] - d[0], btl[1], btl[2]]
        pts.extend([bbr, btr, btr, btl, btl, bbl, bbl, bbr])
    rect(0)
    rect(d[2])
    pts.extend([tl, [tl[0], tl[1], tl[2] - d[2]]])                                    # map.h:195-199
    pts.extend([br, [br[0], br[1], br[2] + d[2]]])                                    # map.h:201-205
    pts.extend([[tl[0] - d[0], tl[1], tl[2]], [tl[0] - d[0], tl[1], tl[2] - d[2]]])   # map.h:207-216
    pts.extend([[br[0] + d[0], br[1], br[2]], [br[0] + d[0], br[1], br[2] + d[2]]])   # map.h:218-227
    return np.array(pts, dtype=np.float64)
