"""The numpy model of ws_map_view_gain / ws_store_view_gain (the rules stated in include/warpsense_hip.h), on a dense box of raw entries
in world order: for every (view, ray) the whole walk k = 0 .. K, nothing shortened.  The per-ray arrays it returns hold everything a
view's record is summed from, so the records of a prefix of the views and of the fan come from one run."""
import math

import numpy as np

import query_model as QM
from raycast_model import tdiv

RECORD = np.dtype([("unknown_k2", "<u8"), ("free_k2", "<u8"), ("unknown", "<u4"), ("free", "<u4"), ("blocked", "<u4"), ("live", "<u4")])
RAY = np.dtype([("unknown", "<u4"), ("stop", "<i4")])
DEAD, OPEN = -2, -1


def march(box, box_lo, res, origins, dirs, max_range, min_value=0, any_weight=False):
    """box[ix, iy, iz]: the raw entry of world voxel box_lo + (ix, iy, iz); the box IS the query box, a voxel outside it counts for
    nothing.  Returns a dict of (m, n) int64 arrays: unknown, unknown_k2, free, free_k2, stop, and outside (samples skipped as
    outside the box before the ray was blocked)."""
    box = np.asarray(box, dtype=np.uint32)
    lo = np.asarray(box_lo, dtype=np.int64).reshape(3)
    shape = np.asarray(box.shape, dtype=np.int64)
    value, weight = QM.unpack(box)
    valid = (weight != 0) if any_weight else (weight > 0)
    cls = np.where(valid, np.where(value >= min_value, 2, 3), 1).astype(np.int8).reshape(-1)  # 1 UNKNOWN 2 FREE 3 OCCUPIED
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 1, 3)
    d = np.asarray(dirs, dtype=np.int64).reshape(1, -1, 3)
    m, n = o.shape[0], d.shape[1]
    L = np.array([math.isqrt(int(x) ** 2 + int(y) ** 2 + int(z) ** 2) for x, y, z in d[0]], dtype=np.int64).reshape(1, n)
    live = (L > 0) & np.all(np.abs(d) < 2 ** 30, axis=2)
    d = np.where(live[..., None], d, 0)
    Ls = np.where(live, L, 1)[..., None]
    step = max(res // 2, 1)
    K = max_range // step
    out = {name: np.zeros((m, n), dtype=np.int64) for name in ("unknown", "unknown_k2", "free", "free_k2", "outside")}
    stop = np.where(np.broadcast_to(live, (m, n)), OPEN, DEAD).astype(np.int64)
    walking = stop == OPEN
    for k in range(K + 1):
        v = (o + tdiv(d * (k * step), Ls)) // res - lo
        inside = walking & np.all((v >= 0) & (v < shape), axis=2)
        c = np.zeros((m, n), dtype=np.int8)
        vi = v[inside]
        c[inside] = cls[(vi[:, 0] * shape[1] + vi[:, 1]) * shape[2] + vi[:, 2]]
        hit = c == 3
        stop[hit] = k
        walking &= ~hit
        out["outside"] += walking & ~inside
        out["unknown"] += c == 1
        out["unknown_k2"] += (c == 1) * (k * k)
        out["free"] += c == 2
        out["free_k2"] += (c == 2) * (k * k)
    out["stop"] = stop
    return out


def records(w, m=None, n=None):
    """(view records, ray records) of the first m views and the first n rays of a march"""
    sl = (slice(0, m), slice(0, n))
    rec = np.zeros(w["stop"][sl].shape[0], dtype=RECORD)
    for name in ("unknown_k2", "free_k2", "unknown", "free"):
        rec[name] = w[name][sl].sum(axis=1)
    rec["blocked"] = (w["stop"][sl] >= 0).sum(axis=1)
    rec["live"] = (w["stop"][sl] != DEAD).sum(axis=1)
    rays = np.zeros(w["stop"][sl].shape, dtype=RAY)
    rays["unknown"], rays["stop"] = w["unknown"][sl], w["stop"][sl]
    return rec, rays


def model(box, box_lo, res, origins, dirs, max_range, min_value=0, any_weight=False):
    return records(march(box, box_lo, res, origins, dirs, max_range, min_value, any_weight))


def from_rays(rays):
    """what a view's record can be recomputed from its rays' records: unknown, blocked, live"""
    return rays["unknown"].astype(np.int64).sum(axis=1), (rays["stop"] >= 0).sum(axis=1), (rays["stop"] != DEAD).sum(axis=1)
