"""The numpy model of ws_store_changes (the rule stated in include/warpsense_hip.h): dictionaries of chunks in; the records, the
labels, the cluster table and the six statistics out.  The transform and the sample are those of fuse_model.py (pull, sample,
lookup), the clustering is frontier_model.py's; what is the query's own is the classes, the kinds, the box and the statistics."""
import numpy as np

import frontier_model as FM
import fuse_model as F

RECORD = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("ref_value", "<i2"), ("kind", "<u2")])
assert RECORD.itemsize == 16
OCCUPIED, FREE = 1, 2
APPEARED, VANISHED, CLUSTERS = 1, 2, 4
LOCAL = np.stack(np.meshgrid(*(np.arange(F.CS, dtype=np.int64),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)  # x major, z fastest


def classes(d, band, free_value):
    """OCCUPIED iff |d| < band, FREE iff d >= free_value, else 0"""
    d = np.asarray(d, dtype=np.int64)
    return np.where(np.abs(d) < band, OCCUPIED, np.where(d >= free_value, FREE, 0))


def kinds(ev, ew, valid, nv, nw, band, free_value, min_weight):
    """(kind, known on both sides, known in CUR alone) per voxel"""
    cur = np.asarray(ew) >= min_weight
    ref = np.asarray(valid, dtype=bool) & (np.asarray(nw) >= min_weight)
    both = cur & ref
    ce, cn = classes(ev, band, free_value), classes(nv, band, free_value)
    kind = np.where(both & (ce == OCCUPIED) & (cn == FREE), APPEARED, np.where(both & (ce == FREE) & (cn == OCCUPIED), VANISHED, 0))
    return kind, both, cur & ~ref


def bounding_box(keys):
    k = np.asarray(sorted(keys), dtype=np.int64).reshape(-1, 3)
    return k.min(axis=0) * F.CS, k.max(axis=0) * F.CS + F.CS - 1


def changes(cur, ref, pose, res, band, free_value, min_weight=1, lo=None, hi=None, flags=APPEARED | VANISHED):
    """(records RECORD [n], labels | None, table | None, stats (6,) uint64) of the call"""
    stats = [0] * 6
    parts = []
    if cur and lo is None:
        lo, hi = bounding_box(cur)
    for key in sorted(cur):
        v = LOCAL + np.asarray(key, dtype=np.int64) * F.CS
        inbox = np.all((v >= np.asarray(lo, dtype=np.int64)) & (v <= np.asarray(hi, dtype=np.int64)), axis=1)
        if not inbox.any():
            continue  # the chunk is not listed
        stats[0] += 1
        q, inside = F.pull(pose, v * res + res // 2)
        ev, ew = F.unpack(cur[key])
        look = inbox & inside & (ew >= min_weight)  # the voxels examined that are known in CUR
        valid, nv, nw = np.zeros(F.CW, dtype=bool), np.zeros(F.CW, dtype=np.int64), np.zeros(F.CW, dtype=np.int64)
        valid[look], nv[look], nw[look] = F.sample(ref, res, q[look])
        kind, both, alone = kinds(ev, np.where(look, ew, 0), valid, nv, nw, band, free_value, min_weight)
        stats[1] += int(both.sum())
        stats[2] += int((kind == APPEARED).sum())
        stats[3] += int((kind == VANISHED).sum())
        stats[4] += int(alone.sum())
        stats[5] += int(np.abs(nv - ev)[both].sum())
        m = (kind != 0) & (((flags >> (np.maximum(kind, 1) - 1)) & 1) != 0)
        rec = np.zeros(int(m.sum()), dtype=RECORD)
        rec["x"], rec["y"], rec["z"], rec["ref_value"], rec["kind"] = v[m, 0], v[m, 1], v[m, 2], nv[m], kind[m]
        parts.append(rec)
    rec = np.concatenate(parts) if parts else np.zeros(0, dtype=RECORD)
    rec = rec[np.lexsort((rec["z"], rec["y"], rec["x"]))]  # ascending world (x, y, z), z fastest, across chunk borders
    labels = table = None
    if flags & CLUSTERS:
        labels, table = FM.clusters(rec)
    return rec, labels, table, np.array(stats, dtype=np.uint64)


def direct(cur, ref, band, free_value, min_weight=1):
    """the identity pose without the sample: entry against entry, voxel by voxel, over the chunks of CUR; (records, stats[1:6])"""
    stats, parts = [0] * 5, []
    for key in sorted(cur):
        ev, ew = F.unpack(cur[key])
        nv, nw = F.unpack(ref[key]) if key in ref else (np.zeros(F.CW, dtype=np.int64),) * 2
        a, b = ew >= min_weight, (nw > 0) & (nw >= min_weight) & (key in ref)
        occ_e, free_e, occ_n, free_n = np.abs(ev) < band, ev >= free_value, np.abs(nv) < band, nv >= free_value
        app, van = a & b & occ_e & free_n, a & b & free_e & occ_n
        stats[0] += int((a & b).sum())
        stats[1] += int(app.sum())
        stats[2] += int(van.sum())
        stats[3] += int((a & ~b).sum())
        stats[4] += int(np.abs(nv - ev)[a & b].sum())
        m = app | van
        rec = np.zeros(int(m.sum()), dtype=RECORD)
        v = LOCAL[m] + np.asarray(key, dtype=np.int64) * F.CS
        rec["x"], rec["y"], rec["z"], rec["ref_value"], rec["kind"] = v[:, 0], v[:, 1], v[:, 2], nv[m], np.where(app[m], APPEARED, VANISHED)
        parts.append(rec)
    rec = np.concatenate(parts) if parts else np.zeros(0, dtype=RECORD)
    return rec[np.lexsort((rec["z"], rec["y"], rec["x"]))], stats


def same(got, want):
    """(records, labels, table, stats) of a call against the model's: bytes"""
    ok = np.asarray(got[0]).tobytes() == want[0].tobytes() and [int(v) for v in got[3]] == [int(v) for v in want[3]]
    for g, w in zip(got[1:3], want[1:3]):
        ok = ok and ((g is None) == (w is None)) and (w is None or np.asarray(g).tobytes() == w.tobytes())
    return ok
