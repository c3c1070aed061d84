"""The numpy model of ws_store_fuse (the rule stated in include/warpsense_hip.h): dictionaries of chunks in, the dictionary of DST's
chunks after the call and the six statistics out.  The cell and T are those of sample_model.py (floor((q - h) / res), fractions,
trilinear sum); what is the fuse's own is the pull transform, the zero-coefficient rule, the integrate and the plan of candidates."""
import itertools

import numpy as np

CS, CW = 64, 64 ** 3
REACH = 1 << 24
Q30 = 1 << 30


def unpack(raw):
    raw = np.asarray(raw, dtype=np.uint32)
    return (raw & 0xFFFF).astype(np.uint16).astype(np.int16).astype(np.int64), (raw >> 16).astype(np.uint16).astype(np.int16).astype(np.int64)


def pack(value, weight):
    v = np.asarray(value, dtype=np.int64).astype(np.int16).astype(np.uint16).astype(np.uint32)
    w = np.asarray(weight, dtype=np.int64).astype(np.int16).astype(np.uint16).astype(np.uint32)
    return v | (w << np.uint32(16))


def tdiv(a, b):
    """C's truncating division, b > 0"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return np.where(a >= 0, a // b, -((-a) // b))


def identity_pose(pivot=(0, 0, 0)):
    return np.array([Q30, 0, 0, 0, Q30, 0, 0, 0, Q30, *pivot, *pivot], dtype=np.int32)


def candidates(src_keys, pose, res, grow=2):
    """the candidate chunk keys of DST, ascending: the plan of the library, operation for operation (double precision).  grow: the
    voxels a chunk of SRC is grown by, 2 in the library (test_fuse_domain_host.py looks at plans that are less generous)"""
    pose = np.asarray(pose, dtype=np.int64)
    pd, ps = pose[9:12], pose[12:15]
    h = res // 2
    vlo = np.maximum(-((-(pd - (REACH - 1) - h)) // res), -2 ** 31)
    vhi = np.minimum((pd + (REACH - 1) - h) // res, 2 ** 31 - 1)
    R = pose[:9].astype(np.float64) / 1073741824.0
    out = set()
    for key in src_keys:
        lo, hi = np.full(3, 1e300), np.full(3, -1e300)
        for c in range(8):
            q = np.array([(float(key[k]) * CS + ((CS + grow) if (c >> k) & 1 else -grow)) * float(res) - float(ps[k]) for k in range(3)])
            for k in range(3):
                p = R[k] * q[0] + R[3 + k] * q[1] + R[6 + k] * q[2] + float(pd[k])
                lo[k], hi[k] = min(lo[k], p), max(hi[k], p)
        c0, c1, any_ = [0] * 3, [0] * 3, True
        for k in range(3):
            a, b = max(lo[k] - 2.0, -4e12), min(hi[k] + 2.0, 4e12)
            v0 = max((int(np.floor(a)) - h) // res, int(vlo[k]))
            v1 = min((int(np.ceil(b)) - h) // res + 1, int(vhi[k]))
            any_ = any_ and v0 <= v1
            c0[k], c1[k] = v0 // CS, v1 // CS
        if any_:
            out.update(itertools.product(*(range(c0[k], c1[k] + 1) for k in range(3))))
    return sorted(out)


def lookup(chunks, v):
    """(raw entries, present) of world voxels v (n, 3) int64 in a dictionary of chunks"""
    key = v >> 6
    raw, present = np.zeros(len(v), dtype=np.uint32), np.zeros(len(v), dtype=bool)
    if not len(v):
        return raw, present
    k0 = key.min(axis=0)
    span = key.max(axis=0) - k0 + 1
    code = ((key[:, 0] - k0[0]) * span[1] + (key[:, 1] - k0[1])) * span[2] + (key[:, 2] - k0[2])
    l = v & 63
    idx = l[:, 0] * 4096 + l[:, 1] * 64 + l[:, 2]
    for c in np.unique(code):
        k = (int(c // (span[1] * span[2]) + k0[0]), int(c // span[2] % span[1] + k0[1]), int(c % span[2] + k0[2]))
        data = chunks.get(k)
        if data is None:
            continue
        m = code == c
        raw[m] = np.asarray(data, dtype=np.uint32).reshape(-1)[idx[m]]
        present[m] = True
    return raw, present


def pull(pose, p):
    """q of the points p (n, 3) int64, and which of them lie inside the reach around pivot_dst"""
    pose = np.asarray(pose, dtype=np.int64)
    rot, pd, ps = pose[:9].reshape(3, 3), pose[9:12], pose[12:15]
    d = p - pd
    inside = np.all(np.abs(d) < REACH, axis=1)
    d = np.where(inside[:, None], d, 0)
    q = ((d @ rot.T + (1 << 29)) >> 30) + ps
    return q, inside


def pull_chunk(pose, key, res):
    """pull() for the 64^3 voxel centres of the chunk `key`, x major: the sum taken axis by axis"""
    pose = np.asarray(pose, dtype=np.int64)
    rot, pd, ps = pose[:9].reshape(3, 3), pose[9:12], pose[12:15]
    d = [(int(key[k]) * CS + np.arange(CS, dtype=np.int64)) * res + res // 2 - pd[k] for k in range(3)]
    ok = [np.abs(v) < REACH for v in d]
    inside = (ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]).reshape(-1)
    d = [np.where(o, v, 0) for o, v in zip(ok, d)]
    q = np.stack([((rot[k, 0] * d[0])[:, None, None] + (rot[k, 1] * d[1])[None, :, None] + (rot[k, 2] * d[2])[None, None, :] + (1 << 29) >> 30) + ps[k]
                  for k in range(3)], axis=-1).reshape(-1, 3)
    return q, inside


def may_receive(src_keys, pose, key, res):
    """False only if no voxel of the dst chunk `key` has its base voxel in a chunk of src_keys: q is monotone in every coordinate of
    p, so over the chunk each component lies between its values at the eight corner voxels, and a valid sample needs the chunk of
    its base voxel (the corner that always takes part)"""
    pose = np.asarray(pose, dtype=np.int64)
    v = np.array([[int(key[k]) * CS + (CS - 1 if (c >> k) & 1 else 0) for k in range(3)] for c in range(8)], dtype=np.int64)
    d = v * res + res // 2 - pose[9:12]
    q = ((d @ pose[:9].reshape(3, 3).T + (1 << 29)) >> 30) + pose[12:15]  # (|d| < 2^35 here: the products stay below 2^63)
    b = (q - res // 2) // res
    lo, hi = b.min(axis=0) >> 6, b.max(axis=0) >> 6
    return bool(np.any(np.all((src_keys >= lo) & (src_keys <= hi), axis=1)))


def sample(src, res, q):
    """(valid, nv, nw) of the fuse's sample of `src` at q (n, 3) int64"""
    h = res // 2
    n = len(q)
    valid_all, nv_all, nw_all = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    live = np.flatnonzero(~np.any(np.abs(q) >= 2 ** 30, axis=1))
    # the corner (0, 0, 0) always takes part: only points whose base voxel lies in a present chunk go on
    live = live[lookup(src, (q[live] - h) // res)[1]]
    q = q[live]
    b = (q - h) // res
    f = (q - h) - b * res
    valid = np.ones(len(q), dtype=bool)
    T = np.zeros(len(q), dtype=np.int64)
    wmin = np.full(len(q), 2 ** 31, dtype=np.int64)
    for c in itertools.product((0, 1), repeat=3):
        coef = np.ones(len(q), dtype=np.int64)
        for k in range(3):
            coef = coef * (f[:, k] if c[k] else res - f[:, k])
        part = coef != 0
        raw, present = lookup(src, b + np.array(c, dtype=np.int64))
        value, weight = unpack(raw)
        valid &= ~part | (present & (weight > 0))
        wmin = np.where(part, np.minimum(wmin, weight), wmin)
        T += np.where(part & present, value * coef, 0)
    valid_all[live], nv_all[live], nw_all[live] = valid, T // (res ** 3), wmin
    return valid_all, nv_all, nw_all


def fuse(dst, src, pose, res, max_weight, fill, grow=2):
    """(DST's chunks after the call, stats (6,) uint64)"""
    cand = candidates(sorted(src), pose, res, grow)
    out = {k: np.array(v, dtype=np.uint32).reshape(-1) for k, v in dst.items()}
    stats = [len(cand), 0, 0, 0, 0, 0]
    if not src:
        return out, np.array(stats, dtype=np.uint64)
    src_keys = np.asarray(sorted(src), dtype=np.int64).reshape(-1, 3)
    for key in cand:
        if not may_receive(src_keys, pose, key, res):
            continue
        q, inside = pull_chunk(pose, key, res)
        valid, nv, nw = sample(src, res, q)
        valid &= inside
        if not valid.any():
            continue
        existed = key in out
        cur = out[key] if existed else np.full(CW, fill, dtype=np.uint32)
        ev, ew = unpack(cur)
        avg = valid & (ew > 0)
        put = valid & (ew <= 0)
        v_avg = tdiv(ev * ew + nv * nw, np.where(avg, ew + nw, 1))
        w_avg = np.minimum(max_weight, ew + nw)
        new = np.where(avg, pack(v_avg, w_avg), np.where(put, pack(nv, nw), cur))
        out[key] = new.astype(np.uint32)
        stats[1] += 0 if existed else 1
        stats[2] += int(avg.sum())
        stats[3] += int(put.sum())
        stats[4] += int(np.abs(nv - ev)[avg].sum())
        stats[5] += int(np.minimum(nw, ew)[avg].sum())
    return out, np.array(stats, dtype=np.uint64)


def receiving(src, pose, res, voxels):
    """(v, nv, nw): those of the DST world voxels `voxels` (n, 3) that receive a valid sample, ascending, and their samples.  A world
    voxel is an int32: rows beyond that are no voxels of DST"""
    v = np.unique(np.asarray(voxels, dtype=np.int64).reshape(-1, 3), axis=0)
    v = v[np.all((v >= -2 ** 31) & (v < 2 ** 31), axis=1)]
    if not len(v) or not src:
        return np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    q, inside = pull(pose, v * res + res // 2)
    valid, nv, nw = sample(src, res, q)
    valid &= inside
    return v[valid], nv[valid], nw[valid]


def fuse_at(dst, src, pose, res, max_weight, fill, voxels):
    """(DST's chunks after the call, stats[1:6]) from the rule applied to an explicit list of DST world voxels (n, 3): pull, sample and
    integrate voxel by voxel.  Nothing of the plan takes part: neither candidates() nor may_receive().  It is the call's result iff
    `voxels` holds every voxel that receives a valid sample (receivers() below)."""
    v, nv, nw = receiving(src, pose, res, voxels)
    out = {k: np.array(d, dtype=np.uint32).reshape(-1) for k, d in dst.items()}
    stats = [0, 0, 0, 0, 0]
    if len(v):
        keys, inv = np.unique(v >> 6, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        l = v & 63
        idx = l[:, 0] * 4096 + l[:, 1] * 64 + l[:, 2]
        for i, key in enumerate(keys):
            key = tuple(int(c) for c in key)
            m = inv == i
            if key not in out:
                out[key] = np.full(CW, fill, dtype=np.uint32)
                stats[0] += 1
            ev, ew = unpack(out[key][idx[m]])
            avg = ew > 0
            v_avg = tdiv(ev * ew + nv[m] * nw[m], np.where(avg, ew + nw[m], 1))
            out[key][idx[m]] = np.where(avg, pack(v_avg, np.minimum(max_weight, ew + nw[m])), pack(nv[m], nw[m])).astype(np.uint32)
            stats[1] += int(avg.sum())
            stats[2] += int((~avg).sum())
            stats[3] += int(np.abs(nv[m] - ev)[avg].sum())
            stats[4] += int(np.minimum(nw[m], ew)[avg].sum())
    return out, np.array(stats, dtype=np.uint64)


def receivers(src, pose, res, margin=3):
    """The DST world voxels (n, 3) int64 within +-margin voxels per axis of the image of an observed SRC voxel: for every voxel b of
    SRC with weight > 0 its low corner point c = b res + h is mapped forward, m = rot^T (c - pivot_src) + pivot_dst in double
    precision, and the voxels floor(m / res) + [-margin, margin]^3 are listed.  Voxel by voxel: nothing is shared with the chunk plan.

    Why this holds every voxel that can receive anything, for a rotation: a valid sample needs its base voxel b valid, since the
    corner (0, 0, 0) has the coefficient prod (res - f_k) > 0.  q then lies within [0, res)^3 of c: q = c + f with integer
    0 <= f_k <= res - 1.  q is rot (p - pivot_dst) + pivot_src rounded to the nearest integer per axis, and rot_q30 is the rotation
    rounded to 2^-30 per entry, which over |p - pivot_dst| < 2^24 adds less than 0.05 mm: rot (p - pivot_dst) + pivot_src = c + f + e
    with |e_k| < 0.55.  So p = m + rot^T (f + e), and per axis |p - m| <= |f + e|_2 < sqrt(3) (res - 0.45): p lies within
    res sqrt(3) + 1 mm of the mapped point, under 1.74 voxels per axis.  The voxel of p is v = (p - h) / res, and with
    v0 = floor(m / res):  -1.74 - 0.5 < v - v0 < 1.74 + 1, so |v - v0| <= 2.  The default margin of 3 leaves an outer shell that no
    valid sample may lie on (tests/test_fuse_domain_host.py holds every scene to that)."""
    pose = np.asarray(pose, dtype=np.int64)
    R, pd, ps = pose[:9].reshape(3, 3).astype(np.float64) / float(Q30), pose[9:12].astype(np.float64), pose[12:15].astype(np.float64)
    local = np.stack(np.meshgrid(*(np.arange(CS, dtype=np.int64),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    base = []
    for key in sorted(src):
        b = local[unpack(np.asarray(src[key], dtype=np.uint32).reshape(-1))[1] > 0] + np.asarray(key, dtype=np.int64) * CS
        m = ((b * res + res // 2).astype(np.float64) - ps) @ R + pd  # rot^T (c - pivot_src) + pivot_dst, row by row
        base.append(np.floor(m / res).astype(np.int64))
    if not base or not sum(len(b) for b in base):
        return np.zeros((0, 3), dtype=np.int64)
    base = np.unique(np.concatenate(base), axis=0)
    r = np.arange(-margin, margin + 1, dtype=np.int64)
    shell = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.unique((base[:, None, :] + shell[None, :, :]).reshape(-1, 3), axis=0)


def same_at(got, want):
    """(chunks, stats) of a call against fuse_at's pair: the key set, every chunk's bytes and stats[1:6]"""
    return (sorted(got[0]) == sorted(want[0]) and all(np.asarray(got[0][k], dtype=np.uint32).tobytes() == want[0][k].tobytes() for k in want[0])
            and [int(v) for v in got[1]][-5:] == [int(v) for v in want[1]])


def same(got, want):
    """(chunks, stats) against the model's pair: the key set, every chunk's bytes and the six statistics"""
    return (sorted(got[0]) == sorted(want[0]) and all(np.asarray(got[0][k], dtype=np.uint32).tobytes() == want[0][k].tobytes() for k in want[0])
            and [int(v) for v in got[1]] == [int(v) for v in want[1]])
