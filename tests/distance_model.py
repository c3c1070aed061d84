"""The numpy model of ws_map_distance (the exact Euclidean transform, rules stated in include/warpsense_hip.h): classes and sites, the
line pass, the brute-force check of it, the drawn entries and the conditions on them."""
import ctypes as C
import itertools

import numpy as np

from query_model import unpack
import query_model as QM
import surface_model as G


TAU, RES, SIZES, PLANTED = G.TAU, G.RES, G.SIZES, G.PLANTED
RANGES = (1, 3, 7, 40, 255)
FLAGS = [dict(any_weight=a, unknown_occupied=u, columns=c) for a, u, c in itertools.product((False, True), repeat=3)]
P_OCCUPIED = 0.002


# ------------------------------------------------------------------------------------------------ the numpy model
def classes(box, any_weight=False):
    """2 occupied (valid and value < 0), 1 free (valid and value >= 0), 0 unknown (not valid)"""
    value, weight = unpack(box)
    valid = weight != 0 if any_weight else weight > 0
    return np.where(valid, np.where(value < 0, 2, 1), 0).astype(np.uint8)


def sites_and_classes(box, any_weight=False, unknown_occupied=False, columns=False):
    cls = classes(box, any_weight)
    if not columns:
        return (cls == 2) | (unknown_occupied & (cls == 0)), cls
    occ, unk, fre = (np.any(cls == k, axis=2) for k in (2, 0, 1))
    site = occ | (unknown_occupied & unk)
    return site, np.where(occ, 2, np.where(site, 0, np.where(fre, 1, 0))).astype(np.uint8)


def line_pass(g, axis, R):
    """g'(i) = min(g(i), min over 1 <= |d| <= R of g(i + d) + d^2) along `axis`; g <= R^2 on entry, so g' is too"""
    g = np.moveaxis(g, axis, 0)
    out = g.copy()
    for d in range(1, min(R, g.shape[0] - 1) + 1):
        np.minimum(out[d:], g[:-d] + d * d, out=out[d:])
        np.minimum(out[:-d], g[d:] + d * d, out=out[:-d])
    return np.moveaxis(out, 0, axis)


def model_box(box, R, any_weight=False, unknown_occupied=False, columns=False):
    """(records shaped like the box, or (nx, ny) for columns; number of sites)"""
    assert 1 <= R <= 255, R
    site, cls = sites_and_classes(box, any_weight, unknown_occupied, columns)
    g = np.where(site, 0, R * R).astype(np.int32)
    for axis in range(g.ndim):
        g = line_pass(g, axis, R)
    return (cls.astype(np.uint32) << np.uint32(30)) | g.astype(np.uint32), int(np.count_nonzero(site))


def model(host, R, lo=None, hi=None, **kw):
    if lo is None:
        lo, hi = QM.window(host.size_, host.pos_)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    return model_box(QM.ring_box(host.data_, host.size_, host.pos_, host.offset_, lo, hi), R, **kw)


def same(got, want):
    return got.dtype == want.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ arbitrary-entry maps
def draw_entries(size, seed, tau=TAU):
    """Uniformly random entries would make half the voxels sites and every d2 tiny.  Here a voxel is occupied with probability
    0.002 (positive weight, value in [-2 tau, -1]); every other voxel has a value in [0, 2 tau] and a weight uniform in
    [-640, 640] -- all three signs, and a negative weight never comes with a negative value, so WS_DISTANCE_ANY_WEIGHT turns
    unknown voxels into free ones and the site share stays.  Then the edge entries of surface_model.PLANTED at fixed places
    (three of them sites by default, three more under ANY_WEIGHT)."""
    import warpsense_amd as W
    rng = np.random.default_rng(seed)
    n = int(np.prod(size))
    occ = rng.random(n) < P_OCCUPIED
    value = np.where(occ, -rng.integers(1, 2 * tau + 1, n), rng.integers(0, 2 * tau + 1, n))
    weight = np.where(occ, rng.integers(1, 641, n), rng.integers(-640, 641, n))
    where = rng.permutation(n)[:len(PLANTED)]
    for i, (w, v) in zip(where, PLANTED):
        value[i], weight[i] = v, w
    return W.pack_entry(value, weight).astype(np.uint32)


def seeds_for(size, which):
    """picked without a GPU so that check_inputs holds for all seven shapes and both maps (tests/test_distance_host.py)"""
    return sum(size) + 1000 * which


def check_inputs(raw, size):
    """The input condition, on the MODEL's output before the device is asked: default flags, R in {3, 7}: at least 3 sites, at
    least 3 % of the records strictly between 0 and R^2 and at least 2 % at R^2; every planted entry is there."""
    value, weight = unpack(raw)
    for pw, pv in PLANTED:
        assert np.any((weight == pw) & (value == pv)), (pw, pv)
    shares = []
    for R in (3, 7):
        rec, n_sites = model_box(raw.reshape(size), R)
        d2 = rec & np.uint32(0xFFFFFF)
        between, clamp = np.count_nonzero((d2 > 0) & (d2 < R * R)) / d2.size, np.count_nonzero(d2 == R * R) / d2.size
        assert n_sites >= 3 and between >= 0.03 and clamp >= 0.02, (size, R, n_sites, between, clamp)
        shares.append((n_sites, between, clamp))
    return shares


CTYPE = dict(QM.CTYPE)
CTYPE.update({"float [4]": C.c_void_p})


def brute(box, R, **kw):
    """the rule as it is written: d2(v) = min(R^2, min over sites s of |v - s|^2), every pair evaluated"""
    site, cls = sites_and_classes(box, **kw)
    v = np.argwhere(np.ones(site.shape, dtype=bool)).astype(np.int64)
    s = np.argwhere(site).astype(np.int64)
    d2 = np.full(len(v), R * R, dtype=np.int64)
    for i in range(0, len(s), 256):
        diff = v[:, None, :] - s[None, i:i + 256, :]
        d2 = np.minimum(d2, np.min(np.sum(diff * diff, axis=2), axis=1))
    return (cls.astype(np.uint32) << np.uint32(30)) | d2.reshape(site.shape).astype(np.uint32), len(s)
