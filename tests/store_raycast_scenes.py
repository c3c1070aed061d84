"""The field over chunks (Chunks) and the case generators of the ws_store_raycast tests: seam, gap, box, far and range cases, with the
model's answer to each."""
import ctypes as C

import numpy as np

import query_model as QM
import raycast_model as R
import store_scenes as SM


TAU, RES = SM.TAU, SM.RES
STEP = RES // 2
CS = 64
CTYPE = dict(QM.CTYPE, **{"ws_store *": C.c_void_p, "const ws_store *": C.c_void_p, "const int32_t *": C.c_void_p, "int32_t *": C.c_void_p})


# ------------------------------------------------------------------------------------------------ the field over chunks
def _code(c, base=0):
    """one ascending int64 per chunk key (|key - base| < 2^20 per axis)"""
    c = np.asarray(c, dtype=np.int64) - base
    assert np.all(np.abs(c) < 2 ** 20), (np.abs(c).max(), 2 ** 20)
    return ((c[..., 0] + 2 ** 20) << 42) | ((c[..., 1] + 2 ** 20) << 21) | (c[..., 2] + 2 ** 20)


class Chunks:
    """the field of ws_store_raycast for raycast_model.model: a dict key -> 262 144 raw entries; a voxel of an absent chunk and a
    voxel outside the inclusive box [lo, hi] (None: everything) are not valid.  base: a chunk key near the chunks, for keys beyond the
    2^20 of the packing; every voxel asked for must then lie within 2^20 chunks of it"""

    def __init__(self, chunks, lo=None, hi=None, base=(0, 0, 0)):
        keys = sorted(chunks)
        self.base = np.asarray(base, dtype=np.int64)
        self.far_is_absent = bool(np.any(self.base != 0))
        self.code = _code(np.asarray(keys, dtype=np.int64).reshape(-1, 3), self.base)
        self.data = (np.stack([np.asarray(chunks[k], dtype=np.uint32).reshape(CS, CS, CS) for k in keys]) if keys
                     else np.zeros((1, CS, CS, CS), dtype=np.uint32))
        self.lo = None if lo is None else np.asarray(lo, dtype=np.int64)
        self.hi = None if hi is None else np.asarray(hi, dtype=np.int64)

    def entries(self, v, any_weight):
        v = np.asarray(v, dtype=np.int64)
        key = v >> 6
        near = np.all(np.abs(key - self.base) < 2 ** 20, axis=1)  # (no chunk lies beyond the packing: the key of such a voxel is not looked up)
        assert self.far_is_absent or near.all(), (self.far_is_absent, near)  # without a base a voxel beyond the packing is a mistake of the fixture
        code = _code(np.where(near[:, None], key, self.base), self.base)
        i = np.minimum(np.searchsorted(self.code, code), max(len(self.code) - 1, 0))
        present = ((self.code[i] == code) & near) if len(self.code) else np.zeros(len(v), dtype=bool)
        l = v & 63
        value, weight = QM.unpack(self.data[i, l[:, 0], l[:, 1], l[:, 2]])
        value, weight = value.astype(np.int64), weight.astype(np.int64)
        if self.lo is not None:
            present = present & np.all((v >= self.lo) & (v <= self.hi), axis=1)
        return value, present & ((weight != 0) if any_weight else (weight > 0))


_WANT = {}


def want(case):
    """the model's (records, gradient) of a case, once"""
    if case["name"] not in _WANT:
        _WANT[case["name"]] = R.model(Chunks(case["chunks"](), case.get("lo"), case.get("hi")), RES, case["origin"], case["dirs"], case["range"],
                                      case.get("any_weight", False), case.get("targets", False))
    return _WANT[case["name"]]


def hits_of(rec):
    return int(np.count_nonzero(rec["range_mm"] >= 0))


# ------------------------------------------------------------------------------------------------ 1. the seam chunks
def seam_cases():
    """2048 random rays from inside, the sphere rays from outside the sphere, rays from outside every chunk, rays that graze the
    chunk edges and the common corner; under both weight rules, once as targets"""
    rng = np.random.default_rng(7)
    o_in = np.array([15, -20, 35], dtype=np.int64)
    d_in = rng.integers(-32768, 32769, (2048, 3))
    c_mm = (np.asarray(SM.SPHERE[0]) - CS) * RES
    o_out = np.array([-3100, -2900, -3000], dtype=np.int64)
    d_sph = np.round(c_mm + np.random.default_rng(1).normal(size=(1024, 3)) * SM.SPHERE[1] * RES * 0.9 - o_out).astype(np.int64)
    o_far = np.array([-5021, 310, 207], dtype=np.int64)  # outside every chunk: the rays come in through the face x = -64
    d_far = np.concatenate([np.abs(rng.integers(-32768, 32769, (512, 1))) + 20000, rng.integers(-24000, 24001, (512, 2))], axis=1)
    # along the edges where the chunks meet (the cell straddles two, four chunks, the absent one among them) and through the corner
    o_graze = np.array([-1010, 12, 12], dtype=np.int64)
    d_graze = np.array([[1, 0, 0], [4096, 1, 0], [4096, 0, -1], [4096, 3, 2], [1010, -12, -12], [1010, 13, -37], [1010, -12, 38], [-1, 0, 0], [0, 0, 0], [-4096, -4000, 100]], dtype=np.int64) * 200
    out = []
    for any_weight in (False, True):
        tag = "any" if any_weight else "pos"
        out.append(dict(name=f"seam in {tag}", chunks=SM.seam_chunks, origin=o_in, dirs=d_in, range=4000, any_weight=any_weight))
        out.append(dict(name=f"seam sphere {tag}", chunks=SM.seam_chunks, origin=o_out, dirs=d_sph, range=6000, any_weight=any_weight))
        out.append(dict(name=f"seam far {tag}", chunks=SM.seam_chunks, origin=o_far, dirs=d_far, range=6000, any_weight=any_weight))
        out.append(dict(name=f"seam graze {tag}", chunks=SM.seam_chunks, origin=o_graze, dirs=d_graze, range=3000, any_weight=any_weight))
    out.append(dict(name="seam targets", chunks=SM.seam_chunks, origin=o_out, dirs=d_sph + o_out, range=6000, targets=True))
    return out


# ------------------------------------------------------------------------------------------------ 2. nothing in the way
GAP_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]


def _gap_chunks():
    """The chunk (0,0,0), and at two chunks' distance along +-x, +-y, +-z and +-(1,1,1) a chunk each; every chunk between is absent:
    eight rows of three chunks with the middle one dropped, rays in both directions from the one in the middle.  All weights 64.  The
    middle chunk is inside (-300) everywhere.  An outer chunk is outside (+300) in the one layer of voxels that faces the gap and
    inside (-300) behind it: the surface lies in the first cell behind the gap."""
    l = np.arange(CS)
    out = {(0, 0, 0): np.full((CS,) * 3, -300)}
    for d in GAP_DIRS:
        for s in (1, -1):
            first = np.zeros((CS,) * 3, dtype=bool)
            for k in range(3):
                if d[k]:
                    layer = (l == (0 if s > 0 else CS - 1)).reshape([CS if j == k else 1 for j in range(3)])
                    first = first | layer
            out[tuple(2 * s * c for c in d)] = np.where(first, 300, -300)
    import warpsense_amd as W
    return {k: W.pack_entry(v.reshape(-1), np.full(v.size, 64)).astype(np.uint32) for k, v in out.items()}


_GAP = {}


def gap_chunks():
    if "c" not in _GAP:
        _GAP["c"] = _gap_chunks()
    return _GAP["c"]


GAP_ORIGIN = np.array([1613, 1627, 1609], dtype=np.int64)  # in the middle chunk; + (j, j, j) mm, j = 0 .. 2 STEP - 1: every phase on every axis


def gap_dirs():
    """per row and direction: the axis itself, two slightly oblique rays, and one so oblique that it misses the far chunk's first layer
    or the far chunk"""
    out = []
    for d in GAP_DIRS:
        a = np.asarray(d, dtype=np.int64)
        e1, e2 = np.roll(a, 1) * (1 if sum(d) == 1 else 0), np.roll(a, 2) * (1 if sum(d) == 1 else 0)
        if sum(d) == 3:
            e1, e2 = np.array([1, -1, 0]), np.array([0, 1, -1])
        for s in (1, -1):
            out += [s * a * 4096, s * a * 4096 + 37 * e1 - 21 * e2, s * a * 4096 - 11 * e1 + 5 * e2, s * a * 4096 + 1900 * e1 + 600 * e2]
    return np.asarray(out, dtype=np.int64) * 16


def gap_cases():
    d = gap_dirs()
    return [dict(name=f"gap {j}", chunks=gap_chunks, origin=GAP_ORIGIN + j, dirs=d, range=8600) for j in range(2 * STEP)]


def first_sample_in(origin, d, key, n_samples):
    """per ray the first sample index whose base voxel lies in chunk `key`, -1 if none: the walk of the rules, nothing shortened"""
    d = np.asarray(d, dtype=np.int64)
    L = np.array([int(np.floor(np.sqrt(float(np.sum(v.astype(object) ** 2))))) for v in d], dtype=np.int64)
    out = np.full(len(d), -1, dtype=np.int64)
    for k in range(n_samples + 1):
        p = origin + R.tdiv(d * (k * STEP), L[:, None])
        inside = np.all(((p - RES // 2) // RES) >> 6 == np.asarray(key), axis=1)
        out[(out < 0) & inside] = k
    return out


# ------------------------------------------------------------------------------------------------ 4. boxes, 5. far-apart chunks
BOXES = {
    "starts in a negative chunk": ((-50, -64, -64), (63, 63, 63)),
    "ends mid-chunk": ((-64, -64, -64), (30, 17, 41)),
    "exceeds the chunks on all sides": ((-100, -90, -70), (90, 100, 130)),
    "one voxel thick": ((-64, -64, 0), (63, 63, 0)),
    "two voxels thick": ((-64, -64, -1), (63, 63, 0)),
    "in the absent chunk": ((1, 1, -60), (60, 60, -2)),
    "far away": ((1000, 1000, 1000), (1100, 1100, 1100)),
    "the bounding box": ((-64,) * 3, (63,) * 3),
}


def box_cases():
    base = seam_cases()[0]  # the 2048 random rays from inside
    return [dict(base, name="box " + name, dirs=base["dirs"][:768], lo=lo, hi=hi) for name, (lo, hi) in BOXES.items()]


def far_cases():
    """short rays inside each of the three far-apart chunks"""
    rng = np.random.default_rng(19)
    out = []
    for i, key in enumerate(SM.FAR_KEYS):
        o = (np.asarray(key, dtype=np.int64) * CS + 5) * RES + np.array([3, -7, 11])  # in a corner of the chunk, the rays run into it
        out.append(dict(name=f"far {i}", chunks=SM.far_chunks, origin=o, dirs=np.abs(rng.integers(-32768, 32769, (512, 3))), range=2500, any_weight=bool(i & 1)))
    return out


RANGE_KEYS = [(0, 0, 0), (13, 0, 0)]  # 12 absent chunks between two present ones


def range_chunks():
    if "r" not in _GAP:
        _GAP["r"] = {RANGE_KEYS[0]: gap_chunks()[(0, 0, 0)], RANGE_KEYS[1]: gap_chunks()[(2, 0, 0)]}
    return _GAP["r"]


def range_case():
    o = np.array([3100, 1600, 1611], dtype=np.int64)
    d = np.array([[4096, 0, 0], [4096, 3, -2], [4096, 5, 1], [-4096, 0, 0], [0, 4096, 0]], dtype=np.int64) * 16
    return dict(name="range", chunks=range_chunks, origin=o, dirs=d, range=(13 * CS + 4) * RES - 3100)


def all_cases():
    return seam_cases() + gap_cases() + box_cases() + far_cases() + [range_case()]


def raw_cast(store, origin, d, n, rng, res=RES, flags=0, lo=None, hi=None):
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    o = np.ascontiguousarray(origin, dtype=np.int32)
    hits = C.c_size_t(77)
    return store._L.ws_store_raycast(store.handle, p(a), p(b), p(o), p(d), n, rng, res, flags, C.byref(hits)), hits.value
