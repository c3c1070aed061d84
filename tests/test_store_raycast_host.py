"""The ray cast of the store without a GPU: the boundary (symbols, header, ctypes signatures), the `Chunks` field that
tests/test_gpu_store_raycast.py hands to the numpy model of the window's ray cast (test_gpu_raycast.model), the chunk lookup of the
kernels against a dict, and the inputs of the GPU tests: for every ray set the model alone yields hits and no-hits.

The ray sets live here, so that the GPU tests and these checks use the same ones; a model result is computed once per process."""
import ctypes as C
import os
import re

import numpy as np

import test_gpu_mesh as M
import test_gpu_raycast as R
import test_gpu_store_mesh as SM
import test_mesh_host as MH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, RES = SM.TAU, SM.RES
STEP = RES // 2
CS = 64
NEW = ["ws_store_raycast", "ws_store_raycast_dev", "ws_store_raycast_records_dev", "ws_store_raycast_gradient_dev", "ws_store_raycast_download",
       "ws_debug_store_raycast_timing"]
CTYPE = dict(MH.CTYPE, **{"ws_store *": C.c_void_p, "const ws_store *": C.c_void_p, "const int32_t *": C.c_void_p, "int32_t *": C.c_void_p})


# ------------------------------------------------------------------------------------------------ the field over chunks
def _code(c, base=0):
    """one ascending int64 per chunk key (|key - base| < 2^20 per axis)"""
    c = np.asarray(c, dtype=np.int64) - base
    assert np.all(np.abs(c) < 2 ** 20)
    return ((c[..., 0] + 2 ** 20) << 42) | ((c[..., 1] + 2 ** 20) << 21) | (c[..., 2] + 2 ** 20)


class Chunks:
    """the field of ws_store_raycast for test_gpu_raycast.model: a dict key -> 262 144 raw entries; a voxel of an absent chunk and a
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
        assert self.far_is_absent or near.all()  # without a base a voxel beyond the packing is a mistake of the fixture
        code = _code(np.where(near[:, None], key, self.base), self.base)
        i = np.minimum(np.searchsorted(self.code, code), max(len(self.code) - 1, 0))
        present = ((self.code[i] == code) & near) if len(self.code) else np.zeros(len(v), dtype=bool)
        l = v & 63
        value, weight = M.unpack(self.data[i, l[:, 0], l[:, 1], l[:, 2]])
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


# ------------------------------------------------------------------------------------------------ the tests
def test_library_exports_and_header_declares_the_store_raycast_entry_points():
    from warpsense_amd import _lib
    L = _lib.load()
    h = MH._header()
    for name in NEW + ["ws_debug_store_raycast_table", "ws_debug_store_raycast_find"]:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    for phrase in ("word for word those of ws_map_raycast", "chunk is NOT VALID, whatever fill_entry is", "Both NULL: everything",
                   "ws_map_raycast on that window returns the\n *     same bytes", "never anything that follows the volume of the box",
                   "apart from\n *     those of ws_store_mesh"):
        assert phrase in h, phrase


def test_ctypes_signatures_agree_with_the_header():
    from warpsense_amd import _lib
    L = _lib.load()
    for name in NEW:
        ret, params = MH._declared(name)
        fn = getattr(L, name)
        assert list(fn.argtypes) == [CTYPE[p] for p in params], (name, params, fn.argtypes)
        if ret.endswith("*"):
            assert fn.restype is C.c_void_p, name
        else:
            assert ret == "int" and fn.restype is C.c_int, name
    assert len(MH._declared("ws_store_raycast")[1]) == 10 and MH._declared("ws_store_raycast")[1] == MH._declared("ws_store_raycast_dev")[1]


def test_chunks_field_agrees_with_the_ring_of_the_assembled_box():
    chunks = SM.seam_chunks()
    rng = np.random.default_rng(5)
    for lo, hi in [SM.bounding_box(chunks), ((-40, -29, -50), (37, 45, 20)), ((-100, -90, -70), (90, 100, 130))]:
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        ring = R.Ring.of_box(SM.assemble(chunks, lo, hi), lo)
        assert np.array_equal(ring.lo, lo) and np.array_equal(ring.hi, hi)
        field = Chunks(chunks, lo, hi)
        v = rng.integers(-140, 141, (6000, 3))
        v[:1500] = rng.integers(-3, 4, (1500, 3))  # around the common corner, the absent chunk among them
        for any_weight in (False, True):
            (va, oka), (vb, okb) = field.entries(v, any_weight), ring.entries(v, any_weight)
            assert np.array_equal(oka, okb) and np.array_equal(va[oka], vb[okb])
            assert 500 < np.count_nonzero(oka) < 5500
        absent = np.all(v >> 6 == np.asarray(SM.ABSENT), axis=1)
        assert absent.sum() > 100 and not field.entries(v, True)[1][absent].any()
    # without a box: everything the chunks hold, nothing else
    free = Chunks(chunks)
    v = rng.integers(-140, 141, (4000, 3))
    inside = np.all((v >= -64) & (v <= 63), axis=1) & ~np.all(v >> 6 == np.asarray(SM.ABSENT), axis=1)
    assert not free.entries(v, True)[1][~inside].any() and free.entries(v, True)[1][inside].any()
    assert not Chunks({}).entries(v, True)[1].any()


def test_chunk_lookup_against_a_dict():
    from warpsense_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(23)
    for n in (0, 1, 2, 3, 7, 1000):
        keys = np.unique(rng.integers(-300, 301, (n, 3)), axis=0).astype(np.int32) if n else np.zeros((0, 3), dtype=np.int32)
        n = len(keys)
        rows = np.concatenate([keys, rng.permutation(n).astype(np.int32).reshape(n, 1)], axis=1).astype(np.int32)
        rows = np.ascontiguousarray(rows)
        places = C.c_size_t(0)
        assert L.ws_debug_store_raycast_table(rows.ctypes.data_as(C.c_void_p), n, None, 0, C.byref(places)) == 0
        size = places.value
        assert size >= max(2, 2 * n) and size & (size - 1) == 0 and size < max(4, 4 * n)  # a power of two >= 2 n, sized by the chunks
        table = np.zeros((size, 4), dtype=np.int32)
        assert L.ws_debug_store_raycast_table(rows.ctypes.data_as(C.c_void_p), n, table.ctypes.data_as(C.c_void_p), size, C.byref(places)) == 0
        assert np.count_nonzero(table[:, 3] != -1) == n
        want_slot = {tuple(int(v) for v in r[:3]): int(r[3]) for r in rows}
        probes = np.concatenate([keys, rng.integers(-310, 311, (500, 3)).astype(np.int32)])
        for key in probes:
            k3 = np.ascontiguousarray(key, dtype=np.int32)
            got = L.ws_debug_store_raycast_find(table.ctypes.data_as(C.c_void_p), size, k3.ctypes.data_as(C.c_void_p))
            assert got == want_slot.get(tuple(int(v) for v in key), 0xffffffff), key


def test_every_ray_set_has_hits_and_no_hits_in_the_model():
    for case in all_cases():
        if case["name"] in ("box one voxel thick", "box in the absent chunk", "box far away"):
            assert hits_of(want(case)[0]) == 0, case["name"]  # no cells: the case is that nothing hits
            continue
        rec, grad = want(case)
        n = hits_of(rec)
        assert 0 < n < len(rec), (case["name"], n, len(rec))
        assert np.any(grad[rec["range_mm"] >= 0] != 0) or case["name"].startswith(("gap", "range", "box two voxels")), case["name"]
    n_seam = [hits_of(want(c)[0]) for c in seam_cases()]
    assert min(n_seam[0], n_seam[1], n_seam[2]) > 100, n_seam


def test_gap_hits_start_at_the_first_sample_behind_the_gap():
    """the +x, +y, +z axis rays of the gap cases hit, and p_{k-1} of the hit is the FIRST sample whose base voxel lies in the far
    chunk, at every phase: a jump that lands one sample late loses the hit"""
    d = gap_dirs()
    n_first = 0
    for j, case in enumerate(gap_cases()):
        rec = want(case)[0]
        for r, key in ((0, (2, 0, 0)), (8, (0, 2, 0)), (16, (0, 0, 2))):  # the axis rays of the three + rows
            k0 = int(first_sample_in(case["origin"], d[r:r + 1], key, case["range"] // STEP)[0])
            assert k0 > 2 * CS and rec["range_mm"][r] >= 0, (j, r)
            assert k0 * STEP <= rec["range_mm"][r] <= (k0 + 1) * STEP, (j, r, k0, rec["range_mm"][r])
            n_first += 1
        assert hits_of(rec[[4, 12, 20, 24, 28]]) >= 4, j  # the - rows and the diagonal hit too
    assert n_first == 3 * 2 * STEP
