"""The chunk-store scenes of the ws_store_* query tests, first built for ws_store_mesh: the seam and far chunks, the assembly of chunks
into one box and the model on it, a store made of chunks, and the three-position walk.  TAU, RES, CS and the rest are this
module's own; the scenes of the other store queries keep theirs in their own modules."""
import ctypes as C

import numpy as np

import mesh_model as M
import query_model as QM


TAU, RES, MW = M.TAU, M.RES, 640
CS, CW = 64, 64 ** 3


# ------------------------------------------------------------------------------------------------ the model on chunks
def bounding_box(keys):
    k = np.asarray(sorted(keys), dtype=np.int64).reshape(-1, 3)
    return k.min(axis=0) * CS, k.max(axis=0) * CS + CS - 1


def assemble(chunks, lo, hi):
    """the dense box [lo, hi] (inclusive world voxels) of raw entries: box[x - lo] = the voxel of its chunk (index lx * 4096 + ly * 64
    + lz, key = floor(voxel / 64)), raw 0 where `chunks` (key -> 262 144 uint32) has no such chunk"""
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    box = np.zeros(tuple(int(v) for v in hi - lo + 1), dtype=np.uint32)
    for key, data in chunks.items():
        base = np.asarray(key, dtype=np.int64) * CS
        a, b = np.maximum(lo, base), np.minimum(hi, base + CS - 1)
        if np.any(a > b):
            continue
        src = np.asarray(data, dtype=np.uint32).reshape(CS, CS, CS)
        box[tuple(slice(int(a[k] - lo[k]), int(b[k] - lo[k]) + 1) for k in range(3))] = \
            src[tuple(slice(int(a[k] - base[k]), int(b[k] - base[k]) + 1) for k in range(3))]
    return box


def model_store(chunks, res, lo=None, hi=None, any_weight=False):
    if lo is None:
        if not chunks:
            return np.empty(0, dtype=M.VERT), np.empty((0, 3), dtype=np.uint32)
        lo, hi = bounding_box(chunks)
    return M.model_box(assemble(chunks, lo, hi), np.asarray(lo, dtype=np.int64), res, any_weight)


def word_index(keys):
    """The world-order formula of store_mesh.hip: for the chunk list `keys` (n x 3) the index of every word, shape (n, 64, 64) over
    (chunk, lx, ly): 4096 B[cx] + lx 64 N[cx] + 64 P[cx, cy] + ly n[cx, cy] + r"""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    n_chunks = len(keys)
    B, N, P, n, r = (np.zeros(n_chunks, dtype=np.int64) for _ in range(5))
    for i, (cx, cy, cz) in enumerate(keys):
        same_x, same_xy = keys[:, 0] == cx, (keys[:, 0] == cx) & (keys[:, 1] == cy)
        B[i], N[i] = np.count_nonzero(keys[:, 0] < cx), np.count_nonzero(same_x)
        P[i], n[i] = np.count_nonzero(same_x & (keys[:, 1] < cy)), np.count_nonzero(same_xy)
        r[i] = np.count_nonzero(same_xy & (keys[:, 2] < cz))
    lx, ly = np.arange(CS, dtype=np.int64)[None, :, None], np.arange(CS, dtype=np.int64)[None, None, :]
    return 4096 * B[:, None, None] + lx * 64 * N[:, None, None] + 64 * P[:, None, None] + ly * n[:, None, None] + r[:, None, None]


# ------------------------------------------------------------------------------------------------ the seam store
ABSENT = (0, 0, -1)
SEAM_KEYS = [(cx, cy, cz) for cx in (-1, 0) for cy in (-1, 0) for cz in (-1, 0)]
SPHERE = ((64.3, 63.6, 64.6), 40.2)  # centre in box coordinates (world + 64), radius in voxels: around the common corner


def split(world):
    """a 128^3 array over the world voxels [-64, 63]^3 as the eight chunks (-1..0)^3"""
    return {k: np.ascontiguousarray(world[tuple(slice(CS * (c + 1), CS * (c + 2)) for c in k)]).reshape(-1) for k in SEAM_KEYS}


_SEAM = {}


def seam_world():
    """the sphere where its value is inside the truncation band, random entries in the slabs within 3 voxels of every chunk face,
    weight 0 elsewhere; the planted pairs of test_gpu_mesh across the z seam"""
    if "world" not in _SEAM:
        import warpsense_amd as W
        sphere = M.sphere_box(2 * CS, *SPHERE).reshape((2 * CS,) * 3)
        value, weight = QM.unpack(sphere)
        weight = np.where(np.abs(value) < TAU, weight, 0)
        rv, rw = QM.unpack(M.draw_entries((2 * CS,) * 3, seed=128).reshape((2 * CS,) * 3))
        near = np.isin(np.arange(2 * CS) % CS, (0, 1, 2, 61, 62, 63))
        slab = near[:, None, None] | near[None, :, None] | near[None, None, :]
        value, weight = np.where(slab, rv, value), np.where(slab, rw, weight)
        z = CS - 1  # world z = -1 and 0: the pair straddles the z seam, in the chunks (-1, -1, -1) and (-1, -1, 0)
        for p, ((va, wa), (vb, wb)) in enumerate(M.PLANT_PAIRS):
            x, y = CS - 10 - 3 * p, CS - 12 - 2 * p
            weight[x:x + 2, y:y + 2, z - 1:z + 3] = np.maximum(np.abs(weight[x:x + 2, y:y + 2, z - 1:z + 3]), 1)
            value[x, y, z], weight[x, y, z] = va, wa
            value[x, y, z + 1], weight[x, y, z + 1] = vb, wb
        _SEAM["world"] = W.pack_entry(value.reshape(-1), weight.reshape(-1)).astype(np.uint32).reshape((2 * CS,) * 3)
        _SEAM["sphere"] = sphere
    return _SEAM["world"]


def seam_chunks():
    if "chunks" not in _SEAM:
        chunks = split(seam_world())
        del chunks[ABSENT]
        _SEAM["chunks"] = chunks
    return _SEAM["chunks"]


def seam_model(any_weight=False, lo=None, hi=None):
    """the model's mesh of the seam store, computed once per case"""
    key = ("model", any_weight, None if lo is None else (tuple(lo), tuple(hi)))
    if key not in _SEAM:
        _SEAM[key] = model_store(seam_chunks(), RES, lo, hi, any_weight)
    return _SEAM[key]


def check_seam_inputs():
    """conditions on the INPUTS: the planted pairs straddle the z seam, and the model's mesh is not small under either rule"""
    value, weight = QM.unpack(seam_world())
    for p, ((va, wa), (vb, wb)) in enumerate(M.PLANT_PAIRS):
        x, y = CS - 10 - 3 * p, CS - 12 - 2 * p
        assert (value[x, y, CS - 1], weight[x, y, CS - 1], value[x, y, CS], weight[x, y, CS]) == (va, wa, vb, wb), ((value[x, y, CS - 1], weight[x, y, CS - 1], value[x, y, CS], weight[x, y, CS]), (va, wa, vb, wb))
    for any_weight in (False, True):
        vert, face = seam_model(any_weight)
        assert len(vert) > 100 and len(face) > 100, (any_weight, len(vert), len(face))


def make_store(chunks, segment_chunks=2):
    import warpsense_amd as W
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=segment_chunks)
    for key in sorted(chunks):
        store.put_chunk(key, chunks[key])
    return store


def raw_mesh(store, lo, hi, res, flags=0):
    nv, nf = C.c_size_t(7), C.c_size_t(7)
    p = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.int32).ctypes.data_as(C.c_void_p)
    a, b = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (lo, hi))
    rc = store._L.ws_store_mesh(store.handle, p(a), p(b), res, flags, C.byref(nv), C.byref(nf))
    return rc, nv.value, nf.value


# ------------------------------------------------------------------------------------------------ 2. the window's bytes
CUT_BOXES = [((-40, -29, -50), (37, 45, 20)), ((-64, -3, -7), (63, 2, 9))]


# ------------------------------------------------------------------------------------------------ 4. far-apart chunks
FAR_KEYS = [(-200, 150, -20), (0, 0, 0), (200, -150, 20)]


def far_chunks():
    out = {}
    for i, key in enumerate(FAR_KEYS):
        if i == 1:
            out[key] = M.sphere_box(CS, (31.4, 32.2, 30.7), 21.3).reshape(-1)
        else:
            out[key] = M.draw_entries((CS,) * 3, seed=400 + i)
    return out


# ------------------------------------------------------------------------------------------------ 8. after real use
WALK = [(0, 0, 0), (40, 0, 0), (80, 0, 0)]  # window positions (voxels); the sensor stands in the middle of the window
ROOM = (4500.0, 1300.0, 900.0)


def walk_scan(k):
    from warpsense_amd import synthetic as S
    return S.os1_128_scan(sensor_mm=tuple(float(c * RES) for c in WALK[k]), rings=32, azimuths=256, half_extents_mm=ROOM, seed=20 + k)


def crossing_faces(vert, face, res):
    """faces with vertices in two different chunks: vertices strictly on both sides of a chunk border plane"""
    n = 0
    S = CS * res
    for name in ("x_mm", "y_mm", "z_mm"):
        q = vert[name][face.astype(np.int64)].astype(np.int64) - res // 2  # a vertex of cell c lies in [c res, (c + 1) res]
        n += int(np.count_nonzero(np.floor_divide(q.max(axis=1) - 1, S) > np.floor_divide(q.min(axis=1), S)))
    return n
