"""The numpy model of ws_map_mesh (the surface-nets rules stated in include/warpsense_hip.h), its vertex dtype, the sphere maps, the
planted entry pairs and the conditions on those inputs."""
import numpy as np

from query_model import unpack
import query_model as QM
import surface_model as G


VERT = np.dtype([("x_mm", "<i4"), ("y_mm", "<i4"), ("z_mm", "<i4"), ("weight", "<u4")])
TAU, RES = G.TAU, G.RES
SIZES = G.SIZES


# ------------------------------------------------------------------------------------------------ the numpy model
def cell_masks(box, any_weight=False):
    """(valid cells, active cells, inside voxels) of a dense box of raw entries; cells have shape box.shape - 1"""
    value, weight = unpack(box)
    valid = (weight != 0) if any_weight else (weight > 0)
    inside = value < 0
    ex, ey, ez = box.shape
    cv = np.ones((ex - 1, ey - 1, ez - 1), dtype=bool)
    n_in = np.zeros(cv.shape, dtype=np.uint8)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                sl = (slice(dx, ex - 1 + dx), slice(dy, ey - 1 + dy), slice(dz, ez - 1 + dz))
                cv &= valid[sl]
                n_in += inside[sl]
    return cv, cv & (n_in > 0) & (n_in < 8), inside


def quad_masks(cv, inside):
    """per axis k the owner voxels a (indexed like the cells: a is the cell q2) of a crossing edge whose four cells are valid"""
    cx, cy, cz = cv.shape
    cvp = np.zeros((cx + 1, cy + 1, cz + 1), dtype=bool)  # cvp[c + 1] = cv[c]: a cell outside the cell range is not valid
    cvp[1:, 1:, 1:] = cv
    out = []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        up = [slice(0, cx), slice(0, cy), slice(0, cz)]
        up[k] = slice(1, up[k].stop + 1)
        m = inside[:cx, :cy, :cz] != inside[tuple(up)]
        for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
            sl = [slice(1, cx + 1), slice(1, cy + 1), slice(1, cz + 1)]
            if di:
                sl[i] = slice(0, sl[i].stop - 1)
            if dj:
                sl[j] = slice(0, sl[j].stop - 1)
            m = m & cvp[tuple(sl)]
        out.append(m)
    return out


def model_counts(box, any_weight=False):
    if min(box.shape) < 2:
        return 0, 0
    cv, active, inside = cell_masks(box, any_weight)
    return int(np.count_nonzero(active)), 2 * sum(int(np.count_nonzero(m)) for m in quad_masks(cv, inside))


def model_box(box, lo, res, any_weight=False):
    """the mesh of a dense box of raw entries, box[ix, iy, iz] = the voxel lo + (ix, iy, iz): (vertices, faces (n, 3) uint32)"""
    if min(box.shape) < 2:
        return np.empty(0, dtype=VERT), np.empty((0, 3), dtype=np.uint32)
    ex, ey, ez = box.shape
    value, weight = unpack(box)
    cv, active, inside = cell_masks(box, any_weight)
    c = np.nonzero(active)  # C order: ascending cell (x, y, z), z fastest
    n_v = len(c[0])
    V = np.empty((8, n_v), dtype=np.int64)
    wmin = np.full(n_v, 2 ** 32 - 1, dtype=np.int64)
    for k in range(8):  # k = dx * 4 + dy * 2 + dz
        at = (c[0] + (k >> 2), c[1] + ((k >> 1) & 1), c[2] + (k & 1))
        V[k] = value[at]
        wmin = np.minimum(wmin, np.abs(weight[at]))
    n = np.zeros(n_v, dtype=np.int64)
    s = np.zeros((3, n_v), dtype=np.int64)
    for ax in range(3):
        bit = 4 >> ax
        for k in range(8):
            if k & bit:
                continue
            va, vb = V[k], V[k | bit]
            cr = (va < 0) != (vb < 0)
            ua, ub = np.abs(va), np.abs(vb)
            m = ua + ub
            o = (2 * ua * res + m) // (2 * np.maximum(m, 1))
            n += cr
            for d in range(3):
                s[d] += np.where(cr, o if d == ax else (res if k & (4 >> d) else 0), 0)
    vert = np.empty(n_v, dtype=VERT)
    for d, name in enumerate(("x_mm", "y_mm", "z_mm")):
        vert[name] = (int(lo[d]) + c[d]) * res + res // 2 + s[d] // np.maximum(n, 1)
    vert["weight"] = wmin
    assert n_v == 0 or int(n.min()) >= 3, (n_v, int(n.min()))
    # faces
    cx, cy, cz = cv.shape
    idxp = np.zeros((cx + 1, cy + 1, cz + 1), dtype=np.int64)
    idxp[1:, 1:, 1:] = (np.cumsum(active.ravel(), dtype=np.int64) - 1).reshape(active.shape)
    keys, quads = [], []
    for k, m in enumerate(quad_masks(cv, inside)):
        i, j = (k + 1) % 3, (k + 2) % 3
        a = np.array(np.nonzero(m), dtype=np.int64)  # (3, n)
        e_i, e_j = np.zeros((3, 1), dtype=np.int64), np.zeros((3, 1), dtype=np.int64)
        e_i[i], e_j[j] = 1, 1
        q = [idxp[tuple(a + 1 - d)] for d in (e_i + e_j, e_j, 0 * e_i, e_i)]
        ins = inside[tuple(a)]
        tri = np.where(ins[None, :], np.array([q[0], q[1], q[2], q[0], q[2], q[3]]), np.array([q[0], q[2], q[1], q[0], q[3], q[2]]))
        keys.append(((a[0] * ey + a[1]) * ez + a[2]) * 3 + k)
        quads.append(tri.T)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    order = np.argsort(keys, kind="stable")
    return vert, np.ascontiguousarray(quads[order].reshape(-1, 3)).astype(np.uint32)


def model(host, res, lo=None, hi=None, any_weight=False):
    if lo is None:
        lo, hi = QM.window(host.size_, host.pos_)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    return model_box(QM.ring_box(host.data_, host.size_, host.pos_, host.offset_, lo, hi), lo, res, any_weight)


def same(got, want):
    return all(QM.same(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ properties of a mesh
def directed_edges(faces):
    f = faces.astype(np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return e[:, 0] * (int(f.max()) + 1 if len(f) else 1) + e[:, 1], e


def mesh_report(vert, faces):
    """closed (every directed edge once, its reverse once), Euler characteristic, unreferenced vertices, signed volume in mm^3"""
    key, e = directed_edges(faces)
    n = int(faces.max()) + 1 if len(faces) else 1
    uniq, cnt = np.unique(key, return_counts=True)
    rev = e[:, 1] * n + e[:, 0]
    und = np.unique(np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1]))
    p = np.stack([vert["x_mm"], vert["y_mm"], vert["z_mm"]], axis=1).astype(np.float64)
    a, b, c = (p[faces[:, k].astype(np.int64)] for k in range(3))
    return {"directed_once": bool(np.all(cnt == 1)), "closed": bool(np.all(cnt == 1)) and bool(np.all(np.isin(rev, uniq))),
            "chi": len(vert) - len(und) + len(faces), "unreferenced": len(vert) - len(np.unique(faces)),
            "volume": float(np.sum(np.einsum("ij,ij->i", a, np.cross(b, c))) / 6.0)}


SPHERES = [(24, (11.3, 12.6, 10.9), 7.3), (40, (19.2, 20.7, 18.4), 13.1)]
SPHERE_LO = (-5, 3, -7)


def sphere_box(edge, centre, radius, res=RES, tau=TAU):
    """value at voxel g = trunc(|g + 0.5 - centre| res - radius res) in float64, clipped to +-tau; weight 64"""
    import warpsense_amd as W
    g = np.stack(np.meshgrid(*(np.arange(edge, dtype=np.float64),) * 3, indexing="ij"), axis=-1) + 0.5
    d = np.sqrt(np.sum((g - np.asarray(centre, dtype=np.float64)) ** 2, axis=-1)) * res - radius * res
    return W.pack_entry(np.clip(np.trunc(d), -tau, tau).astype(np.int64), np.full(d.shape, 64)).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ arbitrary-entry maps
PLANT_PAIRS = [((-32768, 64), (32767, 64)), ((0, 64), (-1, 64)), ((-300, -1), (200, 1)), ((150, 0), (-150, 1))]  # (value, weight) at z, z + 1


def draw_entries(size, seed, tau=TAU):
    """values uniform in [-2 tau, 2 tau]; weights positive with probability 0.9, negative 0.05, zero 0.05 (a face needs 18 valid
    voxels: 0.9^18 = 0.15).  Then the edge cases, each as a pair of z neighbours inside a 2 x 2 x 3 block of positive weights so that
    the pair's cells are valid under the default rule wherever its own weights allow."""
    import warpsense_amd as W
    rng = np.random.default_rng(seed)
    n = int(np.prod(size))
    value = rng.integers(-2 * tau, 2 * tau + 1, n)
    u = rng.random(n)
    weight = np.where(u < 0.9, rng.integers(1, 641, n), np.where(u < 0.95, -rng.integers(1, 641, n), 0))
    value, weight = value.reshape(size), weight.reshape(size)
    for p, ((va, wa), (vb, wb)) in enumerate(PLANT_PAIRS):
        x, y, z = 2 + 3 * p, 3 + 2 * p, 4
        weight[x:x + 2, y:y + 2, z - 1:z + 3] = np.maximum(np.abs(weight[x:x + 2, y:y + 2, z - 1:z + 3]), 1)
        value[x, y, z], weight[x, y, z] = va, wa
        value[x, y, z + 1], weight[x, y, z + 1] = vb, wb
    return W.pack_entry(value.reshape(-1), weight.reshape(-1)).astype(np.uint32)


def check_inputs(raw, size):
    """a condition on the INPUTS: the planted pairs are there, and the model's mesh of the map is not small under either rule"""
    value, weight = unpack(raw.reshape(size))
    for p, ((va, wa), (vb, wb)) in enumerate(PLANT_PAIRS):
        x, y, z = 2 + 3 * p, 3 + 2 * p, 4
        assert (value[x, y, z], weight[x, y, z], value[x, y, z + 1], weight[x, y, z + 1]) == (va, wa, vb, wb), ((value[x, y, z], weight[x, y, z], value[x, y, z + 1], weight[x, y, z + 1]), (va, wa, vb, wb))
    for any_weight in (False, True):
        nv, nf = model_counts(raw.reshape(size), any_weight)
        assert nv > 100 and nf > 100, (size, any_weight, nv, nf)


def seeds_for(size, which):
    return sum(size) + 1000 * which + 7


def make_maps(size, seed):
    import warpsense_amd as W
    lm = W.LocalMap(*size, TAU, 0)
    lm.data[:] = draw_entries(tuple(int(s) for s in lm.size), seed)
    check_inputs(lm.data, tuple(int(s) for s in lm.size))
    params = W.Params(W.MapParams(resolution=RES, max_distance=TAU / 1000.0, max_weight=10, size=tuple(s * RES / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    other = W.LocalMap(*size, TAU, 0)
    other.data[:] = draw_entries(tuple(int(s) for s in lm.size), seed + 1000)
    check_inputs(other.data, tuple(int(s) for s in lm.size))
    tm.tsdf().new_map().to_device(other.device_map())
    return W, tm, lm


def sphere_mesh_numbers(edge, centre, radius, res=RES, tau=TAU):
    """the model's mesh of a sphere map: closed, Euler characteristic 2; returns (volume / the sphere's, largest distance of a vertex
    to the sphere in mm)"""
    box = sphere_box(edge, centre, radius, res=res, tau=tau).reshape((edge,) * 3)
    vert, face = model_box(box, SPHERE_LO, res)
    rep = mesh_report(vert, face)
    assert rep["closed"] and rep["directed_once"] and rep["chi"] == 2 and rep["unreferenced"] == 0, rep
    sphere = 4.0 / 3.0 * np.pi * (radius * res) ** 3
    p = np.stack([vert["x_mm"], vert["y_mm"], vert["z_mm"]], axis=1).astype(np.float64)
    c = (np.asarray(SPHERE_LO) + np.asarray(centre)) * res
    dist = np.abs(np.sqrt(np.sum((p - c) ** 2, axis=1)) - radius * res)
    print(edge, res, len(vert), len(face), rep["volume"] / sphere, dist.max())
    return rep["volume"] / sphere, float(dist.max())
