"""ws_map_mesh — a triangle mesh of a device map by naive surface nets (the rules are stated in include/warpsense_hip.h) against a
numpy model of exactly those rules applied to ws_map_download / ws_map_extract_box of the same map.  Everything is integer:
every comparison is on the raw bytes of the vertex records and of the face indices."""
import ctypes as C
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import test_gpu_surface as G
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERT = np.dtype([("x_mm", "<i4"), ("y_mm", "<i4"), ("z_mm", "<i4"), ("weight", "<u4")])
TAU, RES = G.TAU, G.RES
SIZES = G.SIZES


# ------------------------------------------------------------------------------------------------ the numpy model
def unpack(box):
    value = (box & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32)
    weight = (box >> 16).astype(np.uint16).view(np.int16).astype(np.int32)
    return value, weight


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
    assert n_v == 0 or int(n.min()) >= 3
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
        lo, hi = G.window(host.size_, host.pos_)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    return model_box(G.ring_box(host.data_, host.size_, host.pos_, host.offset_, lo, hi), lo, res, any_weight)


def same(got, want):
    return all(G.same(g, w) for g, w in zip(got, want))


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
        assert (value[x, y, z], weight[x, y, z], value[x, y, z + 1], weight[x, y, z + 1]) == (va, wa, vb, wb)
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


@pytest.mark.parametrize("size", SIZES)
def test_arbitrary_entries_match_the_model(size):
    import warpsense_amd as W
    n = int(np.prod(size))
    pos, off = (0, 0, 0), tuple(s // 2 for s in size)
    views = [W.DeviceMap(size, off, draw_entries(size, seed=seeds_for(size, which)), pos) for which in (0, 1)]
    for v in views:
        check_inputs(v.data_, size)
    t = W.TSDFCuda(views[0], TAU, 640, RES)
    t.new_map().to_device(views[1])
    for which in (0, 1):
        host = W.DeviceMap(size, off, np.empty(n, dtype=np.uint32), pos)
        G.wrapper(t, which).to_host(host)
        assert np.array_equal(host.data_, views[which].data_)
        for any_weight in (False, True):
            got = G.wrapper(t, which).mesh(any_weight=any_weight)
            want = model(host, RES, any_weight=any_weight)
            print(size, which, any_weight, len(want[0]), len(want[1]))
            assert len(want[0]) > 100 and len(want[1]) > 100 and same(got, want), (size, which, any_weight)


def test_rotated_rings_after_the_shift_sequence():
    W, tm, lm = make_maps((21, 17, 13), seed=5)
    for new_pos in [(3, 0, 0), (3, -4, 2), (10, -4, 2), (10, 5, -3), (-2, 5, -3)]:
        tm.shift_map(new_pos)
        assert tm.tsdf().avg_map().mesh()[0].dtype == VERT  # (a call between two shifts: the buffers follow the window)
    for which in (0, 1):
        host = G.download(W, tm, lm, which)
        assert all(int(o) != 0 for o in host.offset_) and list(host.pos_) == [-2, 5, -3]
        for any_weight in (False, True):
            got = G.wrapper(tm.tsdf(), which).mesh(any_weight=any_weight)
            want = model(host, RES, any_weight=any_weight)
            assert len(want[0]) > 100 and len(want[1]) > 100 and same(got, want), (which, any_weight)


def test_boxes():
    """a ring rotated on every axis around a window that is not at the origin, every voxel drawn (through TSDFCuda directly)"""
    import warpsense_amd as W
    size, pos, off = (21, 17, 13), (10, 5, -3), (5, 11, 9)
    data = draw_entries(size, seed=9)
    check_inputs(data, size)
    host = W.DeviceMap(size, off, data, pos)
    t = W.TSDFCuda(host, TAU, 640, RES)
    avg = t.avg_map()
    lo, hi = G.window(host.size_, host.pos_)
    whole = avg.mesh()
    assert same(whole, avg.mesh(lo=lo, hi=hi)) and same(whole, model(host, RES))
    seam = [int(lo[k] + (-(lo[k] - host.pos_[k] + host.offset_[k])) % host.size_[k]) for k in range(3)]
    assert all(lo[k] < seam[k] <= hi[k] for k in range(3)), seam
    boxes = {
        "one voxel thick": ((lo[0], lo[1], 0), (hi[0], hi[1], 0)),
        "one voxel": ((5, 3, -2), (5, 3, -2)),
        "two voxels thick": ((lo[0], seam[1] - 1, lo[2]), (hi[0], seam[1], hi[2])),
        "starts and ends mid-column": ((lo[0] + 2, lo[1] + 3, lo[2] + 1), (hi[0] - 4, hi[1] - 1, hi[2] - 2)),
        "crosses the wrap on every axis": (tuple(s - 2 for s in seam), tuple(s + 1 for s in seam)),
        "one cell column": ((lo[0], hi[1] - 1, lo[2]), (lo[0] + 1, hi[1], hi[2])),
    }
    nonempty = with_vertices = 0
    for name, (a, b) in boxes.items():
        for any_weight in (False, True):
            got = avg.mesh(lo=a, hi=b, any_weight=any_weight)
            want = model(host, RES, a, b, any_weight)
            assert same(got, want), (name, any_weight)
            assert len(got[1]) == 0 or int(got[1].max()) < len(got[0])  # faces of a box refer to vertices of that box
            nonempty += len(want[1]) > 0
            with_vertices += len(want[0]) > 0
            if "one voxel" in name:
                assert len(got[0]) == 0 and len(got[1]) == 0
    # (thin boxes have few cells and a face needs 18 valid voxels: the mid-column box alone has faces under both rules)
    print(nonempty, with_vertices)
    assert nonempty >= 2 and with_vertices >= 6
    nv, nf = C.c_size_t(9), C.c_size_t(9)
    one = (np.array([lo[0], lo[1], 0], dtype=np.int32), np.array([hi[0], hi[1], 0], dtype=np.int32))
    assert t._L.ws_map_mesh(t.handle, 0, one[0].ctypes.data_as(C.c_void_p), one[1].ctypes.data_as(C.c_void_p), 0, C.byref(nv), C.byref(nf)) == 0
    assert (nv.value, nf.value) == (0, 0)  # WS_OK, empty
    # the mesh of a box is not a subset of the whole mesh at its rim: the model decides, and the whole mesh has more
    a, b = boxes["starts and ends mid-column"]
    assert len(avg.mesh(lo=a, hi=b)[1]) < len(whole[1])
    with pytest.raises(W.WsError):
        avg.mesh(lo=(int(lo[0]) - 1, 0, 0), hi=(int(lo[0]), 0, 0))  # outside the window
    with pytest.raises(W.WsError):
        avg.mesh(lo=(0, 0, 0), hi=(0, -1, 0))


def test_sphere_on_the_device_is_closed():
    import warpsense_amd as W
    for edge, centre, radius in SPHERES:
        box = sphere_box(edge, centre, radius)
        size = (edge,) * 3
        pos = tuple(SPHERE_LO[k] + edge // 2 for k in range(3))
        off = (3, edge - 2, edge // 2)  # a rotated ring: storage holds the box in ring order
        data = np.empty(edge ** 3, dtype=np.uint32).reshape(size)
        ax = [(np.arange(SPHERE_LO[k], SPHERE_LO[k] + edge) - pos[k] + off[k] + edge) % edge for k in range(3)]
        data[np.ix_(*ax)] = box
        view = W.DeviceMap(size, off, data.reshape(-1), pos)
        t = W.TSDFCuda(view, TAU, 640, RES)
        got = t.avg_map().mesh()
        want = model_box(box, SPHERE_LO, RES)
        assert same(got, want) and same(got, model(view, RES))
        rep = mesh_report(*got)
        assert rep["closed"] and rep["chi"] == 2 and rep["unreferenced"] == 0, rep


def test_repeatable_aliased_and_partial_downloads():
    W, tm, lm = make_maps((15, 15, 15), seed=21)
    t = tm.tsdf()
    avg = t.avg_map()
    vert, face = avg.mesh()
    assert same(avg.mesh(), (vert, face))  # two calls: identical bytes
    dv, df = avg.mesh(device=True)
    assert dv.is_cuda and df.is_cuda and tuple(dv.shape) == (len(vert), 4) and tuple(df.shape) == (len(face), 3)
    nv = C.c_size_t(0)
    assert dv.data_ptr() == t._L.ws_map_mesh_vertices_dev(t.handle, C.byref(nv)) and nv.value == len(vert)
    assert df.data_ptr() == t._L.ws_map_mesh_faces_dev(t.handle, C.byref(nv)) and nv.value == len(face)
    assert np.array_equal(dv.cpu().numpy().view(np.uint8).reshape(-1), vert.view(np.uint8).reshape(-1))
    assert np.array_equal(df.cpu().numpy().view(np.uint8).reshape(-1), face.view(np.uint8).reshape(-1))
    assert same(tm.surface_mesh(), (vert, face))
    # a surface-cloud call between the mesh call and its download does not disturb it, and the other way round
    avg.mesh()
    rec = avg.surface()
    cv, cf = len(vert) // 3, len(face) // 2
    assert cv > 10 and cf > 10
    pv, pf = np.zeros(cv, dtype=VERT), np.zeros((cf, 3), dtype=np.uint32)
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    assert t._L.ws_map_mesh_download(t.handle, pv.ctypes.data_as(C.c_void_p), pf.ctypes.data_as(C.c_void_p), cv, cf, C.byref(gv), C.byref(gf)) == 0
    assert (gv.value, gf.value) == (len(vert), len(face)) and G.same(pv, vert[:cv]) and G.same(pf, face[:cf])
    assert t._L.ws_map_mesh_download(t.handle, None, None, 0, 0, C.byref(gv), C.byref(gf)) == 0 and (gv.value, gf.value) == (len(vert), len(face))
    n = C.c_size_t(0)
    got = np.zeros(len(rec), dtype=G.REC)
    assert t._L.ws_map_surface_download(t.handle, got.ctypes.data_as(C.c_void_p), None, len(rec), C.byref(n)) == 0 and G.same(got, rec)
    # an empty map: WS_OK, nothing
    lm0 = W.LocalMap(15, 15, 15, TAU, 0)
    v0, f0 = W.TSDFCuda(lm0.device_map(), TAU, 640, RES).avg_map().mesh(any_weight=True)
    assert v0.shape == (0,) and f0.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ after real scans
def test_after_real_scans_at_benchmark_size():
    """the benchmark's 131 072-point scan into the 513^3 map @ 50 mm, two updates, on a ring whose seams lie inside the window"""
    import torch
    import warpsense_amd as W
    tau, res, mw, size = 1000, 50, 640, (512, 512, 512)
    lm = W.LocalMap(*size, tau, 0)
    lm.offset[:] = (lm.size // 2 + np.array([-226, -20, 11])) % lm.size  # (every voxel is the default entry: any rotation is a valid ring)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        pos = [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor]
        t.update_tsdf(torch.from_numpy(pts).cuda(), pos, (0, 0, 32768))
    pert = S.transform_points_mm(S.os1_128_scan(), S.perturbation())
    reg = W.RegistrationCuda(None)
    reg.prepare_registration(torch.from_numpy(pert).cuda())
    T0, it0 = reg.register_cloud(t.device_map(), np.eye(4, dtype=np.float32), 200, 0.1, 0.03, res)
    t0 = time.perf_counter()
    vert, face = t.avg_map().mesh()
    print(f"513^3 mesh() incl. download: {time.perf_counter() - t0:.4f} s, {len(vert)} vertices, {len(face)} faces")
    assert same(t.avg_map().mesh(), (vert, face))
    T1, it1 = reg.register_cloud(t.device_map(), np.eye(4, dtype=np.float32), 200, 0.1, 0.03, res)
    assert it1 == it0 and it0 > 50 and np.array_equal(T0, T1)  # the call left the maps and the pending-scan state alone
    assert int(face.max()) < len(vert)
    assert np.all((face[:, 0] != face[:, 1]) & (face[:, 1] != face[:, 2]) & (face[:, 0] != face[:, 2]))  # no degenerate triangle
    host = W.DeviceMap(lm.size.copy(), lm.offset.copy(), np.empty_like(lm.data), lm.pos.copy())
    t.avg_map().to_host(host)
    lo, hi = G.window(host.size_, host.pos_)
    # whole-window counts against the model's, over x-slabs that overlap by one voxel (cells) and own their faces' owner planes
    n_v = n_f = 0
    step = 32
    for x0 in range(int(lo[0]), int(hi[0]), step):
        x1 = min(x0 + step, int(hi[0]))
        cv, active, inside = cell_masks(G.ring_box(host.data_, host.size_, host.pos_, host.offset_, (max(x0 - 1, int(lo[0])), lo[1], lo[2]), (x1, hi[1], hi[2])))
        first = 1 if x0 > int(lo[0]) else 0  # the slab's first cell plane belongs to the slab before
        n_v += int(np.count_nonzero(active[first:]))
        n_f += 2 * sum(int(np.count_nonzero(m[first:])) for m in quad_masks(cv, inside))
    assert (len(vert), len(face)) == (n_v, n_f) and n_v > 100_000, (len(vert), len(face), n_v, n_f)
    seam_x = int(lo[0] + (-(lo[0] - host.pos_[0] + host.offset_[0])) % host.size_[0])
    assert lo[0] + 40 < seam_x < hi[0] - 40
    boxes = {"around the sensor": ((-100, -100, -55), (100, 100, 55)),
             "across the x seam": ((seam_x - 30, -165, -55), (seam_x + 29, 165, 55)),
             "at a wall": ((180, -150, -45), (215, 150, 45))}
    for name, (a, b) in boxes.items():
        assert int(np.prod([b[k] - a[k] + 1 for k in range(3)])) <= 64 << 20
        got = t.avg_map().mesh(lo=a, hi=b)
        want = model(host, res, a, b)
        print(name, len(want[0]), len(want[1]))
        assert len(want[1]) > 10_000 and same(got, want), name
    fresh_v, fresh_f = t.new_map().mesh(any_weight=True)
    assert len(fresh_v) == 0 and len(fresh_f) == 0


def test_byte_offsets_beyond_4_gib():
    """the 1025^3 window of configs[2] (4.3 GB per map, device-only voxels): after a shift and one scan, a box at the far end of
    memory order against the model on ws_map_extract_box"""
    import torch
    import warpsense_amd as W
    free, _ = torch.cuda.mem_get_info()
    if free / 2 ** 30 < 24:
        if os.environ.get("WS_ALLOW_BIG_SKIP") == "1":
            pytest.skip("needs ~24 GB on the GPU")
        pytest.fail("needs ~24 GB on the GPU (set WS_ALLOW_BIG_SKIP=1 to skip on this box)")
    tau, res, mw, size = 1000, 50, 640, (1024, 1024, 1024)
    mp = W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(s * res / 1000.0 for s in size))
    lm = W.LocalMap(*size, tau, 0, host_voxels=False)
    shift = (500, -5, 3)  # (as test_gpu_surface.py: the LAST storage plane is world x = 512, inside the sensor's room)
    lm.pos[:] = shift
    lm.offset[:] = (lm.size // 2 + np.asarray(shift)) % lm.size
    tm = W.TSDFMapping(W.Params(mp), lm)
    tm.shift_map((shift[0] + 2, shift[1], shift[2] - 1))
    shift = tuple(int(v) for v in lm.pos)
    pts = S.os1_128_scan(sensor_mm=(4.0, 9.0, 2.0), seed=300) + (np.asarray(shift, dtype=np.int32) * res)[None, :]
    tm.update_tsdf(torch.from_numpy(pts).cuda(), pos_rm=list(shift), up_rm=(0, 0, 32768))
    assert tm.tsdf().stats()["error_flags"] == 0
    avg = tm.tsdf().avg_map()
    lo, hi = G.window(lm.size, lm.pos)
    n_side = int(lm.size[0])
    x_far = int(lo[0] + (n_side - 1 - (lo[0] - lm.pos[0] + lm.offset[0])) % n_side)
    assert x_far == 512 and lo[0] + 60 < x_far and x_far + 4 <= hi[0]
    for a, b in [((x_far - 59, lo[1], lo[2]), (x_far, hi[1], hi[2])),                    # the far end of memory order
                 ((x_far - 3, lo[1] + 1, lo[2] + 2), (x_far + 4, hi[1] - 3, hi[2] - 1))]:  # across the x seam
        ext = tuple(int(b[k] - a[k] + 1) for k in range(3))
        assert int(np.prod(ext)) <= 64 << 20
        box = avg.extract_box(a, b).reshape(ext)
        want = model_box(box, np.asarray(a, dtype=np.int64), res)
        got = avg.mesh(lo=a, hi=b)
        assert len(want[1]) > 1000 and same(got, want), (a, b)


# ------------------------------------------------------------------------------------------------ C++ twin
def test_cpp_twin_matches_the_python_route(tmp_path):
    import warpsense_amd as W
    cxx = shutil.which("g++")
    assert cxx is not None, "the C++ drop-in needs g++"
    exe = tmp_path / "mesh_dropin"
    lib = os.path.join(ROOT, "warpsense_amd")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}",
                           os.path.join(ROOT, "tests", "cpp", "mesh_dropin.cpp"), "-o", str(exe), f"-L{lib}", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-lwarpsense_hip", "-lpthread"])
    tau, res, mw, edge = 1000, 50, 640, 65
    pts = S.os1_128_scan(rings=32, azimuths=256, half_extents_mm=(1400.0, 1300.0, 900.0), seed=2)
    pts.tofile(tmp_path / "scan.bin")
    out = subprocess.run([str(exe), str(tmp_path / "scan.bin"), str(len(pts)), str(edge), str(res), str(tau), str(mw)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    lm = W.LocalMap(edge, edge, edge, tau, 0)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    t.update_tsdf(pts, (0, 0, 0), (0, 0, 32768))
    vert, face = t.avg_map().mesh()
    assert len(vert) > 1000 and len(face) > 1000
    assert lines["mesh"] == [str(len(vert)), str(len(face)), f"{G.fnv1a(vert.tobytes()):016x}", f"{G.fnv1a(face.tobytes()):016x}"]
    bv, bf = t.avg_map().mesh(lo=(5, -30, -25), hi=(32, 30, 25), any_weight=True)  # the room's +x wall
    assert 0 < len(bf) and len(bv) < len(vert)
    assert lines["box"] == [str(len(bv)), str(len(bf)), f"{G.fnv1a(bv.tobytes()):016x}", f"{G.fnv1a(bf.tobytes()):016x}"]
