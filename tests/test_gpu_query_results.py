"""The result holders behind ws_map_mesh, ws_store_mesh, ws_map_raycast and ws_store_raycast: the four calls share one piece of host
code, and each keeps a result of its own.  On the two-chunk-seam store of test_gpu_store_mesh and a 127^3 window loaded from it:
results do not disturb each other, every ws_debug_*_timing reader switches its own timer, and a gradient download after a call
without WS_RAYCAST_GRADIENT is refused in the name of the entry point asked.  Everything goes through the raw entry points."""
import ctypes as C

import numpy as np
import pytest

import mesh_model as M
import query_model as QM
import raycast_model as R
import store_scenes as SM

pytestmark = pytest.mark.gpu
TAU, RES, MW = SM.TAU, SM.RES, SM.MW
WS_ERR_INVALID, WS_MAP_AVG, WS_RAYCAST_GRADIENT = -1, 0, 2  # include/warpsense_hip.h
N_RAYS, RANGE = 4096, 6000
ORIGIN = np.array([-3100, -2900, -3000], dtype=np.int32)  # outside the sphere, inside the window


def rays():
    """towards points scattered around the sphere of the seam store: some rays hit it, some pass"""
    c_mm = (np.asarray(SM.SPHERE[0]) - SM.CS) * RES
    return np.ascontiguousarray(np.round(c_mm + np.random.default_rng(3).normal(size=(N_RAYS, 3)) * SM.SPHERE[1] * RES * 0.9 - ORIGIN).astype(np.int32))


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Pair:
    """a fresh seam store and a fresh 127^3 window that holds the store's voxels"""

    def __init__(self):
        import warpsense_amd as W
        self.store = SM.make_store(SM.seam_chunks())
        lm = W.LocalMap(127, 127, 127, TAU, 0)
        self.t = W.TSDFCuda(lm.device_map(), TAU, MW, RES)
        lo, hi = QM.window(lm.size, lm.pos)
        assert tuple(lo) == (-63,) * 3 and tuple(hi) == (63,) * 3
        self.store.load_box(self.t, lo, hi)
        self.L, self.dirs = self.store._L, rays()

    def close(self):
        self.t.close()
        self.store.close()

    def handle(self, q):
        return self.t.handle if q.startswith("map") else self.store.handle

    # the four calls; each returns what the entry point counted
    def call(self, q, flags=None):
        L, a, b, hits = self.L, C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
        ray_flags = WS_RAYCAST_GRADIENT if flags is None else flags
        if q == "map_mesh":
            rc = L.ws_map_mesh(self.t.handle, WS_MAP_AVG, None, None, 0, C.byref(a), C.byref(b))
        elif q == "store_mesh":
            rc = L.ws_store_mesh(self.store.handle, None, None, RES, 0, C.byref(a), C.byref(b))
        elif q == "map_ray":
            rc = L.ws_map_raycast(self.t.handle, WS_MAP_AVG, ptr(ORIGIN), ptr(self.dirs), N_RAYS, RANGE, ray_flags, C.byref(hits))
        else:
            rc = L.ws_store_raycast(self.store.handle, None, None, ptr(ORIGIN), ptr(self.dirs), N_RAYS, RANGE, RES, ray_flags, C.byref(hits))
        assert rc == 0, (q, L.ws_last_error())
        return (a.value, b.value) if q.endswith("mesh") else (hits.value,)

    # the raw download of a result, sized by what the download entry itself reports
    def download(self, q, gradient=True):
        L, h = self.L, self.handle(q)
        if q.endswith("mesh"):
            f = L.ws_map_mesh_download if q == "map_mesh" else L.ws_store_mesh_download
            nv, nf = C.c_size_t(0), C.c_size_t(0)
            assert f(h, None, None, 0, 0, C.byref(nv), C.byref(nf)) == 0
            vert, face = np.zeros(nv.value, dtype=M.VERT), np.zeros((nf.value, 3), dtype=np.uint32)
            assert f(h, ptr(vert), ptr(face), nv.value, nf.value, C.byref(nv), C.byref(nf)) == 0 and (nv.value, nf.value) == (len(vert), len(face))
            return vert, face
        f = L.ws_map_raycast_download if q == "map_ray" else L.ws_store_raycast_download
        n = C.c_size_t(0)
        assert f(h, None, None, 0, C.byref(n)) == 0
        rec, grad = np.zeros(n.value, dtype=R.RAY), np.zeros((n.value, 3), dtype=np.int32)
        rc = f(h, ptr(rec), ptr(grad) if gradient else None, n.value, C.byref(n))
        return (rec, grad) if rc == 0 else rc

    def timing(self, q, enable):
        f = {"map_mesh": self.L.ws_debug_mesh_timing, "store_mesh": self.L.ws_debug_store_mesh_timing, "map_ray": self.L.ws_debug_raycast_timing,
             "store_ray": self.L.ws_debug_store_raycast_timing}[q]
        ms = (C.c_float * 3)(-1.0, -1.0, -1.0)
        assert f(self.handle(q), enable, ms) == 0
        return tuple(float(v) for v in ms)


QUERIES = ["map_mesh", "store_mesh", "map_ray", "store_ray"]


@pytest.fixture(scope="module")
def alone():
    """per query: what it counted and what its download gave, as the only query ever made on a fresh store and a fresh window"""
    out = {}
    for q in QUERIES:
        p = Pair()
        try:
            out[q] = (p.call(q), p.download(q))
        finally:
            p.close()
    return out


def test_results_are_independent(alone):
    # the inputs: both meshes and both range images are not small, and the rays both hit and miss
    for q in ("map_mesh", "store_mesh"):
        assert min(alone[q][0]) > 100 and (len(alone[q][1][0]), len(alone[q][1][1])) == alone[q][0], q
    for q in ("map_ray", "store_ray"):
        (hits,), (rec, grad) = alone[q]
        assert 100 < hits < N_RAYS - 100 and len(rec) == N_RAYS and np.count_nonzero(rec["range_mm"] >= 0) == hits and np.any(grad != 0), q
    p = Pair()
    try:
        counted = {q: p.call(q) for q in QUERIES}
        for q in reversed(QUERIES):
            got = p.download(q)
            assert counted[q] == alone[q][0], q
            assert all(QM.same(g, w) for g, w in zip(got, alone[q][1])), q
    finally:
        p.close()


def test_timing_switches():
    p = Pair()
    try:
        for q in QUERIES:
            at = 0 if q.endswith("mesh") else 1  # the count passes / the march
            p.timing(q, 1)
            p.call(q)
            ms = p.timing(q, -1)
            print(q, "on", ms)
            assert ms[at] > 0 and min(ms) >= 0, (q, ms)
            p.call(q)
            ms = p.timing(q, -1)  # -1 has left it on
            assert ms[at] > 0 and min(ms) >= 0, (q, ms)
            p.timing(q, 0)
            p.call(q)
            assert p.timing(q, -1) == (0.0, 0.0, 0.0), q
            p.call(q)
            assert p.timing(q, -1) == (0.0, 0.0, 0.0), q  # -1 has left it off
    finally:
        p.close()


def test_gradient_download_needs_the_flag():
    p = Pair()
    try:
        for q, name in (("map_ray", b"ws_map_raycast_download"), ("store_ray", b"ws_store_raycast_download")):
            p.call(q, flags=0)
            assert p.download(q, gradient=True) == WS_ERR_INVALID, q
            assert p.L.ws_last_error().startswith(name + b":"), (q, p.L.ws_last_error())
            rec, _ = p.download(q, gradient=False)  # the records of that call are there all the same
            assert len(rec) == N_RAYS
    finally:
        p.close()
