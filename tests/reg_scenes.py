"""Registration scenes: the single-scan scene and pose error, the batch scene with its start poses and the kidnapped-robot case, and
the oracle-backed loop and Gauss-Newton backends that the sharded tests and the soak tools drive."""
import ctypes as C

import numpy as np

import oracle_lib as O
from warpsense_amd import synthetic as S


def build_scene(size=(128, 128, 64), tau=1000, res=50, mw=640, rings=64, az=512, he=(2600.0, 2300.0, 1000.0), scans=1):
    import torch
    import warpsense_amd as W
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64,
                                  size=tuple(s * res / 1000.0 for s in size)))
    lm = W.LocalMap(size[0], size[1], size[2], tau, 0)
    reg = W.TSDFRegistration(params, lm)
    oa = O.OracleMap(size, tau, 0)
    on = oa.copy()
    pts = None
    for k in range(scans):
        pts = S.os1_128_scan(rings=rings, azimuths=az, half_extents_mm=he, seed=21 + k)
        O.update_tsdf(oa, on, pts, (0, 0, 0), (0, 0, 32768), tau, mw, res)
        reg.update_tsdf(torch.from_numpy(pts).cuda(), pose=np.eye(4, dtype=np.float32))
    return reg, oa, pts, res


def pose_error(A, B):
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    dt = np.linalg.norm(A[:3, 3] - B[:3, 3]) / 1000.0  # mm -> m
    R = A[:3, :3] @ B[:3, :3].T
    # atan2 form: well conditioned near 0 (arccos of a float32-rounded trace is not)
    k = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    ang = np.arctan2(np.linalg.norm(k), (np.trace(R) - 1) / 2)
    return dt, ang


def _server(reg_cuda, enable=-1, idle_us=0):
    import ctypes as C
    n = C.c_int32(0)
    rc = reg_cuda._L.ws_debug_reg_server(reg_cuda.handle, int(enable), int(idle_us), C.byref(n))
    assert rc == 0, rc
    return n.value


# ---- the batch case: the 32 x 256 scan of test_gpu_registration's scene, one integration, the cloud moved by CLOUD_PERTURBATION
SCENE = dict(rings=32, az=256)
CLOUD_PERTURBATION = (-45, 25, 5, -2.0)
MAX_ITERATIONS, IT_WEIGHT_GRADIENT, EPSILON = 200, 0.1, 0.03
# start poses as S.perturbation(tx mm, ty mm, tz mm, rz deg); what the oracle does from each (test_reg_batch_host.py):
POSES = [(0, 0, 0, 0),                   # converges after 121 iterations
         (-35, 28, -9, -1.7),            # cut by max_iterations
         (60, 40, 0, 3.0),               # 59
         (20, -15, 5, 0.5),              # cut
         (150, -120, 20, 6.0),           # cut
         (45, -25, -5, 2.0),             # 83
         (300, 200, 0, -8),              # cut
         (1e6, 1e6, 0, 0),               # a kilometre outside the map: c == 0, one iteration, pose unchanged
         (-200, 150, 30, 10),            # 131
         (500.5, 100.25, 3.75, 11.0),    # cut
         (0, 0, 400, 0),                 # cut
         (800, 0, 0, 0)]                 # 167
ORACLE_ITERATIONS = [121, 200, 59, 200, 200, 83, 200, 1, 131, 200, 200, 167]
FAR_AWAY = 7

# ---- the kidnap case: test_gpu_registration's scene with both scans integrated, every fourth point of the moved cloud.
# The tracked pose is replaced by one 0.9 m and 20 degrees off; the lattice (0.4 m, 10 degrees) has a node 3.6 mm / 0.2 degrees
# next to the true pose.  Candidates run KIDNAP_MAX_ITERATIONS iterations only: the registration's own fixed point in this scene
# lies 2 cm above the geometric truth (the TSDF's vertical interpolation; the oracle started AT the truth ends 20 mm higher after
# 33 iterations, 8 mm after 10), so a final pose within 1e-2 m of the truth is what a short run from the right node gives, and
# the long run belongs to the tracking that follows.
KIDNAP_OFFSET_MM, KIDNAP_YAW_DEG = (803.0, -398.0, 0.0), 20.2
KIDNAP_LATTICE = dict(radius_m=0.8, step_m=0.4, yaw_range_deg=20.0, yaw_step_deg=10.0)  # 5 x 5 x 5 = 125 candidates
KIDNAP_MAX_ITERATIONS = 8
KIDNAP_MIN_FRACTION = 0.5
KIDNAP_BEST = 16  # node (-0.8 m, +0.4 m, -20 deg): what batch_best picks from the oracle's own scores


def pose_list(k):
    """k start poses drawn from POSES (repeated in order when k exceeds the list)"""
    return np.stack([S.perturbation(*POSES[i % len(POSES)]) for i in range(k)]) if k else np.zeros((0, 4, 4), dtype=np.float32)


def batch_cloud(pts):
    return S.transform_points_mm(pts, S.perturbation(*CLOUD_PERTURBATION))


def oracle_scene(rings=64, az=512, scans=1, size=(128, 128, 64), tau=1000, res=50, mw=640, he=(2600.0, 2300.0, 1000.0)):
    """the oracle half of reg_scenes.build_scene (same scans, same map), without a GPU"""
    oa = O.OracleMap(size, tau, 0)
    on = oa.copy()
    pts = None
    for k in range(scans):
        pts = S.os1_128_scan(rings=rings, azimuths=az, half_extents_mm=he, seed=21 + k)
        O.update_tsdf(oa, on, pts, (0, 0, 0), (0, 0, 32768), tau, mw, res)
    return oa, pts, res


def kidnap_case(pts):
    """(cloud, true pose float64, wrong guess float32) of the kidnap case"""
    Tp = S.perturbation(*CLOUD_PERTURBATION)
    q = S.transform_points_mm(pts, Tp)[::4]
    truth = np.linalg.inv(Tp.astype(np.float64))
    a = np.deg2rad(KIDNAP_YAW_DEG)
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    guess = truth.copy()
    guess[:3, :3] = Rz @ truth[:3, :3]
    guess[:3, 3] = truth[:3, 3] + np.array(KIDNAP_OFFSET_MM)
    return q, truth, guess.astype(np.float32)


def single(reg, poses, max_it, res, mode=None):
    """ws_register_cloud alone from every pose"""
    if mode is not None:
        reg.reg_.set_loop(mode)
    out = [reg.reg_.register_cloud(reg.tsdf().device_map(), P, max_it, IT_WEIGHT_GRADIENT, EPSILON, res) for P in poses]
    T = np.stack([o[0] for o in out]) if out else np.zeros((0, 4, 4), dtype=np.float32)
    return T, np.array([o[1] for o in out], dtype=np.int32)


def batch(reg, poses, max_it, res):
    return reg.reg_.register_cloud_batch(reg.tsdf().device_map(), poses, max_it, IT_WEIGHT_GRADIENT, EPSILON, res)


def check_batch_equals_single(reg, poses, max_it, res, modes=None):
    import warpsense_amd as W
    T, it, e, c = batch(reg, poses, max_it, res)
    assert T.shape == (len(poses), 4, 4) and T.dtype == np.float32 and it.shape == e.shape == c.shape == (len(poses),), (T.shape, T.dtype, it.shape, e.shape, c.shape, len(poses))
    for mode in (modes if modes is not None else (W.WS_REG_LOOP_RESIDENT, W.WS_REG_LOOP_LAUNCHES)):
        Ts, its = single(reg, poses, max_it, res, mode)
        assert np.array_equal(it, its), (mode, it, its)
        assert np.array_equal(T.view(np.uint32), Ts.view(np.uint32)), (mode, np.argwhere(T != Ts)[:4])
    reg.reg_.set_loop(W.WS_REG_LOOP_RESIDENT)
    # the scores: e and c of perform_registration at the final poses (one call per DISTINCT pose: the list repeats)
    seen = {}
    for k in range(len(poses)):
        key = T[k].tobytes()
        if key not in seen:
            seen[key] = reg.reg_.perform_registration(reg.tsdf().device_map(), T[k], res)[2:]
        assert (int(e[k]), int(c[k])) == seen[key], (k, e[k], c[k], seen[key])
    return T, it, e, c


class _OracleLoop:
    """the oracle's Gauss-Newton loop, one step at a time (wso_gn_begin / wso_reg_iterate / wso_gn_update)"""

    def __init__(self, omap, points, res, T_in, max_iterations, it_weight_gradient, epsilon):
        self.b = OracleGnBackend(omap, points, res)
        self.b.begin(T_in, max_iterations, it_weight_gradient, epsilon)
        self.n = points.shape[0]

    def finished(self):
        return self.b.poll()[0]

    def sums(self):
        return self.b.accumulate(0, self.n).numpy().copy()

    def update(self, sums):
        import torch
        self.b.solve(torch.from_numpy(np.ascontiguousarray(sums, dtype=np.int64)))

    def result(self):
        return self.b.poll()


# ------------------------------------------------------------------ multi-rank driver over gloo (world size 2)
class OracleGnBackend:
    """Test double for HipGnBackend: per-rank partial sums and the solve come from the CPU oracle, so the
    sharding + all-reduce + identical-solve logic of warpsense_amd.dist runs without a GPU."""

    class State(C.Structure):
        _fields_ = [("T", C.c_float * 16), ("center", C.c_int32 * 3), ("alpha", C.c_float), ("prev", C.c_float * 4),
                    ("it_weight_gradient", C.c_float), ("epsilon", C.c_float), ("max_iterations", C.c_int32),
                    ("iterations", C.c_int32), ("finished", C.c_int32)]

    def __init__(self, omap, points, res):
        import torch
        self.m, self.pts, self.res = omap, np.ascontiguousarray(points, dtype=np.int32), res
        self.st = self.State()
        self.sums = torch.zeros(44, dtype=torch.int64)

    def begin(self, T_in, max_iterations, it_weight_gradient, epsilon):
        T = O.colmajor(T_in)
        O.lib().wso_gn_begin(C.byref(self.st), O._p(T), int(max_iterations), C.c_float(it_weight_gradient), C.c_float(epsilon))

    def accumulate(self, first, count):
        T = np.ctypeslib.as_array(self.st.T).reshape(4, 4).T
        if self.st.finished or self.st.iterations >= self.st.max_iterations:
            return self.sums
        h, g, e, c = O.reg_iterate(self.m, T, self.pts[first:first + count], self.res)
        flat = np.concatenate([h.T.reshape(-1), g, [e, c]]).astype(np.int64)
        self.sums.copy_(__import__("torch").from_numpy(flat))
        return self.sums

    def solve(self, sums):
        s = np.ascontiguousarray(sums.numpy(), dtype=np.int64)
        O.lib().wso_gn_update(C.byref(self.st), O._p(s))

    def poll(self):
        fin = bool(self.st.finished or self.st.iterations >= self.st.max_iterations)
        return fin, int(self.st.iterations), np.ctypeslib.as_array(self.st.T).reshape(4, 4).T.copy()
