"""ws_register_cloud_batch without a GPU: the boundary (symbols, header, ctypes signatures), ws_reg_batch_best against an
exact-fraction model, the candidate lattice, and -- on the CPU oracle alone -- the input condition of the GPU tests in
tests/test_gpu_reg_batch.py: the committed pose list ends its loops in every possible way, the kidnap case needs the lattice."""
import ctypes as C
from fractions import Fraction
import re

import numpy as np

import oracle_lib as O
import query_model as QM
import reg_scenes as B
from warpsense_amd import synthetic as S

NEW = ["ws_register_cloud_batch", "ws_reg_batch_best"]
INT32_MAX = 2 ** 31 - 1


def test_library_exports_and_header_declares_the_batch_entry_points():
    from warpsense_amd import _lib
    import warpsense_amd as W
    L = _lib.load()
    h = QM._header()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", h), name
    # the rules are stated where the ABI is declared
    for phrase in ("bit for bit what ws_register_cloud", "k == 0 is WS_OK", "e[a] * c[b] < e[b] * c[a] in int64", "ties: larger c, then lower index",
                   "*best = -1 if none", "asked to leave first", "leaves the single route alone"):
        assert phrase in h, phrase
    assert callable(W.batch_best) and callable(W.candidate_poses)
    assert hasattr(W.RegistrationCuda, "register_cloud_batch") and hasattr(W.TSDFRegistration, "register_candidates")
    assert hasattr(W.TSDFRegistration, "relocalize")


CTYPE = {"ws_reg *": C.c_void_p, "const ws_map *": C.c_void_p, "const float *": C.c_void_p, "float *": C.c_void_p, "int32_t *": C.c_void_p,
         "const int32_t *": C.c_void_p, "size_t": C.c_size_t, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float,
         "int64_t *": C.POINTER(C.c_int64)}


def _declared(name):
    """(return type, [parameter types]) as the header declares `name`, parameter names stripped"""
    m = re.search(r"\n([A-Za-z_0-9 ]+?[ \*])" + name + r"\s*\(([^)]*)\)\s*;", QM._header())
    assert m, name
    params = [re.sub(r"\b[A-Za-z_0-9]+$", "", re.sub(r"/\*.*?\*/", "", p).strip()).strip() for p in m.group(2).split(",")]
    return m.group(1).strip(), params


def test_ctypes_signatures_agree_with_the_header():
    from warpsense_amd import _lib
    L = _lib.load()
    for name in NEW:
        ret, params = _declared(name)
        fn = getattr(L, name)
        assert list(fn.argtypes) == [CTYPE[p] for p in params], (name, params, fn.argtypes)
        assert ret == "int" and fn.restype is C.c_int, name
    assert len(_declared("ws_register_cloud_batch")[1]) == 13


def model_best(e, c, min_count):
    """the rule with exact fractions: smallest e / c among c >= min_count (and c > 0); ties: larger c, then lower index"""
    best = -1
    for i in range(len(e)):
        if c[i] < min_count or c[i] <= 0:
            continue
        if best < 0:
            best = i
            continue
        a, b = Fraction(int(e[i]), int(c[i])), Fraction(int(e[best]), int(c[best]))
        if a < b or (a == b and c[i] > c[best]):
            best = i
    return best


def test_batch_best_hand_cases():
    import warpsense_amd as W
    assert W.batch_best([], [], 1) == -1                                     # k == 0
    assert W.batch_best([10, 20, 30], [4, 5, 6], 7) == -1                    # all below min_count
    assert W.batch_best([10, 20, 30], [4, 5, 6], 6) == 2
    assert W.batch_best([10, 20, 30], [1, 2, 3], 1) == 2                     # equal ratios: the larger c
    assert W.batch_best([10, 20, 30, 5], [1, 2, 3, 0], 0) == 2               # c == 0 has no mean: never chosen
    assert W.batch_best([0, 5], [0, 1], 0) == 1
    assert W.batch_best([30, 20, 10], [3, 2, 1], 1) == 0
    assert W.batch_best([7, 7, 7], [5, 5, 5], 1) == 0                        # equal everything: the lowest index
    assert W.batch_best([0, 0], [3, 9], 1) == 1
    # near INT32_MAX: e[0] / c[0] < e[1] / c[1] by one part in 2^62 -- a cross product in 32 bits, or in double, cannot tell
    e, c = [INT32_MAX - 1, INT32_MAX], [INT32_MAX - 1, INT32_MAX]            # both ratios 1: the larger c
    assert W.batch_best(e, c, 1) == 1
    e, c = [INT32_MAX - 1, INT32_MAX], [INT32_MAX, INT32_MAX - 1]            # (M - 1) / M < M / (M - 1)
    assert W.batch_best(e, c, 1) == 0 and W.batch_best(e[::-1], c[::-1], 1) == 1
    e, c = [INT32_MAX - 2, INT32_MAX - 1], [INT32_MAX - 1, INT32_MAX]        # (M-2)/(M-1) < (M-1)/M  <=>  M^2 - 2M < M^2 - 2M + 1
    assert W.batch_best(e, c, 1) == 0 and W.batch_best(e[::-1], c[::-1], 1) == 1
    assert model_best(e, c, 1) == 0
    assert W.batch_best([5, 1], [INT32_MAX, 1], INT32_MAX) == 0


def test_batch_best_equals_the_fraction_model_on_random_draws():
    import warpsense_amd as W
    rng = np.random.default_rng(20260101)
    for trial in range(400):
        k = int(rng.integers(0, 40))
        kind = trial % 4
        if kind == 0:    # small numbers: many equal ratios and equal pairs
            e, c = rng.integers(0, 12, k), rng.integers(0, 6, k)
        elif kind == 1:  # scores of a scan
            c = rng.integers(0, 131072, k)
            e = (c * rng.integers(40, 90, k)) + rng.integers(0, 3, k)
        elif kind == 2:  # the top of the range
            e, c = INT32_MAX - rng.integers(0, 4, k), INT32_MAX - rng.integers(0, 4, k)
        else:
            e, c = rng.integers(0, INT32_MAX, k, endpoint=True), rng.integers(0, INT32_MAX, k, endpoint=True)
        e, c = e.astype(np.int32), c.astype(np.int32)
        for min_count in (0, 1, 3, int(c.max()) if k else 1, INT32_MAX):
            assert W.batch_best(e, c, min_count) == model_best(e, c, min_count), (trial, e, c, min_count)


def test_candidate_poses_count_order_and_guess_first():
    import warpsense_amd as W
    guess = S.perturbation(1234.5, -678.25, 90.0, 33.0)
    P = W.candidate_poses(guess, 0.8, 0.4, 20.0, 10.0)
    assert P.shape == (125, 4, 4) and P.dtype == np.float32
    assert np.array_equal(P[0], guess)
    # row-major over (x, y, yaw) from the most negative offsets, the all-zero node left out: the guess stands for it
    nodes = [(ix, iy, iw) for ix in range(-2, 3) for iy in range(-2, 3) for iw in range(-2, 3) if (ix, iy, iw) != (0, 0, 0)]
    for n, (ix, iy, iw) in zip(range(1, 125), nodes):
        assert np.allclose(P[n][:3, 3], guess[:3, 3] + np.array([400.0 * ix, 400.0 * iy, 0.0]), atol=1e-3), n
        yaw = np.rad2deg(np.arctan2(P[n][1, 0], P[n][0, 0]))
        assert abs(yaw - (33.0 + 10.0 * iw)) < 1e-4, (n, yaw)
        assert np.array_equal(P[n][3], [0, 0, 0, 1]) and np.array_equal(P[n][2, :3], [0, 0, 1])
    # an axis without a step stays at the guess; a radius below the step too
    assert W.candidate_poses(guess, 0.8, 0.4).shape == (25, 4, 4)
    assert W.candidate_poses(guess, 0.3, 0.4, 5.0, 10.0).shape == (1, 4, 4)
    assert W.candidate_poses(guess, 0.0, 0.0, 30.0, 10.0).shape == (7, 4, 4)


def test_candidate_poses_hand_computed_3x3x3():
    """guess: yaw 90 degrees at (1000, 2000, 300) mm; step 0.5 m, yaw step 90 degrees: the rotations are 0, 90 (the guess) and
    180 degrees, written out; x slowest, yaw fastest, the centre node replaced by the guess in front"""
    import warpsense_amd as W
    guess = np.array([[0, -1, 0, 1000], [1, 0, 0, 2000], [0, 0, 1, 300], [0, 0, 0, 1]], dtype=np.float32)
    P = W.candidate_poses(guess, 0.5, 0.5, 90.0, 90.0)
    assert P.shape == (27, 4, 4)
    rot = {-1: [[1, 0, 0], [0, 1, 0], [0, 0, 1]], 0: [[0, -1, 0], [1, 0, 0], [0, 0, 1]], 1: [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]}
    want = [guess]
    for x in (500, 1000, 1500):
        for y in (1500, 2000, 2500):
            for w in (-1, 0, 1):
                if (x, y, w) == (1000, 2000, 0):
                    continue
                T = np.eye(4, dtype=np.float32)
                T[:3, :3] = rot[w]
                T[:3, 3] = (x, y, 300)
                want.append(T)
    want = np.stack(want)
    assert np.abs(P - want).max() < 1e-6  # (cos 90 degrees in float64 is 6e-17, rounded once to float32)
    assert np.array_equal(P[1][:3, 3], [500, 1500, 300]) and np.array_equal(P[26][:3, 3], [1500, 2500, 300])
    assert np.array_equal(P[13][:3, 3], [1000, 2000, 300]) and np.array_equal(P[14][:3, 3], [1000, 2000, 300])  # yaw -90 / +90 in place


def test_committed_pose_list_ends_its_loops_in_every_way():
    """the input condition of test_gpu_reg_batch, on the oracle: converged, cut, no correspondences, different counts"""
    oa, pts, res = B.oracle_scene(**B.SCENE)
    q = B.batch_cloud(pts)
    poses = B.pose_list(len(B.POSES))
    its = []
    for k, P in enumerate(poses):
        T, it, _ = O.register_cloud(oa, q, P, B.MAX_ITERATIONS, B.IT_WEIGHT_GRADIENT, B.EPSILON, res)
        e, c = O.reg_iterate(oa, T, q, res, 0)[2:]
        its.append(it)
        if k == B.FAR_AWAY:
            assert it == 1 and c == 0 and np.array_equal(T, P)
        else:
            assert c > 1000
    assert its == B.ORACLE_ITERATIONS
    converged = [i for i in its if 1 < i < B.MAX_ITERATIONS]
    assert len(converged) >= 1 and its.count(B.MAX_ITERATIONS) >= 1 and len(set(converged)) >= 2
    # K = 7, the smallest batch of the size and flag tests, already mixes the endings at their lower limits
    assert len(set(B.ORACLE_ITERATIONS[:7])) >= 3


def test_kidnap_case_needs_the_lattice_and_the_lattice_finds_the_pose():
    import warpsense_amd as W
    oa, pts, res = B.oracle_scene(scans=2)
    q, truth, guess = B.kidnap_case(pts)
    prm = W.RegistrationParams()
    poses = W.candidate_poses(guess, **B.KIDNAP_LATTICE)
    assert len(poses) == 125
    finals = [O.register_cloud(oa, q, P, B.KIDNAP_MAX_ITERATIONS, prm.it_weight_gradient, prm.epsilon, res)[0] for P in poses]
    ec = np.array([O.reg_iterate(oa, T, q, res, 0)[2:] for T in finals], dtype=np.int32)
    best = W.batch_best(ec[:, 0], ec[:, 1], int(np.ceil(B.KIDNAP_MIN_FRACTION * len(q))))
    assert best == B.KIDNAP_BEST
    dt, ang = B.pose_error(finals[best], truth)
    assert dt < 1e-2 and ang < 1e-2, (dt, ang)
    # the wrong guess alone (candidate 0 is the guess itself) ends farther from the truth than the best candidate
    alone = B.pose_error(finals[0], truth)
    assert alone[0] > dt and alone[1] > ang and alone[0] > 0.5, alone
    # ... also when it is given the tracker's full iteration budget
    T200 = O.register_cloud(oa, q, guess, prm.max_iterations, prm.it_weight_gradient, prm.epsilon, res)[0]
    assert B.pose_error(T200, truth)[0] > dt
