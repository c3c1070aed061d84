"""The case table of the Gauss-Newton unit tests: start states and sequences of SYNTHETIC sums, built backwards from the step each
update is meant to take, with the state the oracle (wso_gn_begin / wso_gn_update) leaves after every update -- all from fixed seeds,
no GPU, no fixtures.  tests/test_gn_cases_host.py proves on the oracle alone that every class does what it claims;
tests/test_gpu_gn_units.py runs every device form of the update (tests/cpp/gn_units.hip) and two routes of the C ABI on them.

A sequence is a start state (pose T column-major, max_iterations, it_weight_gradient, epsilon) and 1 .. 8 sets of sums.  A set is the
29 slot totals of reg_reduce.h (21 h, 6 g, e, c: int64) and the reference's 44 words made from them (word_slot / word_value below,
restated from reg_reduce.h: e and c are the low 32 bits of their slots, sign-extended).

An update solves (H + w I) x = g with w = (double)(alpha * (float)c) and steps by xi = -x, so a wanted xi is reached with
g = -round((H + w I) xi), computed exactly (integers) from the damping the oracle's state has at that moment.  H is an integer
matrix, symmetric and positive definite unless the class says otherwise.  What a class claims is held by the host test through
the oracle's own solve (Update.xi / Update.theta), never through the target the sums were built from.

Classes (Sequence.cls; an update may carry further tags in Update.tags):
    small_theta        theta log-uniform in [1e-12, 0.25); the tag `tiny` marks theta < 1e-9
    theta_zero         a rotational gradient of exactly zero, H block-diagonal: theta == 0, a pure translation
    quarter_exact      theta == 0.25, the branch point of gn_step (H = 4 I, g = (-1, 0, ..) and its like)
    quarter_below      0 < 0.25 - theta <= 8 ulp: ratios of integers around 2^53 / 2^55
    quarter_above      0 < theta - 0.25 <= 1e-6
    large_theta        theta uniform in [0.25, pi]
    huge_theta         theta in (pi, 7]
    axis_aligned       rotation about +-x, +-y, +-z, thetas on both sides of the branch
    sign_patterns      each of the 64 sign patterns of xi, below and above the branch
    far_pose           start poses 20 .. 60 m from the origin (centre: tens of metres in mm)
    history            eight updates in a row: T, alpha and prev carried forward
    c_zero_first, c_zero_later            c == 0 (also as the low word of a slot total k 2^32): the loop finishes, pose untouched
    c_values           c in {1, 2^24 + 1, 2^31 - 1}, with the damping on from the second update
    c_high_word        a c slot total 2^32 m + k: c is k
    e_high_word        an e slot total whose low word is negative and whose high word is not its sign extension
    singular_zero      H = 0 at alpha 0
    singular_rank      a rank-deficient H (a zero row and column; two equal rows)
    zero_h_damped      H = 0 with alpha > 0, c > 0: the damping alone carries the step
    pivot_first, pivot_later, pivot_tie   a strictly larger element below the diagonal in step 0 only / in one later step only;
                                          an element below the diagonal of exactly the diagonal's magnitude (no exchange)
    large_sums         H and g entries above 2^53, up to 2^62
    converge_equal, converge_below, converge_one_fails    e / c sequences that put a difference exactly at epsilon (no end), one
                                          float below it (end), and only one of the two differences below it (no end)
    max_iterations     max_iterations in {0, 1, 3} under a sequence of five sets
    after_finished     one more set after the loop has finished: it changes nothing

A sequence one of whose expected poses is not finite is dropped (a NaN's bits are no contract); `dropped()` counts them per class.
"""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
from reg_scenes import OracleGnBackend

MAX_UPDATES = 8
N_TERMS, N_SLOTS, N_WORDS = 29, 32, 44
STATE_WORDS = 23  # T[16], alpha, prev[4], iterations, finished as 32-bit patterns
QUARTER_ULP = 2.0 ** -55  # the spacing of doubles just below 0.25

CLASSES = ["small_theta", "theta_zero", "quarter_exact", "quarter_below", "quarter_above", "large_theta", "huge_theta", "axis_aligned",
           "sign_patterns", "far_pose", "history", "c_zero_first", "c_zero_later", "c_values", "c_high_word", "e_high_word",
           "singular_zero", "singular_rank", "zero_h_damped", "pivot_first", "pivot_later", "pivot_tie", "large_sums", "converge_equal",
           "converge_below", "converge_one_fails", "max_iterations", "after_finished"]
# the interval the oracle's theta of an update with that tag lies in: (low, high, low closed, high closed)
THETA_INTERVALS = {
    "small": (1e-12, 0.25, True, False),
    "tiny": (1e-12, 1e-9, True, False),
    "zero": (0.0, 0.0, True, True),
    "quarter_exact": (0.25, 0.25, True, True),
    "quarter_below": (0.25 - 8 * QUARTER_ULP, 0.25, True, False),
    "quarter_above": (0.25, 0.25 + 1e-6, False, True),
    "large": (0.25, np.pi, True, True),
    "huge": (np.pi, 7.0, False, True),
}


# ---- the slots and words of reg_reduce.h, restated
def tri_index(i, j):
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


def h_slot(r, c):
    return tri_index(r, c) if r <= c else tri_index(c, r)


def word_slot(k):
    return h_slot(k % 6, k // 6) if k < 36 else (21 + (k - 36) if k < 42 else 27 + (k - 42))


def low_word(v):
    """the low 32 bits of an int64 as a signed int"""
    v = int(v) & 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def word_value(k, slot_value):
    return int(slot_value) if k < 42 else low_word(slot_value)


def make_slots(H, g, e_total, c_total):
    s = np.zeros(N_TERMS, dtype=np.int64)
    for i in range(6):
        for j in range(i, 6):
            assert int(H[i][j]) == int(H[j][i])
            s[tri_index(i, j)] = int(H[i][j])
        s[21 + i] = int(g[i])
    s[27], s[28] = int(e_total), int(c_total)
    return s


def make_words(slots):
    return np.array([word_value(k, slots[word_slot(k)]) for k in range(N_WORDS)], dtype=np.int64)


# ---- the oracle's state and solve
State = OracleGnBackend.State


def snapshot(st):
    w = np.zeros(STATE_WORDS, dtype=np.uint32)
    w[:16] = np.ctypeslib.as_array(st.T).view(np.uint32)
    w[16] = np.float32(st.alpha).view(np.uint32)
    w[17:21] = np.ctypeslib.as_array(st.prev).view(np.uint32)
    w[21], w[22] = np.uint32(st.iterations), np.uint32(st.finished)
    return w


def damping(alpha, c):
    """w = (double)(alpha * (float)c), the float product of tsdf_registration.cpp:66"""
    return float(np.float32(alpha) * np.float32(int(c)))


def system(words, alpha):
    """(A row-major 6x6, b) in double as wso_gn_update builds them from the 44 words"""
    w = damping(alpha, low_word(words[43]))
    A = np.array([[float(int(words[q * 6 + r])) + (w if r == q else 0.0) for q in range(6)] for r in range(6)], dtype=np.float64)
    b = np.array([float(int(words[36 + r])) for r in range(6)], dtype=np.float64)
    return A, b


def oracle_solve(A, b):
    """(status, x) of wso_solve6"""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(6, dtype=np.float64)
    rc = O.lib().wso_solve6(O._p(A), O._p(b), O._p(x))
    return int(rc), x


def solve6_trace(A, b):
    """wso_solve6 restated in Python doubles: (status, x, pivot row of each step taken).  The host test holds x to the oracle's, bit
    for bit, before it trusts the pivots.  A pivot row other than k is what WS_SOLVE_DIAG_FIRST's ballot decides on."""
    A = [[float(v) for v in row] for row in np.asarray(A, dtype=np.float64)]
    b = [float(v) for v in b]
    inv, pivots = [0.0] * 6, []
    for k in range(6):
        piv, best = k, abs(A[k][k])
        for i in range(k + 1, 6):
            if abs(A[i][k]) > best:
                best, piv = abs(A[i][k]), i
        if best == 0.0:
            return -1, None, pivots
        pivots.append(piv)
        if piv != k:
            A[k], A[piv] = A[piv], A[k]
            b[k], b[piv] = b[piv], b[k]
        inv[k] = 1.0 / A[k][k]
        for i in range(6):
            if i == k:
                continue
            f = A[i][k] * inv[k]
            for j in range(k + 1, 6):
                A[i][j] -= f * A[k][j]
            b[i] -= f * b[k]
    return 0, np.array([b[i] * inv[i] for i in range(6)], dtype=np.float64), pivots


class Update:
    """one set of sums, the oracle's state before and after it, and what it was built for"""

    def __init__(self, slots, words, before, after, alpha_before, live, tags):
        self.slots, self.words, self.before, self.after = slots, words, before, after
        self.alpha_before, self.live, self.tags = alpha_before, live, tuple(tags)

    @property
    def c(self):
        return low_word(self.slots[28])

    @property
    def e(self):
        return low_word(self.slots[27])

    @property
    def stepped(self):
        """the oracle built a transform in this update (live, c != 0, not singular): the pose product and the convergence test ran"""
        return self.live and self.c != 0 and self.solve()[0] == 0

    def solve(self):
        return oracle_solve(*system(self.words, self.alpha_before))

    def xi(self):
        rc, x = self.solve()
        return None if rc else -x

    def theta(self):
        xi = self.xi()
        return None if xi is None else float(np.sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]))

    def pivots(self):
        return solve6_trace(*system(self.words, self.alpha_before))[2]


class Sequence:
    def __init__(self, cls, T0, max_iterations, it_weight_gradient, epsilon, updates, finish_at=None):
        self.cls, self.T0, self.max_iterations = cls, T0, int(max_iterations)
        self.it_weight_gradient, self.epsilon = np.float32(it_weight_gradient), np.float32(epsilon)
        self.updates, self.finish_at = updates, finish_at  # finish_at: the update whose convergence test is expected to end the loop

    def pose(self):
        """the start pose in math layout, as HipGnBackend.begin takes it"""
        return self.T0.reshape(4, 4).T.copy()

    def finite(self):
        return all(np.isfinite(u.after[:16].view(np.float32)).all() for u in self.updates)


def _round_ratio(n, d):
    """n / d (d > 0) rounded to the nearest integer, ties to even"""
    q, r = divmod(n, d)
    return q + (1 if 2 * r > d or (2 * r == d and q % 2) else 0)


class _Builder:
    def __init__(self, cls, T0, max_iterations=200, it_weight_gradient=0.1, epsilon=0.03):
        self.cls, self.T0 = cls, np.ascontiguousarray(T0, dtype=np.float32).reshape(16)
        self.args = (int(max_iterations), np.float32(it_weight_gradient), np.float32(epsilon))
        self.st = State()
        O.lib().wso_gn_begin(C.byref(self.st), O._p(self.T0), self.args[0], C.c_float(self.args[1]), C.c_float(self.args[2]))
        self.updates, self.finish_at = [], None

    @property
    def alpha(self):
        return np.float32(self.st.alpha)

    @property
    def live(self):
        return not self.st.finished and self.st.iterations < self.st.max_iterations

    def gradient(self, H, xi, c):
        """g = -round((H + w I) xi), exactly (every double is an integer over a power of two), with the damping this update will see"""
        wn, wd = damping(self.alpha, low_word(c)).as_integer_ratio()
        ratios = [float(v).as_integer_ratio() for v in xi]
        xd = max(d for _, d in ratios)
        x = [n * (xd // d) for n, d in ratios]
        den = wd * xd
        return [-_round_ratio(sum((int(H[i][j]) * wd + (wn if i == j else 0)) * x[j] for j in range(6)), den) for i in range(6)]

    def push(self, H, g, e_total, c_total, tags=()):
        slots = make_slots(H, g, e_total, c_total)
        words = make_words(slots)
        before, alpha, live = snapshot(self.st), self.alpha, self.live
        O.lib().wso_gn_update(C.byref(self.st), O._p(words))
        self.updates.append(Update(slots, words, before, snapshot(self.st), alpha, live, tags))
        return self.updates[-1]

    def step(self, H, xi, e, c, tags=(), e_total=None, c_total=None):
        c_total = c if c_total is None else c_total
        return self.push(H, self.gradient(H, xi, c_total), e if e_total is None else e_total, c_total, tags)

    def done(self):
        assert 1 <= len(self.updates) <= MAX_UPDATES
        return Sequence(self.cls, self.T0, *self.args, self.updates, self.finish_at)


# ---- ingredients
def _rotation(rv):
    rv = np.asarray(rv, dtype=np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def start_pose(rng, reach_mm=5000.0, min_mm=0.0):
    """a rigid start pose, column-major float32"""
    T = np.eye(4)
    T[:3, :3] = _rotation(_unit(rng) * rng.uniform(0, np.pi))
    t = rng.uniform(-reach_mm, reach_mm, 3)
    if min_mm:
        t = np.where(np.abs(t) < min_mm, np.sign(t) * min_mm + t, t)
    T[:3, 3] = t
    return np.ascontiguousarray(T.T, dtype=np.float32).reshape(16)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def spd(rng):
    """a random symmetric positive definite integer matrix: A A^T + s^2 I with the rotational rows scaled up as a scan's are"""
    s = int(10 ** rng.uniform(1, 5))
    m = int(rng.choice([1, 10, 1000]))
    A = [[int(v) for v in row] for row in rng.integers(-s, s + 1, (6, 8))]
    d = [m, m, m, 1, 1, 1]
    return [[d[i] * d[j] * (sum(A[i][k] * A[j][k] for k in range(8)) + (s * s if i == j else 0)) for j in range(6)] for i in range(6)]


def dominant(rng, lo_bits, hi_bits, off_bits):
    """a diagonally dominant (hence positive definite) integer matrix with diagonal entries in [2^lo_bits, 2^hi_bits)"""
    H = [[0] * 6 for _ in range(6)]
    for i in range(6):
        H[i][i] = int(rng.integers(1 << lo_bits, 1 << hi_bits))
        for j in range(i):
            H[i][j] = H[j][i] = int(rng.integers(-(1 << off_bits), (1 << off_bits) + 1))
    return H


def diag(values):
    return [[int(values[i]) if i == j else 0 for j in range(6)] for i in range(6)]


def make_xi(rng, theta, axis=None, reach_mm=50.0):
    axis = _unit(rng) if axis is None else np.asarray(axis, dtype=np.float64)
    return np.concatenate([axis * theta, rng.uniform(-reach_mm, reach_mm, 3)])


def _errors(rng, k):
    """(e, c) of update k of an ordinary sequence: mean errors 14 apart between an update and the one two before it, so that the
    convergence test (epsilon 0.03) never ends such a sequence"""
    c = int(rng.integers(1000, 200000))
    return int(round((100.0 - 7.0 * k + rng.uniform(0, 1)) * c)), c


_SAMPLERS = {
    "small": lambda rng: float(np.exp(rng.uniform(np.log(1e-12), np.log(0.25)))),
    "tiny": lambda rng: float(np.exp(rng.uniform(np.log(1.2e-12), np.log(0.8e-9)))),
    "quarter_above": lambda rng: 0.25 + float(rng.uniform(1e-9, 0.9e-6)),
    "large": lambda rng: float(rng.uniform(0.25, np.pi)),
    "huge": lambda rng: float(rng.uniform(np.pi + 1e-3, 7.0)),
}


def _h_for(rng, tag):
    # a tiny rotation beside millimetres of translation needs g's rounding (half a unit) far below H theta: large entries
    return dominant(rng, 50, 56, 44) if tag in ("tiny", "small", "quarter_above") else spd(rng)


def targeted_step(b, rng, tag, k, axis=None, signs=None, H=None):
    """one ordinary update aimed at the interval of `tag`; the aim is checked against the oracle's own theta and redrawn if the
    rounding of g moved it out (the draws are seeded: the table is the same on every machine)"""
    saved = bytes(b.st)
    for _ in range(20):
        xi = make_xi(rng, _SAMPLERS[tag](rng), axis)
        if signs is not None:
            xi = np.where(xi == 0, 1e-3, np.abs(xi)) * signs
        e, c = _errors(rng, k)
        u = b.step(H if H is not None else _h_for(rng, tag), xi, e, c, (tag,))
        th = u.theta()
        if not u.live or (th is not None and _in(th, tag)):
            if u.live and tag == "small" and _in(th, "tiny"):
                u.tags = u.tags + ("tiny",)
            return u
        b.updates.pop()
        C.memmove(C.byref(b.st), saved, len(saved))
    raise AssertionError(f"no step into {tag}")


def _in(theta, tag):
    lo, hi, lo_closed, hi_closed = THETA_INTERVALS[tag]
    return (theta > lo or (lo_closed and theta == lo)) and (theta < hi or (hi_closed and theta == hi))


# ---- the classes
def _gen_small(rng, i):
    b = _Builder("small_theta", start_pose(rng))
    for k in range(1 + i % 4):
        targeted_step(b, rng, "tiny" if i % 5 == 0 and k == 0 else "small", k)
    return b.done()


def _gen_theta_zero(rng, i):
    b = _Builder("theta_zero", start_pose(rng), it_weight_gradient=0.1 if i % 2 else 0.0)
    for k in range(1 + i % 3):
        Hr, Ht = spd(rng), spd(rng)
        H = [[(Hr[r][c] if r < 3 and c < 3 else (Ht[r][c] if r >= 3 and c >= 3 else 0)) for c in range(6)] for r in range(6)]
        xi = np.concatenate([[0.0, 0.0, 0.0], rng.uniform(-80, 80, 3)])
        e, c = _errors(rng, k)
        g = b.gradient(H, xi, c)
        assert g[:3] == [0, 0, 0]
        b.push(H, g, e, c, ("zero",))
    return b.done()


def _axis(i):
    a = np.zeros(3)
    a[i % 3] = -1.0 if (i // 3) % 2 else 1.0
    return a


def _gen_quarter_exact(rng, i):
    """x = g (1 / N) with N a power of two: xi is g / N exactly, and sqrt(xi^2) is |xi|"""
    b = _Builder("quarter_exact", start_pose(rng))
    n_bits = [2, 2, 10, 55][i % 4]
    H = diag([1 << n_bits] * 6)
    g = [0] * 6
    a = _axis(i)
    for k in range(3):
        g[k] = -int(a[k]) * (1 << (n_bits - 2))
    if i % 4 != 0:  # with a translation beside it (multiples of 1 / 4 at the least)
        for k in range(3, 6):
            g[k] = -int(rng.integers(-40, 41)) * (1 << (n_bits - 2))
    e, c = _errors(rng, 0)
    b.push(H, g, e, c, ("quarter_exact",))
    if i % 2:
        targeted_step(b, rng, "small", 1)
    return b.done()


def _gen_quarter_below(rng, i):
    b = _Builder("quarter_below", start_pose(rng))
    H = diag([1 << 55] * 6)
    a = _axis(i)
    ulps = 1 + (i // 6) % 8
    g = [0] * 6
    for k in range(3):
        g[k] = -int(a[k]) * ((1 << 53) - ulps)
    for k in range(3, 6):
        g[k] = -int(rng.integers(-40, 41)) * (1 << 53)
    e, c = _errors(rng, 0)
    b.push(H, g, e, c, ("quarter_below",))
    return b.done()


def _gen_quarter_above(rng, i):
    b = _Builder("quarter_above", start_pose(rng))
    if i % 2:
        # the first doubles above 0.25 (spacing 2^-54): g = 2^53 + 2 j over N = 2^55
        H = diag([1 << 55] * 6)
        a = _axis(i // 2)
        j = 1 + (i // 12) if i < 60 else int(rng.integers(1, 1 << 34))
        g = [0] * 6
        for k in range(3):
            g[k] = -int(a[k]) * ((1 << 53) + 2 * j)
        e, c = _errors(rng, 0)
        b.push(H, g, e, c, ("quarter_above",))
    else:
        targeted_step(b, rng, "quarter_above", 0)
    return b.done()


def _gen_large(rng, i):
    b = _Builder("large_theta", start_pose(rng), it_weight_gradient=[0.1, 0.0, 0.05, 1.0][i % 4])
    for k in range(1 + i % 3):
        targeted_step(b, rng, "large", k)
    return b.done()


def _gen_huge(rng, i):
    b = _Builder("huge_theta", start_pose(rng))
    targeted_step(b, rng, "huge", 0)
    if i % 2:
        targeted_step(b, rng, "small", 1)
    return b.done()


def _gen_axis(rng, i):
    b = _Builder("axis_aligned", start_pose(rng))
    tags = ["small", "large", "tiny", "quarter_above", "huge"]
    for k in range(2):
        # the rotational block diagonal and uncoupled from the translation: the two other components of xi are exactly zero
        H = dominant(rng, 50, 56, 44)
        for r in range(3):
            for q in range(6):
                if q != r:
                    H[r][q] = H[q][r] = 0
        targeted_step(b, rng, tags[(i // 6 + k) % len(tags)], k, axis=_axis(i), H=H)
    return b.done()


def _gen_signs(rng, i):
    signs = np.array([-1.0 if (i >> k) & 1 else 1.0 for k in range(6)])
    b = _Builder("sign_patterns", start_pose(rng))
    targeted_step(b, rng, "large" if (i >> 6) & 1 else "small", 0, signs=signs)
    return b.done()


def _gen_far(rng, i):
    b = _Builder("far_pose", start_pose(rng, 60000.0, 20000.0))
    tags = ["small", "large", "small", "quarter_above", "tiny"]
    for k in range(1 + i % 3):
        targeted_step(b, rng, tags[(i + k) % len(tags)], k)
    return b.done()


def _gen_history(rng, i):
    b = _Builder("history", start_pose(rng, 30000.0 if i % 3 == 0 else 5000.0), it_weight_gradient=[0.1, 0.5, 0.01][i % 3])
    for k in range(MAX_UPDATES):
        targeted_step(b, rng, "large" if (i + k) % 4 == 0 else "small", k)
    return b.done()


def _gen_c_zero(rng, i, first):
    b = _Builder("c_zero_first" if first else "c_zero_later", start_pose(rng))
    at = 0 if first else 1 + i % 4
    for k in range(at):
        targeted_step(b, rng, "small" if k % 2 else "large", k)
    H = spd(rng)
    c_total = 0 if i % 2 == 0 else int(rng.integers(1, 1 << 20)) << 32  # c is the slot's low word
    b.push(H, b.gradient(H, make_xi(rng, 0.1), 0), int(rng.integers(0, 1000)), c_total, ("c_zero",))
    if i % 3 == 0:
        targeted_step(b, rng, "small", at + 1)  # and nothing after it
    return b.done()


def _gen_c_values(rng, i):
    c = [1, (1 << 24) + 1, (1 << 31) - 1][i % 3]
    b = _Builder("c_values", start_pose(rng), it_weight_gradient=[0.1, 0.7][(i // 3) % 2])
    for k in range(3):
        # H of the damping's own magnitude at the two large c, so that the rounding of (float)c reaches the step
        H = dominant(rng, 26, 30, 20) if c > 1 else spd(rng)
        e = int(round((100.0 - 7.0 * k + rng.uniform(0, 1)) * min(c, 1 << 24)))
        b.step(H, make_xi(rng, _SAMPLERS["small" if k % 2 else "large"](rng)), e, c, ("c_value",))
    return b.done()


def _gen_c_high(rng, i):
    b = _Builder("c_high_word", start_pose(rng))
    for k in range(2 + i % 2):
        e, c = _errors(rng, k)
        c_total = (int(rng.integers(1, 1 << 30)) << 32) + c
        b.step(spd(rng), make_xi(rng, _SAMPLERS["small"](rng)), e, c, ("c_high",), c_total=c_total)
    return b.done()


def _gen_e_high(rng, i):
    b = _Builder("e_high_word", start_pose(rng))
    for k in range(2 + i % 2):
        e, c = _errors(rng, k)
        low = (-e) & 0xffffffff  # a negative low word ...
        e_total = (int(rng.integers(0, 1 << 30)) << 32) | low  # ... under a high word that is not its sign extension
        assert low_word(e_total) == -e < 0
        b.step(spd(rng), make_xi(rng, _SAMPLERS["small"](rng)), e, c, ("e_high",), e_total=e_total)
    return b.done()


def _gen_singular(rng, i, zero):
    # it_weight_gradient 0 keeps alpha at 0, so that a later update can be singular as well
    at = i % 3
    b = _Builder("singular_zero" if zero else "singular_rank", start_pose(rng), it_weight_gradient=0.0)
    for k in range(at):
        targeted_step(b, rng, "small", k)
    e, c = _errors(rng, at)
    if zero:
        H = diag([0] * 6)
    else:
        H = spd(rng)
        kind, r = (i // 3) % 2, int(rng.integers(0, 6))
        if kind == 0:  # a zero row and column
            for j in range(6):
                H[r][j] = H[j][r] = 0
        else:
            # row q a copy of row 0 (and column q of column 0) under a first pivot that is a power of two and the largest of its
            # column: the multiplier H[q][0] * (1 / H[0][0]) is exactly 1, row and column q are eliminated to exactly zero in
            # step 0 and stay zero, and step q finds no pivot.  (The multipliers come from the pivot's reciprocal: under any other
            # pivot two equal rows leave a rounding error, not a zero.)
            q = 1 + int(rng.integers(0, 5))
            H[0][0] = 1 << int(max(abs(v) for v in H[0])).bit_length()
            for j in range(6):
                H[q][j] = H[j][q] = H[0][j]
            H[q][q] = H[0][q] = H[q][0] = H[0][0]
    g = [int(v) for v in rng.integers(-10 ** 6, 10 ** 6, 6)]
    b.push(H, g, e, c, ("singular",))
    if i % 2:
        targeted_step(b, rng, "small", at + 1)
    return b.done()


def _gen_zero_h(rng, i):
    b = _Builder("zero_h_damped", start_pose(rng), it_weight_gradient=[0.1, 1.0, 0.03][i % 3])
    targeted_step(b, rng, "small", 0)  # alpha is 0 in the first update
    for k in range(1, 2 + i % 3):
        e, c = _errors(rng, k)
        b.step(diag([0] * 6), make_xi(rng, _SAMPLERS["small" if (i + k) % 2 else "large"](rng)), e, c, ("zero_h",))
    return b.done()


def _pivot_matrix(rng, at, tie):
    """diagonally dominant but for one 2 x 2 block at (at, at + 1) whose off-diagonal element is larger than (tie: as large as) its
    first diagonal element; the block is uncoupled from the rows above it, so elimination reaches it unchanged"""
    s = int(10 ** rng.uniform(1, 5))
    H = [[0] * 6 for _ in range(6)]
    for r in range(6):
        H[r][r] = int(rng.integers(900, 1100)) * s
        for q in range(r):
            H[r][q] = H[q][r] = int(rng.integers(-2, 3)) * s
    sign = -1 if rng.random() < 0.5 else 1
    H[at][at] = 30 * s if tie else 10 * s
    H[at][at + 1] = H[at + 1][at] = sign * 30 * s
    for q in range(6):
        if q not in (at, at + 1):
            H[at][q] = H[q][at] = 0
            H[at + 1][q] = H[q][at + 1] = 0
    return H


def _gen_pivot(rng, i, kind):
    b = _Builder("pivot_" + kind, start_pose(rng), it_weight_gradient=0.0)
    n_before = i % 2
    for k in range(n_before):
        targeted_step(b, rng, "small", k)
    at = 0 if kind == "first" else (1 + i % 4 if kind == "later" else i % 5)
    e, c = _errors(rng, n_before)
    b.step(_pivot_matrix(rng, at, kind == "tie"), make_xi(rng, _SAMPLERS["small" if i % 3 else "large"](rng)), e, c, ("pivot_" + kind, f"at{at}"))
    return b.done()


def _gen_large_sums(rng, i):
    b = _Builder("large_sums", start_pose(rng))
    for k in range(1 + i % 3):
        top = 62 if (i + k) % 2 else 61
        H = dominant(rng, top - 1, top, 57)
        reach = 0.35 if top == 62 else 0.9
        xi = rng.uniform(-reach, reach, 6) / np.sqrt(3.0)
        e, c = _errors(rng, k)
        b.step(H, xi, e, c, ("large_sums",))
    return b.done()


def _gen_converge(rng, i, kind):
    """c = 1024 makes every mean error e / 1024 exact; the fifth update compares its error with the third's (prev[2]) and the first's
    (prev[0]), both differences multiples of 1 / 1024.  The first four cannot end the loop: prev[0] is still 0 and the errors are large."""
    c, d = 1024, int(rng.integers(8, 200))  # the difference under test: d / 1024
    sgn, sgn2 = (-1 if i % 2 else 1), (-1 if (i // 4) % 2 else 1)  # of the difference under test, of the other one
    eps = np.float32(d / 1024.0)
    assert float(eps) * 1024 == d
    e5 = int(rng.integers(60000, 90000))
    if kind == "equal":  # one difference exactly epsilon (not below it), the other small
        e3, e1 = (e5 - sgn * d, e5 + sgn2) if (i // 2) % 2 else (e5 - sgn2, e5 - sgn * d)
    elif kind == "below":  # epsilon one float above the larger difference
        eps = np.nextafter(eps, np.float32(np.inf))
        small = sgn2 * int(rng.integers(1, d))
        e3, e1 = (e5 - sgn * d, e5 - small) if (i // 2) % 2 else (e5 - small, e5 - sgn * d)
    else:  # one of the two below epsilon, the other not
        e3, e1 = (e5 - sgn * (d - 1), e5 + sgn * (d + int(rng.integers(0, 3)))) if (i // 2) % 2 else (e5 + sgn * (d + int(rng.integers(0, 3))), e5 - sgn * (d - 1))
    es = [e1, e5 + 20000, e3, e5 - 30000, e5, e5 + 40000]
    b = _Builder("converge_" + kind, start_pose(rng), epsilon=eps)
    for k, e in enumerate(es):
        b.step(spd(rng), make_xi(rng, _SAMPLERS["small"](rng)), e, c, ("converge",))
    b.finish_at = 4 if kind == "below" else None
    return b.done()


def _gen_max_it(rng, i):
    b = _Builder("max_iterations", start_pose(rng), max_iterations=[0, 1, 3][i % 3])
    for k in range(5):
        targeted_step(b, rng, "large" if (i + k) % 3 == 0 else "small", k)
    return b.done()


def _gen_after(rng, i):
    """the loop ends by c == 0, by a singular system or by convergence (errors 0.001 apart from the start on); then one more set"""
    kind = i % 3
    b = _Builder("after_finished", start_pose(rng), it_weight_gradient=0.0)
    if kind == 2:
        b.step(spd(rng), make_xi(rng, 0.01), 10, 1000, ("converge",))  # err 0.01 against the zeros of prev: ends at once
        b.finish_at = 0
    else:
        targeted_step(b, rng, "small", 0)
        H = spd(rng) if kind == 0 else diag([0] * 6)
        b.push(H, [1, 2, 3, 4, 5, 6], 5, 0 if kind == 0 else 77, ("c_zero" if kind == 0 else "singular",))
    for k in range(2):
        targeted_step(b, rng, "large" if k else "small", 2 + k)
    return b.done()


_PLAN = [  # (generator, sequences)
    (_gen_small, 400), (_gen_theta_zero, 40), (_gen_quarter_exact, 24), (_gen_quarter_below, 48), (_gen_quarter_above, 120),
    (_gen_large, 500), (_gen_huge, 40), (_gen_axis, 60), (_gen_signs, 128), (_gen_far, 150), (_gen_history, 300),
    (lambda r, i: _gen_c_zero(r, i, True), 20), (lambda r, i: _gen_c_zero(r, i, False), 40), (_gen_c_values, 60), (_gen_c_high, 40),
    (_gen_e_high, 40), (lambda r, i: _gen_singular(r, i, True), 24), (lambda r, i: _gen_singular(r, i, False), 72), (_gen_zero_h, 42),
    (lambda r, i: _gen_pivot(r, i, "first"), 60), (lambda r, i: _gen_pivot(r, i, "later"), 60), (lambda r, i: _gen_pivot(r, i, "tie"), 40),
    (_gen_large_sums, 150), (lambda r, i: _gen_converge(r, i, "equal"), 32), (lambda r, i: _gen_converge(r, i, "below"), 32),
    (lambda r, i: _gen_converge(r, i, "one_fails"), 40), (_gen_max_it, 60), (_gen_after, 42),
]


@functools.lru_cache(maxsize=None)
def _table():
    kept, dropped = [], {}
    for n, (gen, count) in enumerate(_PLAN):
        rng = np.random.default_rng(7000 + n)
        for i in range(count):
            s = gen(rng, i)
            if s.finite():
                kept.append(s)
            else:
                dropped[s.cls] = dropped.get(s.cls, 0) + 1
    return kept, dropped


def sequences():
    """every kept sequence, in the order of the plan"""
    return _table()[0]


def dropped():
    """class -> sequences dropped because an expected pose was not finite"""
    return dict(_table()[1])


def generated():
    return sum(count for _, count in _PLAN)


def subset(per_class=10):
    """the first `per_class` sequences of every class: a few hundred, every class among them (the routes of the C ABI run these)"""
    seen, out = {}, []
    for s in sequences():
        if seen.get(s.cls, 0) < per_class:
            seen[s.cls] = seen.get(s.cls, 0) + 1
            out.append(s)
    return out


# ---- the case file of tests/cpp/gn_units.hip: a header of eight int32 (magic, sequences, updates in all, MAX_UPDATES, 0 ..), then per
# sequence 20 words of start state (T[16], max_iterations, it_weight_gradient, epsilon, updates), then per sequence and update slot
# (MAX_UPDATES each, unused ones zero) 32 int64 slot totals (29 .. 31: padding), 44 int64 words, 24 words of expected state (23 + pad)
MAGIC = 0x474E3031


def write_case_file(path, seqs):
    n = len(seqs)
    start = np.zeros((n, 20), dtype=np.uint32)
    slots = np.zeros((n, MAX_UPDATES, N_SLOTS), dtype=np.int64)
    words = np.zeros((n, MAX_UPDATES, N_WORDS), dtype=np.int64)
    expect = np.zeros((n, MAX_UPDATES, 24), dtype=np.uint32)
    for i, s in enumerate(seqs):
        start[i, :16] = s.T0.view(np.uint32)
        start[i, 16] = np.uint32(s.max_iterations)
        start[i, 17], start[i, 18] = s.it_weight_gradient.view(np.uint32), s.epsilon.view(np.uint32)
        start[i, 19] = len(s.updates)
        for k, u in enumerate(s.updates):
            slots[i, k, :N_TERMS] = u.slots
            words[i, k] = u.words
            expect[i, k, :STATE_WORDS] = u.after
    total = sum(len(s.updates) for s in seqs)
    with open(path, "wb") as f:
        f.write(np.array([MAGIC, n, total, MAX_UPDATES, 0, 0, 0, 0], dtype=np.int32).tobytes())
        for a in (start, slots, words, expect):
            f.write(a.tobytes())
    return total
