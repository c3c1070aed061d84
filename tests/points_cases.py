"""The case table of the device unit tests of reg_points.h and reg_exchange.h (tests/cpp/points_units.hip, exchange_units.hip):
inputs that no scan chose, all from fixed seeds, no GPU (tests/test_points_cases_host.py holds the table to its claims;
tests/test_gpu_points_units.py runs the programs and derives every `checked` count from here).

A lane's input is a `Gathered`: the transformed point minus the centre (qx, qy, qz), the voxel's raw entry and its six neighbours'
and `ok`, as 12 uint32 (GATHERED_W).  point_terms() below restates registration.cu:224-250 on int64 with the reference's int32
wraps; the programs hold the device functions to the same restatement written in C++.

  1. gradient_lists(), point_terms_cases()      central_gradient and point_terms over their edges
  2. patterns()                                  synthetic workgroups for the two routes of the sums, classes (a) .. (f); every
                                                 pattern runs twice in one launch, the second pass on the next pattern's data (g)
  3. gather_windows()                            windows A .. E of reg_cases.py, a cloud and a sequence of poses each, J, value
                                                 and mask per point from the oracle
  4. EXCHANGE_*                                  how many cases exchange_units.hip generates from its own seeds
"""
import functools
import struct

import numpy as np

import oracle_lib as O
import reg_cases as R

MAGIC = 0x50543031
GATHERED_W = 12  # qx qy qz cur xn xl yn yl zn zl ok pad
REG_THREADS, WAVES, REG_SLOTS, REG_TERMS, MF_AUX = 512, 8, 32, 29, 8
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
BIAS = 0x00808080


def wrap32(x):
    return ((np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def entry(value, weight):
    return (np.asarray(value, dtype=np.int64) & 0xffff) | ((np.asarray(weight, dtype=np.int64) & 0xffff) << 16)


def entry_value(raw):
    v = np.asarray(raw, dtype=np.int64) & 0xffff
    return np.where(v >= 32768, v - 65536, v)


def central_gradient(nxt, last):
    """registration.cu:233-246: both neighbours observed and not of strictly opposite sign; C division"""
    nv, lv = entry_value(nxt), entry_value(last)
    ok = ((np.asarray(nxt, dtype=np.int64) >> 16) != 0) & ((np.asarray(last, dtype=np.int64) >> 16) != 0)
    ok &= ~(((nv > 0) & (lv < 0)) | ((nv < 0) & (lv > 0)))
    d = nv - lv
    return np.where(ok, np.sign(d) * (np.abs(d) // 2), 0)


def point_terms(G):
    """(J [n, 6], v [n], used [n]) as int64 of Gathered rows [n, 12]: registration.cu:217-250"""
    G = np.asarray(G, dtype=np.uint32).astype(np.int64).reshape(-1, GATHERED_W)
    q = wrap32(G[:, 0:3])
    used = (G[:, 10] != 0) & ((G[:, 3] >> 16) != 0)
    g = np.stack([central_gradient(G[:, 4 + 2 * k], G[:, 5 + 2 * k]) for k in range(3)], axis=1) * used[:, None]
    J = np.zeros((len(G), 6), dtype=np.int64)
    J[:, 0] = wrap32(wrap32(q[:, 1] * g[:, 2]) - wrap32(q[:, 2] * g[:, 1]))
    J[:, 1] = wrap32(wrap32(q[:, 2] * g[:, 0]) - wrap32(q[:, 0] * g[:, 2]))
    J[:, 2] = wrap32(wrap32(q[:, 0] * g[:, 1]) - wrap32(q[:, 1] * g[:, 0]))
    J[:, 3:6] = g
    return J, entry_value(G[:, 3]) * used, used.astype(np.int64)


# ------------------------------------------------------------------------------------------------ 1. the point terms
GRADIENT_VALUES = [-32768, -32767, -1, 0, 1, 2, 32766, 32767, -2, 3, -3, 16384, -16385]
GRADIENT_WEIGHTS = [0, 1, -1, -32768]


def gradient_lists():
    return np.asarray(GRADIENT_VALUES, dtype=np.int32), np.asarray(GRADIENT_WEIGHTS, dtype=np.int32)


def gradient_cases():
    return (len(GRADIENT_VALUES) * len(GRADIENT_WEIGHTS)) ** 2


def gradient_entries(g):
    """raw entries (next, last) whose central gradient is g, -16383 <= g <= 16384"""
    g = int(g)
    assert -16383 <= g <= 16384
    if g == 16384:
        nv, lv = 0, -32768
    elif g >= 0:
        nv, lv = 2 * g, 0
    else:
        nv, lv = 0, -2 * g
    return int(entry(nv, 1)), int(entry(lv, 1))


Q_VALUES = [0, 1, -1, 65535, -65535, INT32_MIN, INT32_MAX]
V_VALUES = [-32768, -1, 0, 32767]
# gradients (gx, gy, gz): along one axis only, and along all three
GRADIENT_SETS = [(1, 0, 0), (0, -1, 0), (0, 0, 16384), (-16383, 0, 0), (0, 16383, 0), (1, 1, 1), (16384, -16383, 16383), (-1, 12345, -2)]
STATES = ["counts", "ok_false", "cur_unobserved"]


@functools.lru_cache(maxsize=None)
def point_terms_cases():
    """Gathered rows [n, 12]: every q in Q_VALUES^3 x v x gradients x (counts, ok false, cur unobserved)"""
    q = np.array(np.meshgrid(Q_VALUES, Q_VALUES, Q_VALUES, indexing="ij"), dtype=np.int64).reshape(3, -1).T
    rows = []
    for state in STATES:
        for v in V_VALUES:
            for gs in GRADIENT_SETS:
                G = np.zeros((len(q), GATHERED_W), dtype=np.int64)
                G[:, 0:3] = q & 0xffffffff
                G[:, 3] = entry(v, 0 if state == "cur_unobserved" else -7)
                for k in range(3):
                    G[:, 4 + 2 * k], G[:, 5 + 2 * k] = gradient_entries(gs[k])
                G[:, 10] = 0 if state == "ok_false" else 1
                rows.append(G)
    return np.concatenate(rows).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ 2. the sums
def _byte_values():
    out = []
    for shift in (0, 8, 16):
        out += [0x7f << shift, 0x80 << shift, 0xff << shift, 0x100 << shift]
    return out


J_VALUES = ([0, 1, -1] + _byte_values() + [BIAS, -BIAS, 0x7f7f7f7f, 0x7f7f7f80, 0x7f7f7f81, -0x7f7f7f7f, -0x7f7f7f80, -0x7f7f7f81,
                                           INT32_MAX, INT32_MIN])
ROW_GRADIENTS = [16384, -16383, 1, -1, 12345, -2]
PATTERN_CLASSES = ["a_same", "b_single", "c_alternate", "d_random", "e_partial", "f_waves"]


class Pattern:
    def __init__(self, cls, name, G, waves=WAVES):
        self.cls, self.name, self.waves = cls, name, int(waves)
        self.G = np.asarray(G, dtype=np.int64).astype(np.uint32).reshape(REG_THREADS, GATHERED_W)

    def terms(self):
        """(J, v, used) of the lanes of the waves that call the sums"""
        return point_terms(self.G[:64 * self.waves])


def zero_lane(v=0):
    G = np.zeros(GATHERED_W, dtype=np.int64)
    G[3] = entry(v, 1)
    G[10] = 1
    return G


def cross_lane(axis, a, b, v):
    """a lane with a unit gradient along `axis`: J[(axis + 1) % 3] = a, J[(axis + 2) % 3] = b, J[3 + axis] = 1, value v"""
    G = zero_lane(v)
    G[(axis + 2) % 3] = int(a) & 0xffffffff
    G[(axis + 1) % 3] = (-int(b)) & 0xffffffff
    G[4 + 2 * axis], G[5 + 2 * axis] = gradient_entries(1)
    return G


def gradient_lane(axis, g, v):
    G = zero_lane(v)
    G[4 + 2 * axis], G[5 + 2 * axis] = gradient_entries(g)
    return G


def random_lanes(rng, n):
    """full-range q, raw entries over all of int16 (half of them same-sign extremes), weights of any sign, a tenth unobserved"""
    G = np.zeros((n, GATHERED_W), dtype=np.int64)
    G[:, 0:3] = rng.integers(INT32_MIN, INT32_MAX + 1, (n, 3)) & 0xffffffff
    value = rng.integers(-32768, 32768, (n, 7))
    sign = np.where(rng.random((n, 1)) < 0.5, 1, -1)
    ext = np.where(rng.random((n, 7)) < 0.5, 32767, 1)
    value = np.where(rng.random((n, 7)) < 0.5, np.where(sign > 0, ext, -ext - 1), value)
    weight = rng.integers(-32768, 32768, (n, 7))
    weight[rng.random((n, 7)) < 0.1] = 0
    G[:, 3:10] = entry(value, weight)
    G[:, 10] = rng.random(n) < 0.9
    return G


@functools.lru_cache(maxsize=None)
def patterns():
    out = []
    # (a) all 64 lanes of a wave carry the same value; wave w puts it into rows (w + 1) % 3 and (w + 2) % 3
    for val in J_VALUES:
        for v in (-32768, 32767):
            G = np.stack([cross_lane(t // 64 % 3, val, val, v) for t in range(REG_THREADS)])
            out.append(Pattern("a_same", f"{val:#x} v {v}", G))
    # (b) one lane of every wave carries a value, for every lane position and every row of J
    for row in range(6):
        for lane in range(64):
            G = np.tile(zero_lane(), (REG_THREADS, 1))
            for w in range(WAVES):
                v = 32767 if (lane + w) % 2 else -32768
                if row < 3:
                    val = J_VALUES[1:][(lane * 6 + row + 7 * w) % (len(J_VALUES) - 1)]
                    G[64 * w + lane] = cross_lane((row + 2) % 3, val, 0, v)
                else:
                    G[64 * w + lane] = gradient_lane(row - 3, ROW_GRADIENTS[(lane + w) % len(ROW_GRADIENTS)], v)
            out.append(Pattern("b_single", f"row {row} lane {lane}", G))
    # (c) lanes alternate between the extremes of opposite sign
    for hi, lo in ((INT32_MAX, INT32_MIN), (0x7f7f7f7f, -0x7f7f7f7f), (0x7f7f7f80, -0x7f7f7f80), (BIAS, -BIAS)):
        G = np.stack([cross_lane(t // 64 % 3, hi if t % 2 else lo, lo if t % 2 else hi, 32767 if t % 2 else -32768) for t in range(REG_THREADS)])
        out.append(Pattern("c_alternate", f"{hi:#x}", G))
    # (d) random values of the full range
    rng = np.random.default_rng(20261)
    for i in range(8):
        out.append(Pattern("d_random", str(i), random_lanes(rng, REG_THREADS)))
    # (e) waves with 0, 1, 63 and 64 valid points at the low and at the high end; the other lanes hold data and ok == false
    for n_valid in (0, 1, 63, 64):
        for end in ("low", "high"):
            G = random_lanes(rng, REG_THREADS)
            lane = np.arange(REG_THREADS) % 64
            G[:, 10] = (lane < n_valid) if end == "low" else (lane >= 64 - n_valid)
            out.append(Pattern("e_partial", f"{n_valid} {end}", G))
    # (f) only waves 0 .. w - 1 call the sums
    for w in (1, 2, 4, 8):
        out.append(Pattern("f_waves", str(w), random_lanes(rng, REG_THREADS), waves=w))
    return out


PASSES = 2  # (g): pass 1 of pattern p runs the data of pattern (p + 1) % n with p's waves


def limbs(J):
    """the four signed byte limbs of J with J = s0 + 256 s1 + 65536 s2 + 2^24 s3 + 0x808080"""
    u = (np.asarray(J, dtype=np.int64) & 0xffffffff) ^ BIAS
    b = np.stack([(u >> (8 * k)) & 0xff for k in range(4)], axis=-1)
    return np.where(b >= 128, b - 256, b)


def exact_totals(p):
    """the 29 totals of a pattern as Python integers (no wrap)"""
    J, v, used = (a.astype(object) for a in p.terms())
    t = [int((J[:, i] * J[:, j]).sum()) for i in range(6) for j in range(i, 6)]
    t += [int((J[:, i] * v).sum()) for i in range(6)]
    return t + [int(abs(v).sum()), int(used.sum())]


# ------------------------------------------------------------------------------------------------ 3. the gathers
GATHER_POINTS = 384
# "nudged": pose 0 moved by 0.6 voxels along z (at 65 m from the origin the case's own poses are more than a voxel apart)
STEP_NAMES = ["pose0", "nudged", "pose1", "pose0", "out", "pose0", "pose2"]


def int_transform(T):
    """M[12] column-major 3x4 and the centre as make_int_transform computes them from the column-major float pose"""
    Tc = O.colmajor(T)
    M = (Tc * np.float32(32768)).astype(np.int32)
    out = np.zeros(16, dtype=np.int32)
    for j in range(4):
        out[3 * j:3 * j + 3] = M[4 * j:4 * j + 3]
    out[12:15] = Tc[12:15].astype(np.int32)
    return out


class GatherWindow:
    def __init__(self, cid):
        c = R.case(cid)
        self.id, self.case, self.res, self.om = cid, c, c.res, c.om
        self.points = c.cloud(GATHER_POINTS)
        out = np.array(c.poses[0], dtype=np.float32)
        out[0, 3] += float((int(c.om.size[0]) + 4) * c.res)  # the whole window's width along x
        nudged = np.array(c.poses[0], dtype=np.float32)
        nudged[2, 3] += np.float32(0.6 * c.res)
        self.poses = [c.poses[0], nudged, c.poses[1], c.poses[0], out, c.poses[0], c.poses[2]]
        self.expect = np.zeros((len(self.poses), GATHER_POINTS, 8), dtype=np.int32)
        self.voxel = np.zeros((len(self.poses), GATHER_POINTS, 3), dtype=np.int64)
        self.admitted = np.zeros((len(self.poses), GATHER_POINTS), dtype=bool)
        observed = c.all_observed()
        for s, T in enumerate(self.poses):
            J, val, mask = O.calc_jacobis(c.om, T, self.points, c.res)
            assert (J >= INT32_MIN).all() and (J <= INT32_MAX).all()
            self.expect[s, :, :6], self.expect[s, :, 6], self.expect[s, :, 7] = J, val, mask
            self.admitted[s] = O.calc_jacobis(observed, T, self.points, c.res)[2] != 0
            self.voxel[s] = R.voxel_of(R.transform_exact(T, self.points)[0], c.res)


@functools.lru_cache(maxsize=None)
def gather_windows():
    return [GatherWindow(cid) for cid in R.IDS]


# ------------------------------------------------------------------------------------------------ 4. the counted exchange
# exchange_units.hip draws its totals and presets from mix64 of (line, case, call, slot); what Python needs are the counts
EXCHANGE_TOTALS = ["random", "halves_all_ones", "zero", "single_slot"]
EXCHANGE_PRESETS = ["zero", "all_ones", "low56_full", "count_ff", "low56_minus_2_37", "low56_minus_2_36", "random"]
EXCHANGE_CASES = len(EXCHANGE_TOTALS) * len(EXCHANGE_PRESETS)
COLLECT_EXCHANGES, PEER_EXCHANGES, PEER_WORLDS = 4, 4, (1, 2, 8)


def expected_counts():
    """line of a unit program -> the number of cases it must report"""
    pats, wins = patterns(), gather_windows()
    per_form = sum(len(w.poses) * GATHER_POINTS for w in wins)
    n = len(pats) * PASSES
    points = {"central_gradient": gradient_cases(), "point_terms": len(point_terms_cases()),
              "sums int64": n * REG_TERMS, "sums mfma": n * REG_TERMS, "mfma_finalize zeroes": n * (REG_SLOTS + MF_AUX),
              "gather_point": per_form, "gather_point<true>": per_form, "gather_point_loop": per_form}
    exchange = {"counted_add/poll/fold": EXCHANGE_CASES * REG_SLOTS, "counted_publish<false>": EXCHANGE_CASES * 2 * REG_SLOTS,
                "counted_collect": EXCHANGE_CASES * COLLECT_EXCHANGES * REG_SLOTS,
                "peer_exchange": EXCHANGE_CASES * len(PEER_WORLDS) * PEER_EXCHANGES * REG_SLOTS, "counted_poll gives up": 2}
    return points, exchange


def write_case_file(path):
    vals, weights = gradient_lists()
    pt, pats, wins = point_terms_cases(), patterns(), gather_windows()
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", MAGIC, len(vals), len(weights), len(pt), len(pats), len(wins), GATHER_POINTS, len(STEP_NAMES)))
        f.write(vals.tobytes())
        f.write(weights.tobytes())
        f.write(np.ascontiguousarray(pt, dtype=np.uint32).tobytes())
        f.write(np.asarray([p.waves for p in pats], dtype=np.int32).tobytes())
        f.write(np.stack([p.G for p in pats]).astype(np.uint32).tobytes())
        for w in wins:
            om = w.om
            f.write(struct.pack("<12i", *(int(v) for v in om.size), *(int(v) for v in om.pos), *(int(v) for v in om.offset), w.res, om.n_vox, 0))
            f.write(np.ascontiguousarray(om.data, dtype=np.uint32).tobytes())
            f.write(np.ascontiguousarray(w.points, dtype=np.int32).tobytes())
            f.write(np.stack([int_transform(T) for T in w.poses]).astype(np.int32).tobytes())
            f.write(np.ascontiguousarray(w.expect, dtype=np.int32).tobytes())
