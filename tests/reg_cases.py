"""The case table of the registration route tests: windows that are shifted, wrapped and tiny, clouds with a named edge set, three
poses per case -- all from fixed seeds, no GPU, no fixtures (tests/test_reg_cases_host.py proves on the oracle alone that every
case exercises what it claims; tests/test_gpu_reg_routes.py runs every device route on them).

Every registration route computes voxel = q / res (C division), admits |voxel - pos| <= size/2 - 1 per axis and reads the voxel
and its six neighbours at the ring coordinate (x - pos + offset + size) % size.  The windows below are the smallest on which those
three steps differ from the construction window (pos = 0, offset = size/2):

    id  size       pos (voxels)         offset       res
    A   33x37x21   (40, -25, 7)         (5, 36, 0)   50   offset 0, size-1 and interior on one map each; pos of both signs
    B   3x3x3      (-2, 1, 0)           (2, 0, 1)    50   lim = size/2 - 1 = 0: one voxel admitted, every neighbour is a ring wrap
    C   33x33x33   (0, 0, 0)            (0, 16, 32)  7    non-power-of-two FastDiv; truncation makes voxel 0 double width
    D   65x65x65   (65500, -65500, 0)   (1, 2, 3)    1    the window next to the +-65 536 mm limit of a transformed coordinate
    E   65x65x65   after three shifts   --           50   pos / offset as LocalMap.shift (and TSDFMapping.shift_map) leave them

A transformed coordinate is a wrapped int32 divided by 32768: it lies in [-65 536, 65 535] mm whatever the point and the pose.
Window D reaches 65 532 mm, so every voxel of it can be reached; a point 131 072 mm further out lands in it as well (the
`wrap_*` classes below), which is what the case is for.  ws_map_create refuses a MAP resolution below 2 mm (the ray step of the
TSDF update is resolution / 2); the registration takes its own resolution argument, so D's device map is created with 2 and
registered with 1.

A-D hold random raw entries (the recipe of test_loop_sums_on_a_map_of_arbitrary_entries: values over all of int16, half of them
same-sign extremes next to each other, weights of any sign, a fifth unobserved); B's seed is the first whose single admitted
voxel is observed and has a gradient along every axis.
E is a real TSDF: one update with a 16 x 128 scan at pos 0, then three shifts, mirrored on the host by LocalMap.shift.  The
scan observes a sixth of the window, so three quarters of E's body are drawn inside observed voxels.

Poses: identity; S.perturbation(0.3 res, 0.2 res, 0, 1.0); and the 54 m pre-transform of the random-entry test scaled by
res / 2000 (3 degrees about z).  Two departures, both forced by conditions the host test holds the table to:
  * under the two non-identity poses a cloud around a window far from the origin (D: a degree at 65 m is 1.1 m) leaves the window,
    so every cloud carries pre-images of points inside the window for both poses (`pose1_*`, `pose2_*`), some of them 131 072 mm
    further out along one axis so that the int32 transform wraps for them;
  * a cross-product term beyond +-0x7f7f7f80 needs |q - center| * |gradient| near 2^31, i.e. a pose whose translation is about
    65 m in two axes when the window is 2 m from the origin: A's third pose keeps the recipe's x and rotation and has
    y = 65 000 mm, z = -65 250 mm (both times 32768 still fit int32), and its first pre-images sit in voxels whose y and z
    gradients are both +-16383.
"""
import functools

import numpy as np

import oracle_lib as O
from warpsense_amd import synthetic as S

WRAP_MM = 131072  # 2^32 / 32768: two points this far apart along an axis transform to the same coordinate
REACH_MM = 65536

WINDOWS = {
    "A": dict(name="shifted", size=(33, 37, 21), pos=(40, -25, 7), offset=(5, 36, 0), res=50, seed=101),
    "B": dict(name="tiny", size=(3, 3, 3), pos=(-2, 1, 0), offset=(2, 0, 1), res=50, seed=132),
    "C": dict(name="res7", size=(33, 33, 33), pos=(0, 0, 0), offset=(0, 16, 32), res=7, seed=103),
    "D": dict(name="res1_reach", size=(65, 65, 65), pos=(65500, -65500, 0), offset=(1, 2, 3), res=1, seed=104),
    "E": dict(name="after_shift", size=(65, 65, 65), res=50, seed=105),
}
IDS = list(WINDOWS)

# window E: the scan, and the shifts as voxel steps (shift_map takes the new position: the running sum)
E_TAU, E_MAX_WEIGHT = 1000, 640
E_SCAN = dict(rings=16, azimuths=128, half_extents_mm=(1300.0, 1200.0, 900.0), seed=31)
E_SHIFTS = [(7, -5, 3), (-9, 0, 0), (0, 11, -4)]

# point counts, chosen by the code's own edges
COUNTS_ALL = [1, 65, 513, 1025, 3075]      # a wave; the batch workgroup; first streamed point of batch variant 1; ragged second trip
COUNTS_HOST = [1, 63, 64, 65, 511, 512, 513, 1025, 3075]
COUNTS_SWITCH = [131072, 131073]           # matrix cores / v_mad_i64 switch of the resident kernels (window A)
COUNTS_THIRD_STAGE = [262144, 262145]      # the first point of the third stage of accumulate_points (window A)
BODY_POINTS = 4096
LOOP_LIMITS = (1, 2, 6)
LOOP_LIMITS_LARGE = (1, 3)                 # from 131 072 points up
# On the random maps a Gauss-Newton step hardly moves the pose (h is of the order 10^15 per point), so a loop of 6 iterations is
# cut; with the first 24 points of C's cloud the normal equations are bad enough that the fourth iteration finds no point at all.
# Found by search; the host test holds it.
LOOP_THAT_EMPTIES = ("C", 24)
IT_WEIGHT_GRADIENT, EPSILON = 0.1, 0.03


def e_positions():
    """the window positions of E after each shift"""
    return np.cumsum(np.asarray(E_SHIFTS, dtype=np.int64), axis=0)


def raw_entries(size, rng):
    """random raw entries that use the whole width of the arithmetic (test_loop_sums_on_a_map_of_arbitrary_entries)"""
    n_vox = int(size[0]) * int(size[1]) * int(size[2])
    value = rng.integers(-32768, 32768, n_vox).astype(np.int64)
    ext = np.where(rng.random(n_vox) < 0.5, 32767, 1)
    value = np.where(rng.random(n_vox) < 0.5, np.where((np.arange(n_vox) // (int(size[1]) * int(size[2]))) % 2 == 0, ext, -ext - 1), value)
    weight = rng.integers(-32768, 32768, n_vox).astype(np.int64)
    weight[rng.random(n_vox) < 0.2] = 0
    return ((value & 0xffff) | ((weight & 0xffff) << 16)).astype(np.uint32)


def voxel_of(q_mm, res):
    """q / res as C divides: truncation toward zero"""
    q = np.asarray(q_mm, dtype=np.int64)
    return (np.sign(q) * (np.abs(q) // int(res))).astype(np.int64)


def voxel_centre(b, res):
    """a millimetre coordinate in the middle of voxel b (voxel 0 spans -(res-1) .. res-1, a negative voxel b*res-(res-1) .. b*res)"""
    b = np.asarray(b, dtype=np.int64)
    return np.where(b > 0, b * res + res // 2, np.where(b < 0, b * res - res // 2, 0)).astype(np.int64)


def transform_exact(T, p):
    """(wrapped int32 coordinate, unwrapped int64 coordinate) of cu_transform_point: M = (int)(T * 32768), sum, / 32768"""
    M = (np.asarray(T, dtype=np.float32) * np.float32(32768)).astype(np.int32).astype(np.int64)
    p = np.asarray(p, dtype=np.int64).reshape(-1, 3)
    acc = p @ M[:3, :3].T + M[:3, 3]
    wrapped = ((acc + 2 ** 31) % 2 ** 32) - 2 ** 31
    trunc = lambda v: np.sign(v) * (np.abs(v) // 32768)
    return trunc(wrapped), trunc(acc)


def world_view(om):
    """the window's raw entries in world order: W[i, j, k] is voxel pos - size/2 + (i, j, k)"""
    size, pos, off = (np.asarray(v, dtype=np.int64) for v in (om.size, om.pos, om.offset))
    ring = [(np.arange(size[k]) - size[k] // 2 + off[k] + size[k]) % size[k] for k in range(3)]
    return om.data.reshape(tuple(int(s) for s in size))[np.ix_(*ring)], pos - size // 2


def _gradient(value, weight, axis):
    """the central gradient of the registration at interior voxels along `axis` (0 elsewhere)"""
    nv, lv = np.roll(value, -1, axis), np.roll(value, 1, axis)
    nw, lw = np.roll(weight, -1, axis), np.roll(weight, 1, axis)
    ok = (nw != 0) & (lw != 0) & ~(((nv > 0) & (lv < 0)) | ((nv < 0) & (lv > 0)))
    d = nv - lv
    return np.where(ok, np.sign(d) * (np.abs(d) // 2), 0)


class Case:
    def __init__(self, cid, om, res, poses, edge, classes, body):
        self.id, self.om, self.res, self.poses = cid, om, int(res), poses
        self.name = WINDOWS[cid]["name"]
        self.edge, self.classes, self.body = edge, classes, body  # classes: name -> indices into edge
        self.half = (om.size // 2).astype(np.int64)
        self.map_resolution = max(self.res, 2)  # what ws_map_create admits; the registration's own argument is self.res

    def cloud(self, n):
        """the first n points of: the edge set, then draws with replacement from the body"""
        n = int(n)
        rng = np.random.default_rng(WINDOWS[self.id]["seed"] * 1000003 + n)
        draws = self.body[rng.integers(0, len(self.body), max(n - len(self.edge), 0))]
        return np.ascontiguousarray(np.concatenate([self.edge, draws])[:n], dtype=np.int32)

    def all_observed(self):
        """a copy of the map whose every voxel is observed: the mask of calc_jacobis on it is the admission test alone"""
        m = self.om.copy()
        m.data[(m.data >> 16) == 0] |= np.uint32(0x10000)
        return m

    def ring_coordinate(self, b):
        """the ring coordinate per axis of world voxel b, from OracleMap.index"""
        idx = self.om.index(int(b[0]), int(b[1]), int(b[2]))
        return np.array(np.unravel_index(idx, tuple(int(s) for s in self.om.size)), dtype=np.int64)

    def batch_poses(self):
        """k = 7 start poses: the case's three and four perturbations around the second"""
        r = float(self.res)
        extra = [S.perturbation(0.3 * r + dx * r, 0.2 * r + dy * r, dz * r, 1.0 + rz)
                 for dx, dy, dz, rz in ((0.2, -0.1, 0.1, 0.5), (-0.4, 0.3, 0.0, -0.7), (0.05, 0.05, -0.2, 0.1), (-0.1, -0.3, 0.15, -1.5))]
        return np.stack(list(self.poses) + extra).astype(np.float32)


def _window_e():
    import warpsense_amd as W
    size, res = WINDOWS["E"]["size"], WINDOWS["E"]["res"]
    oa = O.OracleMap(size, E_TAU, 0)
    on = oa.copy()
    O.update_tsdf(oa, on, e_scan(), (0, 0, 0), (0, 0, 32768), E_TAU, E_MAX_WEIGHT, res)
    lm = W.LocalMap(*size, E_TAU, 0)
    lm.data[:] = oa.data
    for new_pos in e_positions():
        lm.shift(new_pos)
    return O.OracleMap(size, 0, 0, pos=lm.pos.copy(), offset=lm.offset.copy(), data=lm.data.copy())


def e_scan():
    return S.os1_128_scan(**E_SCAN)


def _poses(cid, res):
    r = float(res)
    t3 = (40_000 * r / 2000, -30_000 * r / 2000, 20_000 * r / 2000)
    if cid == "A":
        t3 = (t3[0], 65_000.0, -65_250.0)
    return [np.eye(4, dtype=np.float32), S.perturbation(0.3 * r, 0.2 * r, 0, 1.0), S.perturbation(*t3, 3.0)]


def _preimages(T, targets_mm, shift_units):
    """points that the pose T takes to targets_mm + WRAP_MM * shift_units before the int32 wrap, i.e. to (about) targets_mm after it"""
    T = np.asarray(T, dtype=np.float64)
    want = np.asarray(targets_mm, dtype=np.float64) + WRAP_MM * np.asarray(shift_units, dtype=np.float64) - T[:3, 3]
    return np.rint(want @ np.linalg.inv(T[:3, :3]).T).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(cid):
    spec = WINDOWS[cid]
    res = spec["res"]
    rng = np.random.default_rng(spec["seed"])
    if cid == "E":
        om = _window_e()
    else:
        om = O.OracleMap(spec["size"], 0, 0, pos=spec["pos"], offset=spec["offset"], data=raw_entries(spec["size"], rng))
        if cid == "B":
            i = om.index(*spec["pos"])
            if (om.data[i] >> 16) == 0:
                om.data[i] |= np.uint32(0x10000)
    size, pos = om.size.astype(np.int64), om.pos.astype(np.int64)
    half, lim = size // 2, size // 2 - 1
    Wd, lo = world_view(om)
    weight = (Wd >> 16).astype(np.uint16).astype(np.int16).astype(np.int64)
    value = (Wd & 0xffff).astype(np.uint16).astype(np.int16).astype(np.int64)
    observed = weight != 0
    poses = _poses(cid, res)

    def admitted_voxel(fixed=None, want_observed=True):
        """a random admitted voxel (axis -> coordinate in `fixed` pinned), observed if one of 200 draws is"""
        b = None
        for _ in range(200):
            b = pos + rng.integers(-lim, lim + 1)
            for k, v in (fixed or {}).items():
                b[k] = v
            if not want_observed or observed[tuple(b - lo)]:
                break
        return b

    def inside(b):
        """a random millimetre point inside voxel b"""
        c = voxel_centre(b, res)
        j = (res - 1) // 2
        return c + (rng.integers(-j, j + 1, 3) if j else 0)

    pts, classes = [], {}

    def add(name, p):
        classes.setdefault(name, []).append(len(pts))
        pts.append(np.asarray(p, dtype=np.int64))

    # the first point of every cloud: counted under the identity (n = 1 is not an empty sum)
    add("centre", inside(admitted_voxel({k: pos[k] for k in range(3)} if cid == "B" else None)))
    # pre-images for the two other poses; `wide` of them wrap (131 072 mm further out along one axis, either side)
    late = []
    for pi in (1, 2):
        targets = []
        if cid == "A" and pi == 2:
            # voxels whose y and z gradients are both +-16383: with |q - center| ~ 65 m in y and z the first cross term nears 2^31
            gy, gz = _gradient(value, weight, 1), _gradient(value, weight, 2)
            inner = np.zeros(Wd.shape, dtype=bool)
            inner[1:-1, 1:-1, 1:-1] = True
            hot = np.argwhere(inner & observed & (np.abs(gy) == 16383) & (np.abs(gz) == 16383))
            targets += [voxel_centre(h + lo, res) for h in hot[:40]]
        while len(targets) < 56:
            targets.append(voxel_centre(admitted_voxel(), res))
        for i, t in enumerate(targets):
            unit = np.zeros(3)
            if i % 3 == 2 and not (cid == "A" and pi == 2 and i < 40):
                unit[i % 9 // 3] = 1 if i % 2 else -1
            p = _preimages(poses[pi], t, unit)
            name = f"pose{pi}_" + ("wrapped" if unit.any() else "plain")
            if i < 8:  # eight per pose right behind the first point: a cloud of 65 points has them
                add(name, p)
            else:
                late.append((name, p))
    # the named edge classes under the identity, per axis and side
    for k in range(3):
        for side, tag in ((-1, "lo"), (1, "hi")):
            for _ in range(2):
                add(f"last_{k}{tag}", inside(admitted_voxel({k: pos[k] + side * lim[k]})))
                add(f"refused_{k}{tag}", inside(admitted_voxel({k: pos[k] + side * half[k]}, want_observed=False)))
        for ring, tag in ((0, "ring0"), (size[k] - 1, "ringmax")):
            d = (ring - om.offset[k]) % size[k]
            d = d - size[k] if d > half[k] else d  # the world voxel pos + d has that ring coordinate
            for _ in range(2):
                add(f"{tag}_{k}", inside(admitted_voxel({k: pos[k] + d}, want_observed=abs(d) <= lim[k])))
        # a point 131 072 mm out along this axis: the identity wraps it into the window
        for side in (-1, 1):
            p = inside(admitted_voxel())
            p[k] += side * WRAP_MM
            add(f"wrap_identity_{k}", p)
        if cid == "C":
            for q in (0, 1, -1, res - 1, -(res - 1), res, -res, res + 1, -(res + 1)):
                p = inside(admitted_voxel())
                p[k] = q
                add(f"q{q:+d}_{k}", p)
    for n, q in late:
        add(n, q)
    edge = np.stack(pts).astype(np.int32)
    # the body: random points over the window and a band of 2 res around it (never beyond the reach of a coordinate)
    lo_mm, hi_mm = (pos - half) * res - (res - 1) - 2 * res, (pos + half) * res + (res - 1) + 2 * res
    lo_mm, hi_mm = np.maximum(lo_mm, -REACH_MM + 1), np.minimum(hi_mm, REACH_MM - 1)
    body = rng.integers(lo_mm, hi_mm + 1, (BODY_POINTS, 3)).astype(np.int32)
    if cid == "E":
        # one scan of 2048 rays observes a sixth of the window: three quarters of E's body lie in observed voxels, so that the
        # sums are made of thousands of points like those of the random maps
        seen = np.argwhere(observed)
        for i, h in enumerate(seen[rng.integers(0, len(seen), 3 * BODY_POINTS // 4)]):
            body[i] = inside(h + lo)
    return Case(cid, om, res, poses, edge, {k: np.asarray(v) for k, v in classes.items()}, body)


def loop_end(om, q, T_in, max_it, res):
    """(iterations, cause, trace) of the oracle's loop: 'cut' by max_iterations, 'empty' (c == 0) or 'converged'"""
    T, it, trace = O.register_cloud(om, q, T_in, max_it, IT_WEIGHT_GRADIENT, EPSILON, res, trace_cap=max(max_it, 1))
    if it and int(trace[it - 1][43]) == 0:
        cause = "empty"
    elif it >= max_it:
        cause = "cut"
    else:
        cause = "converged"
    return T, it, cause, trace
