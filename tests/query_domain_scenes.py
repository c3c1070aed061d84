"""The windows, entries, rays and chunk stores at other resolutions and far positions on which every map and store query is tested
(tests/test_gpu_query_domain.py on the device, tests/test_query_domain_host.py on the models alone)."""
import numpy as np

import distance_model as D
import mesh_model as M
import query_model as QM
import raycast_model as R
import store_raycast_scenes as H
import store_scenes as SM
import surface_model as G


TAU, MW = G.TAU, 640
I32 = 2 ** 31 - 1
CS = 64

# ------------------------------------------------------------------------------------------------ the window grid
SIZE = (21, 17, 13)        # the smallest of G.SIZES
OFF = (5, 11, 9)           # the ring's seam lies inside the window on every axis
NEAR = (0, 0, 3)
ROWS = [(2, NEAR), (3, NEAR), (51, NEAR), (1024, NEAR),
        (50, (40_000_000, -20_000_000, 3)),        # voxel x beyond 2^24 (marker rounding), mm near 2 * 10^9
        (1024, (-2_000_000, 1_000_000, 3)),        # negative far, the largest resolution
        (2, (1_000_000_000, -500_000_000, 3))]     # the ring sum b - pos + offset + size at 10^9
FAR_ROWS = ROWS[4:]


BIG = 2 ** 30 - 1
SPECIAL = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0], [BIG, BIG, -BIG], [-BIG, 3, BIG], [BIG, -BIG, 7], [2 ** 30, 1, 1],
                    [0, 0, 0], [-2 ** 31, 0, 0]], dtype=np.int64)  # the list of test_rotated_rings_after_the_shift_sequence
N_RANDOM = 2048


_ENTRIES = []


def entries():
    """storage-order entries of the two maps, drawn once: the mesh's draw (ray cast, mesh, surface) and the distance field's draw"""
    if not _ENTRIES:
        _ENTRIES.extend([M.draw_entries(SIZE, seed=5), D.draw_entries(SIZE, seed=5)])
    return _ENTRIES


def ring(pos, which=0):
    return R.Ring(entries()[which], SIZE, pos, OFF)


def rays(res, pos):
    """origin at the window's centre, 2048 random directions and the special ones; max_range"""
    lo, _ = QM.window(SIZE, pos)
    o, d = R.random_rays(SIZE, seed=sum(SIZE), lo=lo, n=N_RANDOM, res=res)
    return o, np.concatenate([d, SPECIAL]), 60 * res


def counts(want):
    return H.hits_of(want[0]), int(np.count_nonzero(np.any(want[1] != 0, axis=1)))


def inner_box(pos):
    lo, hi = QM.window(SIZE, pos)
    return lo + (1, 2, 1), hi - (2, 1, 1)


def edge_case(res, sign, axis=0):
    """an origin with |o| + max_range + 2 res == INT32_MAX exactly on `axis`, in the centre voxel of a window: (pos, origin, range)"""
    rng = 60 * res
    pos, o = [7, -5, 3], [7 * res + 1, -5 * res + 2, 3 * res + 3]
    o[axis] = sign * (I32 - rng - 2 * res)
    pos[axis] = o[axis] // res
    return tuple(pos), np.asarray(o, dtype=np.int64), rng


def wrap_targets(o, rng, res):
    """targets from an origin at the negative edge of x: 64 with d_x = 2^30 - 1 (live), 64 with 2^30 (dead), 64 whose true d_x of about
    2^32 wraps, in 32 bits, to a short ray towards -x (dead; live and mostly hitting if the subtraction were 32-bit)"""
    g = np.random.default_rng(3)
    m = rng + 2 * res
    out = []
    for dx, spread in ((2 ** 30 - 1, 2 ** 29), (2 ** 30, 2 ** 29), (2 ** 32 - (m + 1000), m + 1000)):
        d = np.concatenate([np.full((64, 1), dx, dtype=np.int64), g.integers(-spread, spread + 1, (64, 2))], axis=1)
        out.append(o + d)
    tgt = np.concatenate(out)
    assert np.all(np.abs(tgt) <= I32), (np.abs(tgt).max(), I32)
    return tgt


# ------------------------------------------------------------------------------------------------ the store grid
STORE_RES = (1, 3, 51, 1024)  # ws_store_raycast and ws_store_mesh admit map_resolution >= 1: half = 0, step = 1
GAP = 13                      # absent chunks between the block and the isolated chunk, along x


def store_keys(res, where):
    """(key origin K of the 2 x 2 x 2 block K .. K + 1, x key of the isolated chunk).  "near": the block straddles the world origin.
    "+" / "-": the isolated chunk is the outermost chunk whose every voxel the mesh's range rule admits, within one chunk of
    +-INT32_MAX mm; the block lies 13 absent chunks nearer to the origin"""
    if where == "near":
        return (-1, -1, -1), 1 + GAP
    k_out = (I32 // res - 1 - (CS - 1)) // CS  # 64 k + 63 <= INT32_MAX / res - 1
    assert (CS * k_out + CS) * res <= I32 < (CS * (k_out + 2)) * res, ((CS * k_out + CS) * res, I32, (CS * (k_out + 2)) * res)
    if where == "+":
        return (k_out - GAP - 2, 3, -2), k_out
    k_neg = (I32 // res - 1) // CS  # the chunk -k holds the voxels -64 k .. -64 k + 63: (64 k + 1) res <= INT32_MAX
    return (-k_neg + GAP + 1, 3, -2), -k_neg


_STORE = {}


def store_chunks(res, where):
    """seven chunks of the block (the one at K + (1, 1, 0) absent) and the isolated chunk, drawn entries"""
    if "world" not in _STORE:
        _STORE["world"] = M.draw_entries((2 * CS,) * 3, seed=128).reshape((2 * CS,) * 3)
        _STORE["lone"] = M.draw_entries((CS,) * 3, seed=77)
    K, x_lone = store_keys(res, where)
    w = _STORE["world"]
    out = {}
    for c in SM.SEAM_KEYS:
        if c == SM.ABSENT:
            continue
        out[tuple(K[k] + c[k] + 1 for k in range(3))] = np.ascontiguousarray(w[tuple(slice(CS * (v + 1), CS * (v + 2)) for v in c)]).reshape(-1)
    out[(x_lone, K[1], K[2])] = _STORE["lone"]
    return out


def store_base(res, where):
    return store_keys(res, where)[0]


def store_boxes(res, where):
    """None (the default box) and a sub-box that cuts through the chunks of the block"""
    K = np.asarray(store_keys(res, where)[0], dtype=np.int64) * CS
    return [None, (K + (24, 35, 14), K + (101, 109, 84))]


def store_rays(res, where):
    """(origin, dirs, range) of the ray sets: "in" -- from the block's common corner, 2048 random directions and the special ones,
    60 res; "gap" -- from the absent stretch two chunks off the block towards the isolated chunk, across the absent chunks between,
    with the largest range the origin admits on the far side"""
    K, x_lone = store_keys(res, where)
    Kv = np.asarray(K, dtype=np.int64) * CS
    g = np.random.default_rng(19)
    o_in = (Kv + CS) * res + np.array([res // 3, -(res // 2), res // 5])
    d_in = np.concatenate([g.integers(-32768, 32769, (N_RANDOM, 3)), SPECIAL])
    towards = 1 if x_lone > K[0] else -1
    x_from = (K[0] + 3) * CS + 5 if towards > 0 else (K[0] - 1) * CS - 5  # a voxel in the absent chunk next but one to the block
    o_gap = np.array([x_from * res + 1, (Kv[1] + 20) * res + 2, (Kv[2] + 30) * res], dtype=np.int64)
    lone_lo = np.array([x_lone * CS, Kv[1], Kv[2]], dtype=np.int64)
    tgt = (lone_lo + g.integers(2, CS - 2, (256, 3))) * res
    tgt[:, 0] = (lone_lo[0] + (2 if towards > 0 else CS - 3)) * res  # the face of the isolated chunk that looks at the block
    d_gap = np.concatenate([tgt - o_gap, -(tgt - o_gap)[:16], np.array([[towards, 0, 0], [towards * 4096, 1, -1]])])
    reach = (GAP + 1) * CS * res
    if where != "near":
        reach = I32 - 2 * res - int(np.abs(o_gap).max())  # |o| + max_range + 2 res == INT32_MAX exactly
        assert reach > (GAP - 2) * CS * res, (reach, (GAP - 2) * CS * res)
    return {"in": (o_in, d_in, 60 * res), "gap": (o_gap, d_gap, int(reach))}


def store_model(res, where, name, box=None, any_weight=False):
    o, d, rng = store_rays(res, where)[name]
    lo, hi = (None, None) if box is None else box
    return R.model(H.Chunks(store_chunks(res, where), lo, hi, base=store_base(res, where)), res, o, d, rng, any_weight)


STORE_CASES = [(res, where) for res in STORE_RES for where in ("near", "+", "-")]


def store_id(case):
    return f"res{case[0]}{case[1]}"


def moved(rec, s_mm):
    """ray records moved by s_mm where they hit"""
    out = rec.copy()
    hit = rec["range_mm"] >= 0
    for k, name in enumerate(("x_mm", "y_mm", "z_mm")):
        out[name][hit] = rec[name][hit] + int(s_mm[k])
    return out


def moved_vert(vert, s_mm):
    out = vert.copy()
    for k, name in enumerate(("x_mm", "y_mm", "z_mm")):
        out[name] = vert[name] + int(s_mm[k])
    return out


def moved_surface(rec, s):
    out = rec.copy()
    for k, name in enumerate("xyz"):
        out[name] = rec[name] + int(s[k])
    return out
