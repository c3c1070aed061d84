"""The scenes of the ground tests: columns of random runs with planted floors, as a region of the world, as the chunks of a store and
as the content of a window; and the ramp and kerb scenes of the bridge to the planner."""
import numpy as np

import ground_model as G
import store_scenes as SM

TAU, RES, MW, CS = G.TAU, 50, 640, 64

# ------------------------------------------------------------------------------------------------ random runs
def random_columns(shape, seed, max_run):
    """(value, weight) of `shape`: every column a sequence of runs of one class (free 1/2, occupied 1/4, unknown 1/4), 1 .. max_run
    voxels each; an unknown voxel has weight 0 or a negative weight, so WS_GROUND_ANY_WEIGHT changes the classes"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    value, weight = G.entries(shape)
    for x in range(nx):
        for y in range(ny):
            z = 0
            while z < nz:
                n = int(rng.integers(1, max_run + 1))
                kind = int(rng.choice((1, 1, 2, 0)))
                s = slice(z, min(nz, z + n))
                k = s.stop - s.start
                if kind == 2:
                    value[x, y, s], weight[x, y, s] = -rng.integers(1, 2 * TAU + 1, k), rng.integers(1, MW + 1, k)
                elif kind == 1:
                    value[x, y, s], weight[x, y, s] = rng.integers(0, 2 * TAU + 1, k), rng.integers(1, MW + 1, k)
                else:
                    value[x, y, s], weight[x, y, s] = rng.integers(-TAU, TAU + 1, k), -rng.integers(0, 2, k) * rng.integers(1, MW + 1, k)
                z += n
    return value, weight


def plant(value, weight, x, y, z, free, v0=-300, v1=300):
    """the column (x, y) unknown but for a floor at z with `free` free voxels above it"""
    value[x, y, :], weight[x, y, :] = 0, 0
    value[x, y, max(0, z - 1):z], weight[x, y, max(0, z - 1):z] = -TAU, 5
    G.put_floor(value, weight, x, y, z, v0=v0, v1=v1, free=free)


# ------------------------------------------------------------------------------------------------ the stack of chunks
REGION_LO, REGION_SHAPE = (-6, -4, 0), (12, 8, 3 * CS)   # x and y cross the chunk border at 0; three chunks stacked in z
STACK_KEYS = [(cx, cy, cz) for cx in (-1, 0) for cy in (-1, 0) for cz in (0, 1, 2)]
FULL_BOX = ((-5, -3, 0), (3, 2, 3 * CS - 1))             # 9 x 6 columns: no multiple of four
# planted floors (world x, y, z, free voxels above): at lz = 62, 63 and 0; lz = 63 of the middle chunk with headroom to the last voxel of
# the top chunk; a floor whose free space ends at the chunk border, under unknown voxels; a floor in mid-chunk for the cut boxes
PLANTED = {"lz 62": (-5, -3, 62, 10), "lz 63": (-4, -3, 63, 70), "lz 0": (-3, -3, 64, 12), "lz 63, headroom to the top": (-2, -3, 127, 64),
           "free ends at the border": (-1, -2, 60, 3), "mid-chunk": (0, -2, 100, 30)}
_CACHE = {}


def stack_region():
    if "region" not in _CACHE:
        value, weight = random_columns(REGION_SHAPE, 4100, 70)
        for i, (x, y, z, free) in enumerate(PLANTED.values()):
            plant(value, weight, x - REGION_LO[0], y - REGION_LO[1], z, free, v0=-(37 + 100 * i), v1=11 + 90 * i)
        _CACHE["region"] = G.pack(value, weight)
    return _CACHE["region"]


def stack_chunks(absent_layer=None):
    """key -> 262 144 entries: the region inside the twelve chunks, weight 0 around it; absent_layer: no chunk of that cz"""
    key = ("chunks", absent_layer)
    if key not in _CACHE:
        world = np.zeros((2 * CS, 2 * CS, 3 * CS), dtype=np.uint32)  # x, y in [-64, 63]
        r = stack_region()
        world[CS + REGION_LO[0]:CS + REGION_LO[0] + r.shape[0], CS + REGION_LO[1]:CS + REGION_LO[1] + r.shape[1], :] = r
        _CACHE[key] = {k: np.ascontiguousarray(world[CS * (k[0] + 1):CS * (k[0] + 2), CS * (k[1] + 1):CS * (k[1] + 2), CS * k[2]:CS * (k[2] + 1)]).reshape(-1)
                       for k in STACK_KEYS if k[2] != absent_layer}
    return _CACHE[key]


def stack_model(absent_layer, lo, hi, H, **kw):
    key = ("model", absent_layer, tuple(lo), tuple(hi), H, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = G.model_box(SM.assemble(stack_chunks(absent_layer), lo, hi), lo, H, **kw)
    return _CACHE[key]


def make_store(chunks, shift=(0, 0, 0)):
    import warpsense_amd as W
    store = W.DeviceGlobalMap(TAU, 0, segment_chunks=5)
    for key in sorted(chunks):
        store.put_chunk(tuple(int(k + s) for k, s in zip(key, shift)), chunks[key])
    return store


FLAGS = [dict(any_weight=a, unknown_headroom=u, top=t) for a in (False, True) for u in (False, True) for t in (False, True)]


# ------------------------------------------------------------------------------------------------ windows
def make_window(size, pos, off, box):
    """a TSDFCuda over a ring of `size` at `pos` rotated by `off`, whose averaged map holds `box` (world order, the whole window)"""
    import warpsense_amd as W
    import query_model as QM
    n = int(np.prod(size))
    view = W.DeviceMap(size, off, np.zeros(n, dtype=np.uint32), pos)
    t = W.TSDFCuda(view, TAU, MW, RES)
    lo, hi = QM.window(size, pos)
    t.avg_map().insert_box(lo, hi, np.ascontiguousarray(box, dtype=np.uint32).reshape(-1))
    return t, tuple(int(v) for v in lo), tuple(int(v) for v in hi)


def window_box(shape, seed, max_run):
    value, weight = random_columns(shape, seed, max_run)
    nz = shape[2]
    plant(value, weight, 1, 1, 2, nz - 4)            # a floor near the bottom with free space almost to the top
    plant(value, weight, 2, 1, nz - 2, 1)            # a floor whose one free voxel is the last voxel of the window
    value[3, 2, :], weight[3, 2, :] = TAU, 5         # an occupied voxel at the very top, free below it: never a level
    value[3, 2, nz - 1] = -300
    return G.pack(value, weight)


# ------------------------------------------------------------------------------------------------ the bridge: a ramp and a kerb
RAMP_SHAPE = (30, 5, 32)
LOWER_Z, UPPER_Z = 4, 16     # two floors one level apart
BAND = (5, 12)               # the height band of a robot on the lower floor, for ws_*_distance(COLUMNS)


def ramp_floor_z(x):
    return LOWER_Z if x < 8 else UPPER_Z if x >= 20 else LOWER_Z + (x - 7)


def ramp_world():
    """lower floor for x < 8, a ramp of one voxel per column for x = 8 .. 19, the upper floor for x >= 20; two solid voxels under every
    floor voxel, free space above it to the top, nothing known below"""
    value, weight = G.entries(RAMP_SHAPE)
    for x in range(RAMP_SHAPE[0]):
        z = ramp_floor_z(x)
        for y in range(RAMP_SHAPE[1]):
            value[x, y, z - 2:z], weight[x, y, z - 2:z] = -TAU, 5
            G.put_floor(value, weight, x, y, z, v0=-200, v1=300, free=RAMP_SHAPE[2] - 1 - z)
    return G.pack(value, weight)


KERB_SHAPE = (12, 4, 32)


def kerb_world():
    """a floor at z = 6 for x < 6, a solid kerb of two voxels, a floor at z = 8 for x >= 6"""
    value, weight = G.entries(KERB_SHAPE)
    for x in range(KERB_SHAPE[0]):
        z = 6 if x < 6 else 8
        for y in range(KERB_SHAPE[1]):
            value[x, y, 4:z], weight[x, y, 4:z] = -TAU, 5
            G.put_floor(value, weight, x, y, z, free=KERB_SHAPE[2] - 1 - z)
    return G.pack(value, weight)


def world_chunks(world, lo):
    """the dense box `world` whose first voxel is world voxel `lo`, as chunks (weight 0 around it)"""
    lo = np.asarray(lo, dtype=np.int64)
    hi = lo + np.asarray(world.shape) - 1
    out = {}
    for cx in range(int(lo[0] // CS), int(hi[0] // CS) + 1):
        for cy in range(int(lo[1] // CS), int(hi[1] // CS) + 1):
            for cz in range(int(lo[2] // CS), int(hi[2] // CS) + 1):
                base = np.array([cx, cy, cz]) * CS
                chunk = np.zeros((CS, CS, CS), dtype=np.uint32)
                a, b = np.maximum(lo, base), np.minimum(hi, base + CS - 1)
                chunk[tuple(slice(int(a[k] - base[k]), int(b[k] - base[k]) + 1) for k in range(3))] = \
                    world[tuple(slice(int(a[k] - lo[k]), int(b[k] - lo[k]) + 1) for k in range(3))]
                out[(cx, cy, cz)] = chunk.reshape(-1)
    return out
