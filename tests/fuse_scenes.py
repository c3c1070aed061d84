"""The scenes of the ws_store_fuse tests: random chunks, the identity case and its route through the C oracle, rigid transforms, the
sphere-and-floor map, and the stores of a GPU test with their read-back."""
import numpy as np

import fuse_model as F
import oracle_lib as O

RES, TAU, MW = 64, 600, 640
FILL = int(F.pack(TAU, 0))


def draw(seed, src):
    """a chunk of random entries.  src: weights 0 (three in ten) or 1 .. 32767; dst: also negative weights.  Values reach +-32767, and
    the weights are large enough for ew + nw to pass max_weight"""
    rng = np.random.default_rng(seed)
    value = np.where(rng.random(F.CW) < 0.05, rng.choice([-32767, 32767], F.CW), rng.integers(-TAU, TAU + 1, F.CW))
    u = rng.random(F.CW)
    weight = np.where(u < 0.6, rng.integers(1, 700, F.CW), np.where(u < 0.7, rng.choice([32767, 32000], F.CW), 0))
    if not src:
        weight = np.where(rng.random(F.CW) < 0.15, -rng.integers(1, 32768, F.CW), weight)
    return F.pack(value, weight)


def identity_case():
    """3 src and 3 dst chunks, two shared"""
    src = {(0, 0, 0): draw(1, True), (0, 0, 1): draw(2, True), (-1, 0, 0): draw(3, True)}
    dst = {(0, 0, 0): draw(4, False), (0, 0, 1): draw(5, False), (0, -1, 0): draw(6, False)}
    return dst, src


def oracle_route(dst, src, max_weight, fill):
    """the C oracle's integrate chunk by chunk over the union of the keys: new = the src chunk or weight 0, avg = the dst chunk or fill"""
    out = {}
    for key in sorted(set(dst) | set(src)):
        new = np.array(src[key], dtype=np.uint32) if key in src else np.full(F.CW, F.pack(7, 0), dtype=np.uint32)
        avg = np.array(dst[key], dtype=np.uint32) if key in dst else np.full(F.CW, fill, dtype=np.uint32)
        O.lib().wso_update_avg(O._p(new), O._p(avg), F.CW, int(max_weight), TAU)  # (it also resets `new`: not looked at)
        out[key] = avg
    return out


def rot(yaw=0.0, pitch=0.0, roll=0.0, t=(0, 0, 0)):
    """4 x 4: Rz(yaw) Ry(pitch) Rx(roll) in degrees, translation t in mm"""
    a, b, c = np.deg2rad([yaw, pitch, roll])
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, t
    return T


def split(world, first_key):
    """a dense (64 a, 64 b, 64 c) array as chunks, its first voxel the first voxel of chunk first_key"""
    n = [s // 64 for s in world.shape]
    return {(first_key[0] + i, first_key[1] + j, first_key[2] + k): np.ascontiguousarray(world[64 * i:64 * i + 64, 64 * j:64 * j + 64, 64 * k:64 * k + 64]).reshape(-1)
            for i in range(n[0]) for j in range(n[1]) for k in range(n[2])}


def sphere_and_floor(shift=(0.0, 0.0, 0.0), weight=20, res=RES):
    """a TSDF over the world voxels [-64, 63]^3, chunks (-1 .. 0)^3: a sphere above a floor, observed (weight > 0) inside the
    truncation band only; `shift` moves the scene, in voxels"""
    c = np.arange(-64, 64, dtype=np.float64) + 0.5
    x, y, z = np.meshgrid(c - shift[0], c - shift[1], c - shift[2], indexing="ij")
    d = np.minimum(np.sqrt((x - 3.3) ** 2 + (y + 4.1) ** 2 + (z - 6.2) ** 2) - 30.4, z + 41.3) * res
    value = np.clip(np.rint(d), -TAU, TAU).astype(np.int64)
    return split(F.pack(value, np.where(np.abs(d) < TAU, weight, 0)).reshape(128, 128, 128), (-1, -1, -1))


def make_store(chunks, max_chunks=0, fill=(TAU, 0), segment_chunks=2):
    import warpsense_amd as W
    store = W.DeviceGlobalMap(fill[0], fill[1], max_chunks=max_chunks, segment_chunks=segment_chunks)
    for key in sorted(chunks):
        store.put_chunk(key, chunks[key])
    return store


def read(store):
    return {k: store.chunk(k) for k in store.keys()}
