"""The numpy model of ws_store_coarsen (the rule stated in include/warpsense_hip.h): dictionaries of chunks in, the dictionary of DST's
chunks after the call and the four statistics out.  Chunks are 262 144 uint32, index x * 4096 + y * 64 + z, keyed by
floor(world voxel / 64); the parent of a key is floor(key / 2)."""
import numpy as np

CS, CW = 64, 64 ** 3


def unpack(raw):
    raw = np.asarray(raw, dtype=np.uint32)
    return (raw & 0xFFFF).astype(np.uint16).astype(np.int16).astype(np.int64), (raw >> 16).astype(np.uint16).astype(np.int16).astype(np.int64)


def pack(value, weight):
    v = np.asarray(value, dtype=np.int64).astype(np.int16).astype(np.uint16).astype(np.uint32)
    w = np.asarray(weight, dtype=np.int64).astype(np.int16).astype(np.uint16).astype(np.uint32)
    return v | (w << np.uint32(16))


def parents_of(keys):
    """the parents of (n, 3) keys, unique and ascending (cx, cy, cz), as an (m, 3) int64 array"""
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    return np.asarray(sorted({tuple(int(v) for v in row) for row in np.floor_divide(k, 2)}), dtype=np.int64).reshape(-1, 3)


def coarsen_entries(value, weight, min_observed, fill):
    """the rule on arrays whose LAST axis holds the eight children: (entries, n)"""
    value, weight = np.asarray(value, dtype=np.int64), np.asarray(weight, dtype=np.int64)
    observed = weight > 0
    n = observed.sum(axis=-1)
    S = np.where(observed, value, 0).sum(axis=-1)
    W = np.where(observed, weight, 1 << 40).min(axis=-1)
    mean = np.floor_divide(S, np.maximum(n, 1))  # floor toward minus infinity
    return np.where(n >= min_observed, pack(mean, np.where(n > 0, W, 0)), np.uint32(fill)).astype(np.uint32), n


def coarsen_chunk(src, key, min_observed, fill):
    """the dst chunk `key` from the chunks of src: (262 144 uint32, n per voxel, whether any child chunk exists)"""
    fine = np.zeros((2 * CS,) * 3, dtype=np.uint32)  # weight 0: a child in an absent chunk is unobserved
    any_child = False
    for c in range(8):
        d = (c >> 2, (c >> 1) & 1, c & 1)
        child = tuple(2 * int(key[a]) + d[a] for a in range(3))
        if child in src:
            any_child = True
            fine[tuple(slice(CS * d[a], CS * d[a] + CS) for a in range(3))] = np.asarray(src[child], dtype=np.uint32).reshape(CS, CS, CS)
    # the children of the coarse voxel (X, Y, Z) are fine[2 X + i, 2 Y + j, 2 Z + k]
    eight = fine.reshape(CS, 2, CS, 2, CS, 2).transpose(0, 2, 4, 1, 3, 5).reshape(CS, CS, CS, 8)
    value, weight = unpack(eight)
    out, n = coarsen_entries(value, weight, min_observed, fill)
    return out.reshape(-1), n.reshape(-1), any_child


def coarsen(dst, src, keys=None, min_observed=8, fill=0):
    """(DST's chunks after the call, [chunks processed, chunks created, voxels that received a value, voxels with 1 <= n < min_observed])"""
    out = {k: np.array(v, dtype=np.uint32) for k, v in dst.items()}
    listed = parents_of(list(src)) if keys is None else np.asarray(sorted({tuple(int(v) for v in k) for k in np.asarray(keys).reshape(-1, 3)}), dtype=np.int64).reshape(-1, 3)
    stats = [0, 0, 0, 0]
    for key in (tuple(int(v) for v in k) for k in listed):
        data, n, any_child = coarsen_chunk(src, key, min_observed, fill)
        if not any_child and key not in out:
            continue
        stats[0] += 1
        stats[1] += key not in out
        stats[2] += int(np.count_nonzero(n >= min_observed))
        stats[3] += int(np.count_nonzero((n >= 1) & (n < min_observed)))
        out[key] = data
    return out, stats


def pyramid(base, levels, min_observed=8, fill=0):
    """[base, level 1, ...]: the model applied `levels` times, each level from nothing"""
    out = [base]
    for _ in range(levels):
        out.append(coarsen({}, out[-1], None, min_observed, fill)[0])
    return out


def same(a, b):
    """two chunk dictionaries hold the same keys and bytes"""
    return sorted(a) == sorted(b) and all(np.asarray(a[k], dtype=np.uint32).tobytes() == np.asarray(b[k], dtype=np.uint32).tobytes() for k in a)
