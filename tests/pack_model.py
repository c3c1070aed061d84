"""The packed form of the store's chunks as numpy states it, written from the format text of include/warpsense_hip.h alone (ws_store_pack):
bricks, classes, the 40-word header and the payload stream; and the brick cases the host and the device tests share.

    chunk: 64^3 uint32, index x*4096 + y*64 + z; 8 x 8 x 8 bricks of 8^3 words
    brick b = ((x>>3)*8 + (y>>3))*8 + (z>>3); word (x&7)*64 + (y&7)*8 + (z&7) inside it
    class 0: every word == fill; 1: every word == word 0 != fill (1 payload word); 2: anything else (512 payload words)
    header: key[3], uniform bricks, dense bricks, first payload word lo, hi, 0, then 32 words of 2-bit class codes
"""
import numpy as np

CW = 64 ** 3
HDR = 40
FILL = np.uint32(600)            # (tau = 600, weight 0) as a raw entry
OTHER = np.uint32(600 | 9 << 16)  # free space at tau with a weight


def bricks(chunk):
    """(512, 512): the words of every brick in brick word order, bricks ascending"""
    c = np.asarray(chunk, dtype=np.uint32).reshape(8, 8, 8, 8, 8, 8)  # bx x7 by y7 bz z7
    return c.transpose(0, 2, 4, 1, 3, 5).reshape(512, 512)


def unbricks(b):
    return np.asarray(b, dtype=np.uint32).reshape(8, 8, 8, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(CW)


def classes(chunk, fill):
    b = bricks(chunk)
    all_fill = (b == np.uint32(fill)).all(axis=1)
    all_w0 = (b == b[:, :1]).all(axis=1)
    return np.where(all_fill, 0, np.where(all_w0, 1, 2)).astype(np.uint32)


def pack_chunk(chunk, key, fill, first=0):
    """(header[40], the chunk's own payload words)"""
    code, b = classes(chunk, fill), bricks(chunk)
    h = np.zeros(HDR, dtype=np.uint32)
    h[0:3] = np.asarray(key, dtype=np.int32).view(np.uint32)
    h[3], h[4] = int((code == 1).sum()), int((code == 2).sum())
    h[5], h[6] = first & 0xFFFFFFFF, first >> 32
    for i in range(512):
        h[8 + i // 16] |= np.uint32(int(code[i]) << (2 * (i % 16)))
    parts = [b[i, :1] if code[i] == 1 else b[i] for i in range(512) if code[i]]
    return h, (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32))


def pack(chunks, fill, keys=None):
    """(headers (n, 40), payload, stats[4]) of the chunks {key: words} in ascending key order"""
    keys = sorted(chunks) if keys is None else sorted(tuple(int(v) for v in k) for k in keys)
    headers, parts, first = np.zeros((len(keys), HDR), dtype=np.uint32), [], 0
    for i, key in enumerate(keys):
        headers[i], own = pack_chunk(chunks[key], key, fill, first)
        parts.append(own)
        first += len(own)
    payload = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    uniform, dense = int(headers[:, 3].sum()), int(headers[:, 4].sum())
    return headers, payload, [512 * len(keys) - uniform - dense, uniform, dense, 4 * (headers.size + payload.size)]


def expand(header, own, fill):
    """the 64^3 words of one chunk from its header and its own payload words"""
    out, at = np.empty((512, 512), dtype=np.uint32), 0
    for i in range(512):
        c = (int(header[8 + i // 16]) >> (2 * (i % 16))) & 3
        assert c != 3
        out[i] = fill if c == 0 else own[at] if c == 1 else own[at:at + 512]
        at += (0, 1, 512)[c]
    return unbricks(out)


def expand_all(headers, payload, fill):
    out = {}
    for h in headers:
        first = int(h[5]) | int(h[6]) << 32
        out[tuple(int(v) for v in h[0:3].view(np.int32))] = expand(h, payload[first:first + int(h[3]) + 512 * int(h[4])], fill)
    return out


def at(x, y, z):
    return x * 4096 + y * 64 + z


def word(b, w):
    """chunk index of word w of brick b"""
    return at((b >> 6) * 8 + (w >> 6), ((b >> 3) & 7) * 8 + ((w >> 3) & 7), (b & 7) * 8 + (w & 7))


def odd_word(b):
    """the one word of brick b that differs in the odd_* cases: 197 is odd, so every word number is the odd one of exactly one brick"""
    return (197 * b + 61) % 512


# the bricks of the `halves` case, all in the brick column 168 .. 175 (one wave's ballots): (brick, its one odd word or None for a
# uniform brick, the bit that differs from fill)
HALVES = ((168, 300, 0), (170, 37, 31), (171, None, 31), (173, None, 0))

_CASES = {}


def brick_cases(fill=FILL, other=OTHER):
    """{name: chunk}: the twelve chunks of the brick cases (made once, never written to)"""
    key = (int(fill), int(other))
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(40)
    full = lambda v: np.full(CW, v, dtype=np.uint32)
    c = {"all_fill": full(fill), "one_word": full(other)}
    # a single non-fill word at word 0 of brick 0 and of brick 511 / at word 511 of both
    c["single_first"], c["single_last"] = full(fill), full(fill)
    for b in (0, 511):
        c["single_first"][word(b, 0)] = other
        c["single_last"][word(b, 511)] = other
    # uniform bricks but for their last word (brick 77), and next to it a brick that is uniform indeed
    c["but_last"] = full(fill)
    for w in range(512):
        c["but_last"][word(77, w)] = other
        c["but_last"][word(78, w)] = other
    c["but_last"][word(77, 511)] = other ^ np.uint32(1)
    # word 0 equals fill while the others do not: twice, once with the others all alike
    c["word0_fill"] = full(fill)
    for w in range(1, 512):
        c["word0_fill"][word(300, w)] = other
        c["word0_fill"][word(5, w)] = np.uint32(w)
    # a uniform brick next to a dense one in the same brick column (bricks 8 k .. 8 k + 7 share a wave), on both sides
    c["neighbours"] = full(fill)
    for b, kind in ((160, 2), (161, 1), (162, 2), (167, 1), (166, 2), (504, 1), (505, 2)):
        for w in range(512):
            c["neighbours"][word(b, w)] = other if kind == 1 else np.uint32(1 + b * 512 + w)
    c["random"] = rng.integers(0, 2 ** 32, CW, dtype=np.uint64).astype(np.uint32)
    # every brick drawn from {fill, one other word}: a third all fill, a third all other, a third mixed
    mode = rng.integers(0, 3, 512)
    b = np.where(mode[:, None] == 0, fill, np.where(mode[:, None] == 1, other, np.where(rng.random((512, 512)) < 0.5, fill, other))).astype(np.uint32)
    c["two_words"] = unbricks(b)
    # every brick has ONE deciding word, and every word number 0 .. 511 is the deciding one of one brick: in fill (a classifier blind
    # to that position calls the brick default) and in a uniform brick (it calls the brick uniform)
    odd = odd_word(np.arange(512))
    b = np.full((512, 512), fill, dtype=np.uint32)
    b[np.arange(512), odd] = other
    c["odd_in_fill"] = unbricks(b)
    b = np.full((512, 512), other, dtype=np.uint32)
    b[np.arange(512), odd] = other ^ np.uint32(1)
    c["odd_in_uniform"] = unbricks(b)
    # a difference from fill in the lowest or in the highest bit alone, in one word of a brick and in all of them
    c["halves"] = full(fill)
    for brick, w, bit in HALVES:
        for i in range(512) if w is None else (w,):
            c["halves"][word(brick, i)] = fill ^ np.uint32(1 << bit)
    for v in c.values():
        v.setflags(write=False)
    _CASES[key] = c
    return c


# the keys the cases live under in a store: negative ones, and the key ends of two_store_scenes.KEY_END_KEYS
IMAX, IMIN = 2 ** 31 - 1, -2 ** 31
CASE_KEYS = {"all_fill": (0, 0, 0), "one_word": (-1, -1, -1), "single_first": (IMAX, IMIN, 0), "single_last": (IMAX - 1, IMIN, 0), "but_last": (IMIN, IMAX, -1),
             "word0_fill": (-3, 2, -2), "neighbours": (0, 0, 1), "random": (0, -1, 0), "two_words": (5, 5, 5),
             "odd_in_fill": (-7, 3, 4), "odd_in_uniform": (3, -4, 2), "halves": (1, 0, -5)}
N_CASES = len(CASE_KEYS)


def case_store(fill=FILL, other=OTHER):
    """{key: chunk} of the cases"""
    return {CASE_KEYS[name]: chunk for name, chunk in brick_cases(fill, other).items()}
