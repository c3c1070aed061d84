"""Stores of many chunks for the packed snapshots (ws_store_pack / ws_store_unpack): N chunks that cycle through the brick cases of
pack_model.py under a fixed pseudo-random spread of keys, and the model's stream over them.  The model packs each distinct chunk once
(pack_model.pack_chunk) and stamps key and first payload word per header, so a thousand chunks take well under a second.

The cycle has 80 places: most hold one of the eight cheap cases (at most 2051 payload words), one in twenty `random` or `two_words`,
one in forty one of the two all-dense `odd_*` cases: about 60 MB of payload for 1030 chunks."""
import numpy as np

import pack_model as PM

CHEAP = ("all_fill", "one_word", "single_first", "single_last", "halves", "but_last", "word0_fill", "neighbours")
HEAVY = {9: "odd_in_fill", 19: "random", 39: "two_words", 49: "odd_in_uniform", 59: "random", 79: "two_words"}
KEY_ENDS = [(PM.IMAX, PM.IMIN, 0), (PM.IMAX - 1, PM.IMIN, 0), (PM.IMIN, PM.IMAX, -1), (-1, -1, -1)]


def case_of(i):
    """the name of the brick case of the i-th chunk made"""
    return HEAVY.get(i % 80) or CHEAP[(i - i // 20) % len(CHEAP)]


def scene_keys(n):
    """n distinct keys in the order the chunks are made: drawn from [-40, 40)^3 with a fixed seed, the four key ends spread among
    them; not ascending"""
    rng = np.random.default_rng(1030)
    drawn = {tuple(int(v) for v in k) for k in rng.integers(-40, 40, (2 * n, 3))} - set(KEY_ENDS)
    keys = [sorted(drawn)[i] for i in rng.permutation(len(drawn))][:n - len(KEY_ENDS)]
    for j, end in enumerate(KEY_ENDS):
        keys.insert((j * 37 + 5) % (len(keys) + 1), end)
    assert len(keys) == n == len(set(keys)) and keys != sorted(keys)
    return keys


_SCENES = {}


def scene(n):
    """dict(chunks={key: chunk}, names={key: case name}, keys=the keys ascending); the chunks are the arrays of PM.brick_cases()"""
    if n not in _SCENES:
        cases, keys = PM.brick_cases(), scene_keys(n)
        names = {key: case_of(i) for i, key in enumerate(keys)}
        _SCENES[n] = dict(chunks={key: cases[names[key]] for key in keys}, names=names, keys=sorted(keys))
    return _SCENES[n]


_PACKED = {}


def stream(sc, keys=None):
    """(headers, payload, stats) of the chunks of a scene (None: all) as PM.pack(sc["chunks"], PM.FILL, keys) gives them"""
    keys = sc["keys"] if keys is None else sorted(tuple(int(v) for v in k) for k in keys)
    for name in {sc["names"][k] for k in keys} - set(_PACKED):
        _PACKED[name] = PM.pack_chunk(PM.brick_cases()[name], (0, 0, 0), PM.FILL)
    headers, parts, first = np.zeros((len(keys), PM.HDR), dtype=np.uint32), [], 0
    for i, key in enumerate(keys):
        header, own = _PACKED[sc["names"][key]]
        headers[i] = header
        headers[i, 0:3] = np.asarray(key, dtype=np.int32).view(np.uint32)
        headers[i, 5], headers[i, 6] = first & 0xFFFFFFFF, first >> 32
        parts.append(own)
        first += len(own)
    payload = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    uniform, dense = int(headers[:, 3].sum()), int(headers[:, 4].sum())
    return headers, payload, [512 * len(keys) - uniform - dense, uniform, dense, 4 * (headers.size + payload.size)]
