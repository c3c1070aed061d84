"""Stores with a history for the calls that read one chunk store and write or compare another (ws_store_fuse, ws_store_coarsen,
ws_store_changes): a pure-Python replay of the directory rules of api_store.hip, a history of puts and drops that leaves a store
holding exactly the chunks of a scene in slots that are neither in key order nor fresh, the pairs of pool geometries of the two-store
tests, their scenes with the numpy models' results, and the host arithmetic of the long coarsen plan."""
import numpy as np

import changes_model as M
import changes_scenes as CS
import coarsen_model as CM
import fuse_model as F
import fuse_scenes as S
from fuse_scenes import FILL, MW, RES, TAU

CHUNK_BYTES = 4 * CM.CW
# (first store, second store): SRC and DST of fuse and coarsen, CUR and REF of changes; 0 is the default of 256 chunks per segment
PAIRS = [(1, 4), (4, 1), (2, 1), (1, 0), (0, 2), (2, 2)]


def shift_of(segment_chunks):
    """seg_shift of ws_store_create: the default is 256 chunks, any other value is rounded up to a power of two"""
    want, shift = segment_chunks or 256, 0
    while (1 << shift) < want:
        shift += 1
    return shift


class Directory:
    """The key -> slot directory of a ws_store as api_store.hip keeps it: free_slots is a stack, next_slot counts up, and the capacity
    is whole segments (store_make_room, store_grow, store_take_slot, ws_store_put_chunk, ws_store_drop_chunk)."""

    def __init__(self, segment_chunks):
        self.shift, self.dir, self.free, self.next, self.nseg = shift_of(segment_chunks), {}, [], 0, 0
        self.recycled = set()  # the keys whose present slot came off the stack of freed slots
        self.wrote = {}  # slot -> (what, key) of the last bytes put there: they stay in the segment after a drop

    def capacity(self):
        return self.nseg << self.shift

    def make_room(self, fresh):
        if fresh > len(self.free) + self.capacity() - self.next:
            chunks = self.next + fresh - len(self.free)
            self.nseg = max(self.nseg, (chunks + (1 << self.shift) - 1) >> self.shift)

    def take(self, key):
        if self.free:
            self.dir[key] = self.free.pop()
            self.recycled.add(key)
        else:
            self.dir[key], self.next = self.next, self.next + 1

    def put(self, key, what="real"):
        if key not in self.dir:
            self.make_room(1)
            self.take(key)
        self.wrote[self.dir[key]] = (what, key)

    def create(self, keys):
        """what a fuse or a coarsen does for the chunks it creates: room for all of them, then slots in key order"""
        keys = sorted(set(keys) - set(self.dir))
        self.make_room(len(keys))
        for key in keys:
            self.take(key)

    def drop(self, key):
        self.free.append(self.dir.pop(key))
        self.recycled.discard(key)

    def run(self, ops):
        for op, key, what in ops:
            self.put(key, what) if op == "put" else self.drop(key)
        return self


def history(keys, seed):
    """The operations that leave a store holding exactly `keys`: [(op, key, what)], op "put" or "drop", what "real", "other" (other bytes
    under a real key, overwritten later) or "decoy" (a key outside every scene).  The keys go in in an order shuffled by seed, two decoys
    after each; a third of them first receive other bytes; then half of the decoys, a third of the real chunks and the other decoys are
    dropped, and those real chunks are put again: they take the slots the last decoys left."""
    rng = np.random.default_rng(seed)
    keys = sorted(tuple(int(v) for v in k) for k in keys)
    order = [keys[i] for i in rng.permutation(len(keys))]
    third = max(1, len(order) // 3) if order else 0
    early = [order[i] for i in sorted(rng.choice(len(order), third, replace=False))] if order else []
    again = [order[i] for i in rng.choice(len(order), third, replace=False)] if order else []
    decoys = [((1 << 20) + i, -(1 << 20) - seed, 7) for i in range(2 * len(order) + 2)]
    ops = []
    for i, key in enumerate(order):
        ops += [("put", key, "other" if key in early else "real"), ("put", decoys[2 * i], "decoy"), ("put", decoys[2 * i + 1], "decoy")]
    ops += [("put", d, "decoy") for d in decoys[-2:]]
    ops += [("put", key, "real") for key in reversed(early)]
    ops += [("drop", d, "decoy") for d in decoys[::2]] + [("drop", key, "real") for key in again] + [("drop", d, "decoy") for d in decoys[1::2]]
    ops += [("put", key, "real") for key in again]
    return ops


def replay(keys, segment_chunks, seed):
    return Directory(segment_chunks).run(history(keys, seed))


def claims(d, keys):
    """what a history must have achieved, on a directory: (not monotone in key order, reused slots, segments the chunks span)"""
    slots = [d.dir[k] for k in sorted(keys)]
    return slots != sorted(slots), len(d.recycled & set(keys)), len({s >> d.shift for s in slots})


def hold(d, keys, segment_chunks):
    """the claims every aged store of three chunks or more must meet"""
    mixed, reused, spans = claims(d, keys)
    return sorted(d.dir) == sorted(keys) and mixed and reused >= 1 and (spans >= 3 or segment_chunks not in (1, 2))


def astray(d, other_shift):
    """Where the lookup of each chunk's slot would land if the address were formed with the shift of the OTHER store:
    segment table [slot >> other_shift], chunk (slot & (2^other_shift - 1)) of that segment.  Per key: "same", the key of the chunk
    that owns the place, ("stale", what, key) for a free slot that still holds the bytes last put there, "unwritten" for a slot of a
    segment nothing was ever put into, or "outside" (past the segment table or past the segment)."""
    owner = {slot: key for key, slot in d.dir.items()}
    out = {}
    for key, slot in d.dir.items():
        seg, off = slot >> other_shift, slot & ((1 << other_shift) - 1)
        if seg >= d.nseg or off >= (1 << d.shift):
            out[key] = "outside"
        else:
            at = (seg << d.shift) + off
            out[key] = "same" if at == slot else owner[at] if at in owner else ("stale",) + d.wrote[at] if at in d.wrote else "unwritten"
    return out


def seen(d, other_shift, chunks):
    """the keys whose lookup under the other store's shift lands outside every allocation, and those that land in other bytes: another
    chunk of the scene whose bytes differ, or a free slot that still holds a decoy's bytes or the other bytes a real key was first given
    (random draws, unlike every chunk of a scene).  A bit-for-bit comparison cannot miss the second; the first is a fault."""
    where = astray(d, other_shift)
    differs = lambda a, b: np.asarray(chunks[a]).tobytes() != np.asarray(chunks[b]).tobytes()
    outside = sorted(k for k, w in where.items() if w == "outside")
    other = sorted(k for k, w in where.items() if isinstance(w, tuple) and
                   (w[1] in ("decoy", "other") or differs(w[2], k) if w[0] == "stale" else differs(w, k)))
    return outside, other


def aged_store(chunks, segment_chunks, seed, fill=(TAU, 0), max_chunks=0):
    """(store, record): a DeviceGlobalMap that holds exactly `chunks` after history(chunks, seed).  The record is read from the device:
    a segment's number cannot be read from a pointer, so the pointers of ws_store_chunk_dev are grouped by the segment the replay
    names, and the record is returned only if every group shares one base address a whole number of chunks below its members, the
    groups do not overlap, and capacity() is the replay's count of segments.  record: slots (by ascending key), segments, reused,
    spans (segments that hold a chunk), mixed (the slots are not monotone in key order), freed (device addresses of the free slots)."""
    import warpsense_amd as W
    from warpsense_amd._abi import _i3c
    store = W.DeviceGlobalMap(fill[0], fill[1], max_chunks=max_chunks, segment_chunks=segment_chunks)
    decoy = S.draw(9000 + seed, False)
    other = decoy ^ np.uint32(0x5A5A5A5A)
    d, freed = Directory(segment_chunks), {}
    ptr = lambda key: store._L.ws_store_chunk_dev(store.handle, _i3c(key))
    for op, key, what in history(chunks, seed):
        if op == "put":
            store.put_chunk(key, chunks[key] if what == "real" else other if what == "other" else decoy)
            d.put(key, what)
            freed.pop(d.dir[key], None)
        else:
            freed[d.dir[key]] = ptr(key)
            store.drop_chunk(key)
            d.drop(key)
    assert store.keys() == sorted(chunks) == sorted(d.dir) and store.capacity() == d.capacity()
    mask, bases = (1 << d.shift) - 1, {}
    for key, slot in d.dir.items():
        bases.setdefault(slot >> d.shift, set()).add(ptr(key) - (slot & mask) * CHUNK_BYTES)
    for slot, p in freed.items():
        bases.setdefault(slot >> d.shift, set()).add(p - (slot & mask) * CHUNK_BYTES)
    assert all(len(b) == 1 for b in bases.values()), bases
    start = sorted(next(iter(b)) for b in bases.values())
    assert all(b - a >= (CHUNK_BYTES << d.shift) for a, b in zip(start, start[1:])), start
    mixed, reused, spans = claims(d, chunks) if chunks else (False, 0, 0)
    return store, dict(slots=[d.dir[k] for k in sorted(chunks)], segments=d.nseg, reused=reused, spans=spans, mixed=mixed, freed=set(freed.values()), directory=d)


def check_record(record, n_chunks, segment_chunks):
    """the claims of the module docstring on the record of a store of three chunks or more"""
    if n_chunks >= 3:
        assert record["mixed"] and record["reused"] >= 1 and (record["spans"] >= 3 or segment_chunks not in (1, 2)), record


# ------------------------------------------------------------------------------------------------ the scenes
def observed(seed):
    """a chunk of random entries, every weight > 0"""
    rng = np.random.default_rng(seed)
    return CM.pack(rng.integers(-TAU, TAU + 1, CM.CW), rng.integers(1, 700, CM.CW))


_CACHE = {}


def _once(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _fuse_pose(T, pivot=None):
    import warpsense_amd as W
    return W.fuse_pose(T, pivot)


def _fuse_translation():
    """the identity rotation with a translation by whole voxels, negative keys on both sides"""
    src = {(-1, -1, -1): S.draw(21, True), (-2, -1, -1): S.draw(22, True), (-1, 0, -2): S.draw(23, True)}
    dst = {(-3, -1, 1): S.draw(24, False), (-2, -1, 1): S.draw(25, False), (-3, -1, 2): S.draw(26, False)}
    return dict(kind="fuse", first=src, second=dst, pose=_fuse_pose(S.rot(t=(-64 * RES - 3 * RES, 5 * RES, 130 * RES))))


def _fuse_general():
    """17 degrees yaw, 3 degrees pitch, (13, -7, 4) mm on the sphere-and-floor map in 2 x 2 x 2 chunks"""
    src, dst = S.sphere_and_floor(), S.sphere_and_floor(shift=(0.4, -0.3, 0.2), weight=35)
    del dst[(0, 0, 0)]
    return dict(kind="fuse", first=src, second=dst, pose=_fuse_pose(S.rot(17, 3, 0, (13, -7, 4))))


def _fuse_grow():
    """3 src and 3 dst chunks, two shared: (-1, 0, 0) is created while (0, 0, 0) and (0, 0, 1) are rewritten"""
    dst, src = S.identity_case()
    return dict(kind="fuse", first=src, second=dst, pose=F.identity_pose())


def _coarsen_mixed():
    src = {(-1, -1, -1): observed(31), (-3, 2, -2): observed(32), (1, 0, 0): observed(33), (2, 0, 0): observed(34),
           (10, 10, 11): observed(35), (11, 10, 11): observed(36)}
    return dict(kind="coarsen", first=src, second={}, keys=None, min_observed=8)


def _eight():
    src = {}
    for c in range(8):
        chunk = S.draw(20 + c, False).copy()
        chunk[c::97] = CM.pack(-32768, 3)
        chunk[(c + 5)::89] = CM.pack(-32768, 32767)
        src[(c >> 2, (c >> 1) & 1, c & 1)] = chunk
    return src


def _coarsen_listed():
    """(0, 0, 0) is overwritten, (7, 7, 7) turns to fill, (1, 0, 0) -- which has a child -- and (-1, 0, 0) are not listed and stay,
    (2, 2, 2) is created, (9, 9, 9) has neither a child nor a chunk"""
    src = {(0, 0, 0): observed(41), (1, 1, 1): observed(42), (2, 0, 0): observed(43), (4, 4, 4): observed(44)}
    dst = {(0, 0, 0): S.draw(45, False), (1, 0, 0): S.draw(46, False), (7, 7, 7): S.draw(47, False), (-1, 0, 0): S.draw(48, False)}
    return dict(kind="coarsen", first=src, second=dst, keys=[(7, 7, 7), (0, 0, 0), (9, 9, 9), (0, 0, 0), (2, 2, 2), (7, 7, 7)], min_observed=8)


def corner_case():
    """2 x 2 x 2 chunks with keys -1 and 0: everything observed free on both sides but the voxels at local 0 and 63 on every axis,
    which are occupied in one of the maps; (0, 0, -1) is in CUR only, (-1, -1, 0) in REF only"""
    free, cur, ref = np.full((64, 64, 64), F.pack(TAU, 9), dtype=np.uint32), {}, {}
    for i, key in enumerate((a, b, c) for a in (-1, 0) for b in (-1, 0) for c in (-1, 0)):
        one, two = free.copy(), free.copy()
        for j, l in enumerate((x, y, z) for x in (0, 63) for y in (0, 63) for z in (0, 63)):
            (one if (i + j) & 1 else two)[l] = F.pack(-3 + j, 4 + i)
        cur[key], ref[key] = one.reshape(-1), two.reshape(-1)
    del ref[(0, 0, -1)], cur[(-1, -1, 0)]
    return cur, ref


def _changes_pose():
    cur, ref = CS.pose_maps()
    return dict(kind="changes", first=cur, second=ref, pose=_fuse_pose(S.rot(4, -2, 3, (13.0, -7.4, 4.2)), (32 * RES, 64 * RES, 32 * RES)))


SCENES = {
    "fuse_translation": _fuse_translation,
    "fuse_general": _fuse_general,
    "fuse_grow": _fuse_grow,
    "coarsen_mixed": _coarsen_mixed,
    "coarsen_eight_1": lambda: dict(kind="coarsen", first=_once("eight", _eight), second={}, keys=None, min_observed=1),
    "coarsen_eight_8": lambda: dict(kind="coarsen", first=_once("eight", _eight), second={}, keys=None, min_observed=8),
    "coarsen_listed": _coarsen_listed,
    "changes_scene": lambda: dict(kind="changes", first=CS.scene()["cur"], second=CS.scene()["ref"], pose=F.identity_pose()),
    "changes_corner": lambda: dict(kind="changes", first=corner_case()[0], second=corner_case()[1], pose=F.identity_pose()),
    "changes_pose": _changes_pose,
}
# the pairs with a default pool allocate 256 MiB per segment: one scene of each call there
DEFAULT_POOL_SCENES = ("fuse_translation", "coarsen_mixed", "changes_corner")


def scene(name):
    return _once("scene " + name, SCENES[name])


def cases(kind):
    """the (pair, scene name) combinations of one call"""
    return [(pair, name) for pair in PAIRS for name in SCENES if name.startswith(kind) and (0 not in pair or name in DEFAULT_POOL_SCENES)]


def want(name, second=None):
    """the model's result of a scene, computed once: fuse (chunks, stats), coarsen (chunks, stats), changes (records, labels, table,
    stats).  second: other chunks of the second store than the scene's (a fuse into a padded DST)"""
    s = scene(name)
    if second is not None:
        return F.fuse(second, s["first"], s["pose"], RES, MW, FILL)

    def make():
        if s["kind"] == "fuse":
            return F.fuse(s["second"], s["first"], s["pose"], RES, MW, FILL)
        if s["kind"] == "coarsen":
            return CM.coarsen(s["second"], s["first"], s["keys"], s["min_observed"], FILL)
        return M.changes(s["first"], s["second"], s["pose"], RES, CS.BAND, CS.FREE, 1, None, None, M.APPEARED | M.VANISHED | M.CLUSTERS)
    return _once("want " + name, make)


def volume(name):
    """how much of a scene the comparison rests on: voxels averaged or set (fuse), voxels valued (coarsen), the larger of the
    records and the voxels known on both sides (changes)"""
    w = want(name)
    if scene(name)["kind"] == "fuse":
        return int(w[1][2]) + int(w[1][3])
    if scene(name)["kind"] == "coarsen":
        return int(w[1][2])
    return max(len(w[0]), int(w[3][1]))


def read_store(name):
    """the chunks of the store a wrong shift would be seen on: SRC of a fuse or a coarsen (the first store), REF of changes (the
    second); with ("first" | "second", the other one)"""
    return ("second", "first") if scene(name)["kind"] == "changes" else ("first", "second")


def seeds(name):
    """the seeds of the two histories of a scene (different for the two stores)"""
    i = sorted(SCENES).index(name)
    return 11 + 2 * i, 12 + 2 * i


def pyramid_case():
    """the sphere-and-floor map with a lone chunk at (5, -3, 2), and the model's three levels over it (the case of
    test_gpu_store_coarsen.py)"""
    def make():
        base = dict(S.sphere_and_floor())
        base[(5, -3, 2)] = observed(61)
        return dict(base=base, levels=CM.pyramid(base, 3, 8, FILL))
    return _once("pyramid", make)


# ------------------------------------------------------------------------------------------------ coarsen at the ends of the keys
IMAX, IMIN = 2 ** 31 - 1, -2 ** 31
KEY_END_KEYS = [(IMAX, IMIN, 0), (IMAX - 1, IMIN, 0), (IMIN, IMAX, -1), (-1, -1, -1), (0, 0, 0)]
# parents whose children 2 k + {0, 1} all lie beyond int32 in x.  The last two are chosen so that the children's keys, cast to int32
# without the range check, wrap onto chunks SRC holds: (IMAX - 1, IMIN, 0) and (IMAX, IMIN, 0), and (IMIN, IMAX, -1)
KEY_END_LISTED = [(2 ** 30, 0, 0), (-2 ** 30 - 1, 0, 0), (-2 ** 30 - 1, -2 ** 30, 0), (2 ** 30, 2 ** 30 - 1, -1)]


def key_end_source():
    return _once("key ends", lambda: {key: observed(80 + i) for i, key in enumerate(KEY_END_KEYS)})


def wrapped_children(key):
    """the children of `key` as a cast to int32 without a range check would name them"""
    wrap = lambda v: (v + 2 ** 31) % 2 ** 32 - 2 ** 31
    return [tuple(wrap(2 * key[a] + ((c >> (2 - a)) & 1)) for a in range(3)) for c in range(8)]


# ------------------------------------------------------------------------------------------------ the long coarsen plan
TABLE_WORDS, ROW_WORDS, PLAN_ROWS = 8192, 12, 700  # STORE_TABLE_WORDS, COARSEN_ROW; 700 rows are 8400 words
PLAN_FIXED_ROWS = (0, 681, 682, 683, 699)


def plan_rows():
    """the eight rows of the 700-row plan that have a child, ascending: the fixed ones and three drawn"""
    rng = np.random.default_rng(8192)
    free = [i for i in range(2, PLAN_ROWS - 2) if all(abs(i - f) > 2 for f in PLAN_FIXED_ROWS)]
    drawn = []
    while len(drawn) < 3:
        i = int(rng.choice(free))
        if all(abs(i - v) > 2 for v in drawn):
            drawn.append(i)
    return sorted(PLAN_FIXED_ROWS + tuple(drawn))


def plan_child(row, j):
    """the one child chunk of parent (row, 0, 0) in SRC: octant j & 7, so the eight rows use all eight places of a plan row"""
    return (2 * row + ((j >> 2) & 1), (j >> 1) & 1, j & 1)
