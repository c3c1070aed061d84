"""CPU tests of ws_store_coarsen's rule and of ws_store_parents_of: the host entry point against the numpy model (coarsen_model.py),
the properties of the model itself, and the declaration of the entry points.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import coarsen_model as CM
import query_model as QM
from warpsense_amd import _lib

WS_OK, WS_ERR_INVALID = 0, -1


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_parents(keys, capacity=None):
    """(status, the copied prefix, the reported count) of the C entry point itself"""
    L = _lib.load()
    k = np.ascontiguousarray(np.asarray(keys, dtype=np.int32).reshape(-1, 3))
    n = C.c_size_t(12345)
    cap = len(k) if capacity is None else capacity
    out = np.full((max(cap, 1), 3), 77, dtype=np.int32)
    rc = L.ws_store_parents_of(_p(k) if len(k) else None, len(k), _p(out) if cap else None, cap, C.byref(n))
    return rc, out[:min(cap, n.value)], n.value


def test_parents_of_negative_components():
    """-1 -> -1, -3 -> -2, 1 -> 0: the arithmetic shift, floor(k / 2)"""
    rc, got, n = raw_parents([(-1, -3, 1)])
    assert rc == WS_OK and n == 1 and got.tolist() == [[-1, -2, 0]]
    keys = [(-1, -1, -1), (-3, 2, -2), (1, 0, 0), (2, 0, 0), (0, 0, 0), (-2, -2, -2), (-4, 5, -5)]
    rc, got, n = raw_parents(keys)
    want = CM.parents_of(keys)
    assert rc == WS_OK and n == len(want) and np.array_equal(got, want)
    assert [tuple(r) for r in got.tolist()] == sorted(tuple(r) for r in got.tolist())  # ascending (cx, cy, cz)
    assert (-2, 1, -1) in [tuple(r) for r in got.tolist()] and (0, 0, 0) in [tuple(r) for r in got.tolist()] and (1, 0, 0) in [tuple(r) for r in got.tolist()]


def test_parents_of_duplicates_capacity_and_far_keys():
    rng = np.random.default_rng(3)
    keys = rng.integers(-9, 10, (500, 3))
    keys = np.concatenate([keys, keys[:100]])  # duplicates
    want = CM.parents_of(keys)
    rc, got, n = raw_parents(keys)
    assert rc == WS_OK and n == len(want) < 500 and np.array_equal(got, want)
    # a capacity smaller than the count: the prefix, and still the count
    rc, got, n = raw_parents(keys, capacity=7)
    assert rc == WS_OK and n == len(want) and np.array_equal(got, want[:7])
    rc, got, n = raw_parents(keys, capacity=0)
    assert rc == WS_OK and n == len(want) and len(got) == 0
    # keys at +-2^25 (the chunks of voxels near +-2^31)
    far = [(1 << 25, -(1 << 25), (1 << 25) - 1), (-(1 << 25), (1 << 25) - 1, -(1 << 25) + 1), ((1 << 25) - 1, -(1 << 25) + 1, 1 << 25)]
    rc, got, n = raw_parents(far)
    assert rc == WS_OK and np.array_equal(got, CM.parents_of(far)) and n == 3
    assert [1 << 24, -(1 << 24), (1 << 24) - 1] in got.tolist() and [-(1 << 24), (1 << 24) - 1, -(1 << 24)] in got.tolist()
    # no keys at all; refusals
    rc, got, n = raw_parents(np.zeros((0, 3)))
    assert rc == WS_OK and n == 0
    L = _lib.load()
    k = np.zeros((1, 3), dtype=np.int32)
    assert L.ws_store_parents_of(None, 1, _p(k), 1, None) == WS_ERR_INVALID and L.ws_last_error().decode().startswith("ws_store_parents_of:")
    assert L.ws_store_parents_of(_p(k), 1, None, 1, None) == WS_ERR_INVALID
    assert L.ws_store_parents_of(_p(k), 1, _p(k), 1, None) == WS_OK  # n_out may be NULL


def test_python_parents_of_is_the_model():
    import warpsense_amd as W
    keys = [(-1, -1, -1), (-3, 2, -2), (1, 0, 0), (2, 0, 0), (1, 0, 0)]
    got = W.parents_of(keys)
    assert got.dtype == np.int32 and np.array_equal(got, CM.parents_of(keys))
    assert W.parents_of(np.zeros((0, 3), dtype=np.int32)).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the model's own properties
FILL = int(CM.pack(600, 0))


def test_constant_field_stays_constant():
    src = {(0, 0, 0): np.full(CM.CW, CM.pack(-137, 9), dtype=np.uint32), (1, 1, 1): np.full(CM.CW, CM.pack(-137, 9), dtype=np.uint32)}
    out, stats = CM.coarsen({}, src, None, 8, FILL)
    data = out[(0, 0, 0)].reshape(64, 64, 64)
    assert sorted(out) == [(0, 0, 0)] and np.all(data[:32, :32, :32] == CM.pack(-137, 9)) and np.all(data[32:, 32:, 32:] == CM.pack(-137, 9))
    assert np.all(data[:32, 32:, :] == FILL) and stats == [1, 1, 2 * 32 ** 3, 0]


def test_linear_field_at_the_coarse_centre():
    """d = n . p - c with an integer normal, all children observed, untruncated: the mean of the eight integer values is the field at
    the mean of the eight centres, which is the coarse voxel's centre (2 V + 1) r; the floor takes less than 1 mm off"""
    r, normal, c = 4, np.array([3, -2, 5]), 611
    v = np.stack(np.meshgrid(*(np.arange(64),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    d = (v * r + r // 2) @ normal - c
    assert np.abs(d).max() < 32767
    out, _ = CM.coarsen({}, {(0, 0, 0): CM.pack(d, 5)}, None, 8, FILL)
    V = np.stack(np.meshgrid(*(np.arange(32),) * 3, indexing="ij"), axis=-1)
    centre = ((2 * V + 1) * r) @ normal - c  # the coarse voxel V of edge 2 r has its centre at V 2 r + r
    value, weight = CM.unpack(out[(0, 0, 0)].reshape(64, 64, 64)[:32, :32, :32])
    assert np.all(weight == 5) and np.all(value <= centre) and np.all(centre - value < 1)
    # with odd sums the floor does take something off: a field offset by a half
    out, _ = CM.coarsen({}, {(0, 0, 0): CM.pack(d + (v[:, 2] & 1), 5)}, None, 8, FILL)
    value2, _ = CM.unpack(out[(0, 0, 0)].reshape(64, 64, 64)[:32, :32, :32])
    assert np.all(value2 == value)  # S = 8 d + 4: floor((8 d + 4) / 8) = d


def test_floor_rule_for_a_sum_of_minus_one():
    """S = -1, n = 1 .. 8: floor(-1 / n) = -1 for every n (a truncating division would give 0 from n = 2)"""
    for n in range(1, 9):
        value = np.zeros(8, dtype=np.int64)
        value[0] = -1
        weight = np.where(np.arange(8) < n, 3, 0)
        e, got_n = CM.coarsen_entries(value, weight, 1, FILL)
        assert int(got_n) == n and CM.unpack(e)[0] == -1 and CM.unpack(e)[1] == 3
    # and the two ends of S
    e, _ = CM.coarsen_entries(np.full(8, -32768), np.full(8, 1), 8, FILL)
    assert CM.unpack(e)[0] == -32768
    e, _ = CM.coarsen_entries(np.full(8, 32767), np.full(8, 32767), 8, FILL)
    assert CM.unpack(e) == (32767, 32767)


def test_min_observed_on_three_observed_children():
    value = np.array([10, 20, 31, 999, 999, 999, 999, 999])
    weight = np.array([4, 2, 7, 0, -3, 0, -32768, 0])
    for min_observed, want in [(1, CM.pack(20, 2)), (3, CM.pack(20, 2)), (4, FILL), (8, FILL)]:
        e, n = CM.coarsen_entries(value, weight, min_observed, FILL)
        assert int(n) == 3 and int(e) == int(want), min_observed


def test_weight_is_the_minimum_over_observed_children_only():
    value = np.arange(8)
    weight = np.array([50, -7, 0, 12, 32767, -32768, 13, 40])
    e, n = CM.coarsen_entries(value, weight, 1, FILL)
    assert int(n) == 5 and CM.unpack(e) == ((0 + 3 + 4 + 6 + 7) // 5, 12)


def test_model_chunk_layout_and_listed_keys():
    """the child chunk (1, 0, 1) of parent 0 lands in the octant x >= 32, y < 32, z >= 32; a listed parent without children is not
    created, an existing one becomes fill; an unlisted chunk keeps its bytes"""
    rng = np.random.default_rng(8)
    chunk = CM.pack(rng.integers(-600, 601, CM.CW), rng.integers(1, 50, CM.CW))
    out, stats = CM.coarsen({}, {(1, 0, 1): chunk}, None, 1, FILL)
    data = out[(0, 0, 0)].reshape(64, 64, 64)
    octant = np.zeros((64, 64, 64), dtype=bool)
    octant[32:, :32, 32:] = True
    assert np.all(data[~octant] == FILL) and np.all(CM.unpack(data[octant])[1] > 0) and stats == [1, 1, 32 ** 3, 0]
    v, w = CM.unpack(chunk.reshape(64, 64, 64)[2:4, 6:8, 10:12])
    assert CM.unpack(data[33, 3, 37]) == (int(v.sum()) // 8, int(w.min()))
    old = {(5, 5, 5): chunk, (0, 0, 0): chunk, (9, 9, 9): chunk}
    out, stats = CM.coarsen(old, {(1, 0, 1): chunk}, [(5, 5, 5), (7, 7, 7), (5, 5, 5)], 1, FILL)
    assert sorted(out) == sorted(old) and np.all(out[(5, 5, 5)] == FILL) and np.array_equal(out[(0, 0, 0)], chunk) and stats == [1, 0, 0, 0]


def test_stats_dataclass_and_pyramid_arguments():
    import warpsense_amd as W
    s = W.CoarsenStats(5, 1, 4, 2)
    assert s.as_tuple() == (5, 1, 4, 2) and (s.chunks, s.created, s.valued, s.short) == (5, 1, 4, 2)
    with pytest.raises(ValueError):
        W.MapPyramid(None, 0, 64)


def test_symbols_are_declared_bound_and_exported():
    L = _lib.load()
    for name, n_params in (("ws_store_coarsen", 7), ("ws_store_parents_of", 5), ("ws_debug_store_coarsen_timing", 3)):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        ret, params = QM._declared(name)
        assert ret == "int" and len(params) == n_params and len(getattr(L, name).argtypes) == n_params, (name, params)
    assert QM._declared("ws_store_coarsen")[1] == ["ws_store *", "ws_store *", "const int32_t *", "size_t", "int32_t", "uint32_t", "uint64_t [4]"]
    assert QM._declared("ws_store_parents_of")[1] == ["const int32_t *", "size_t", "int32_t *", "size_t", "size_t *"]
    header = QM._header()
    assert "#define WS_COARSEN_DEFAULT 0u" in header and _lib.WS_COARSEN_DEFAULT == 0
    assert L.ws_version() == 1
    # refusals that need no device: NULL stores
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert L.ws_store_coarsen(None, None, None, 0, 8, 0, stats) == WS_ERR_INVALID and list(stats) == [7, 7, 7, 7]
    assert L.ws_last_error().decode().startswith("ws_store_coarsen:")
    assert L.ws_debug_store_coarsen_timing(None, 0, None) == WS_ERR_INVALID
