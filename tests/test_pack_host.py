"""CPU tests of the packed form of the store's chunks (ws_store_pack, include/warpsense_hip.h): the numpy model (pack_model.py) against
the host-only calls ws_pack_chunk / ws_pack_expand_chunk byte for byte on the brick cases, ws_pack_check against single corruptions
and a stream beyond 2^32 words, the PackedMap file, the route to and from a host GlobalMap, and the declarations.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pack_model as PM
import pack_scenes as PS
import query_model as QM
import warpsense_amd as W
from warpsense_amd import _lib
from warpsense_amd._abi import _i3c, _ptr

CASES = PM.brick_cases()


def c_pack(chunk, key, fill, cap=PM.CW):
    L = _lib.load()
    header, own, words = np.full(PM.HDR, 0xDEADBEEF, dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32), C.c_uint64(0)
    rc = L.ws_pack_chunk(_ptr(np.ascontiguousarray(chunk)), _i3c(key), int(fill), _ptr(header), _ptr(own), cap, C.byref(words))
    return rc, header, own[:min(int(words.value), cap)], int(words.value)


def c_expand(header, own, fill):
    out = np.zeros(PM.CW, dtype=np.uint32)
    own = np.ascontiguousarray(own, dtype=np.uint32)
    assert _lib.load().ws_pack_expand_chunk(_ptr(np.ascontiguousarray(header)), _ptr(own) if own.size else None, int(fill), _ptr(out)) == 0
    return out


def c_check(headers, words):
    headers = np.ascontiguousarray(headers, dtype=np.uint32)
    return _lib.load().ws_pack_check(_ptr(headers), int(headers.shape[0]), int(words))


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_and_host_calls_agree_byte_for_byte(name):
    chunk, key = CASES[name], PM.CASE_KEYS[name]
    want_h, want_own = PM.pack_chunk(chunk, key, PM.FILL)
    rc, header, own, words = c_pack(chunk, key, PM.FILL)
    assert rc == 0 and words == len(want_own) and header.tobytes() == want_h.tobytes() and own.tobytes() == want_own.tobytes()
    # the round trip, with the fill of the pack and with another: only the default bricks follow it
    assert c_expand(header, own, PM.FILL).tobytes() == chunk.tobytes() == PM.expand(want_h, want_own, PM.FILL).tobytes()
    other_fill = np.uint32(0x12345678)
    again = c_expand(header, own, other_fill)
    assert again.tobytes() == PM.expand(want_h, want_own, other_fill).tobytes()
    is_default = np.repeat(PM.classes(chunk, PM.FILL) == 0, 512)
    assert (PM.bricks(again).reshape(-1)[is_default] == other_fill).all() and (PM.bricks(again).reshape(-1)[~is_default] == PM.bricks(chunk).reshape(-1)[~is_default]).all()


def test_the_cases_hold_what_their_names_say():
    k = {name: PM.classes(c, PM.FILL) for name, c in CASES.items()}
    assert (k["all_fill"] == 0).all() and (k["one_word"] == 1).all()
    for name in ("single_first", "single_last"):
        assert k[name][[0, 511]].tolist() == [2, 2] and int((k[name] != 0).sum()) == 2
    assert k["but_last"][[77, 78]].tolist() == [2, 1]
    assert k["word0_fill"][[5, 300]].tolist() == [2, 2]
    assert k["neighbours"][160:168].tolist() == [2, 1, 2, 0, 0, 0, 2, 1] and k["neighbours"][504:506].tolist() == [1, 2]
    assert (k["random"] == 2).all()
    assert all(int((k["two_words"] == c).sum()) > 100 for c in (0, 1, 2))
    assert len(CASES) == 12 == PM.N_CASES and len(set(PM.CASE_KEYS.values())) == 12 and sorted(PM.CASE_KEYS) == sorted(CASES)
    # the odd word of the 512 bricks is each of the 512 word numbers once
    rows, odd = np.arange(512), PM.odd_word(np.arange(512))
    assert sorted(odd.tolist()) == list(range(512)) and [PM.odd_word(b) for b in (0, 1, 511)] == [61, 258, (197 * 511 + 61) % 512]
    for name, flat, masked_class in (("odd_in_fill", PM.FILL, 0), ("odd_in_uniform", PM.OTHER, 1)):
        b = PM.bricks(CASES[name])
        assert (k[name] == 2).all()
        # exactly one word of every brick is unlike its other 511, which are all alike: it is word odd_word(b)
        assert ((b != flat).sum(axis=1) == 1).all() and (b[rows, odd] != flat).all()
        # with that one word masked the class is 0 resp. 1, for every brick: each of the 512 positions decides one brick's class
        masked = b.copy()
        masked[rows, odd] = flat
        assert (PM.classes(PM.unbricks(masked), PM.FILL) == masked_class).all()
        for w in (0, 7, 8, 63, 64, 448, 511):  # ... and a model blind to ONE word number gets exactly the brick that owns it wrong
            blind = b.copy()
            blind[:, w] = b[:, (w + 1) % 512]
            wrong = np.flatnonzero(PM.classes(PM.unbricks(blind), PM.FILL) != 2)
            assert wrong.tolist() == [int(np.flatnonzero(odd == w)[0])], (name, w, wrong)
    halves = {brick: (w, bit) for brick, w, bit in PM.HALVES}
    assert sorted(halves) == [168, 170, 171, 173] and len({brick >> 3 for brick in halves}) == 1  # one brick column
    assert k["halves"][sorted(halves)].tolist() == [2, 2, 1, 1] and int((k["halves"] != 0).sum()) == 4
    b = PM.bricks(CASES["halves"])
    for brick, (w, bit) in halves.items():
        unlike = np.flatnonzero(b[brick] != PM.FILL)
        assert unlike.tolist() == ([w] if w is not None else list(range(512))) and set((b[brick][unlike] ^ PM.FILL).tolist()) == {1 << bit}
    assert sorted({bit for _, bit in halves.values()}) == [0, 31] and {(w is None, bit) for w, bit in halves.values()} == {(a, c) for a in (False, True) for c in (0, 31)}


def test_capacity_of_pack_chunk():
    chunk = CASES["neighbours"]
    _, own = PM.pack_chunk(chunk, (0, 0, 1), PM.FILL)
    rc, header, _, words = c_pack(chunk, (0, 0, 1), PM.FILL, cap=len(own) - 1)
    assert rc == -4 and words == len(own) and header[4] == 4 and header[3] == 3  # WS_ERR_CAPACITY: the size and the header are told
    assert c_pack(chunk, (0, 0, 1), PM.FILL, cap=len(own))[0] == 0


def model_stream():
    return PM.pack(PM.case_store(), PM.FILL)


def test_check_accepts_the_model_and_refuses_each_corruption():
    headers, payload, stats = model_stream()
    assert c_check(headers, len(payload)) == 0 and c_check(headers[:0], 0) == 0
    assert stats[0] + stats[1] + stats[2] == 512 * len(headers) and stats[3] == 4 * (headers.size + payload.size)
    i = next(j for j in range(len(headers) - 1) if headers[j][3] + headers[j][4] > 0)  # a chunk with payload that is not the last one

    def broken(name):
        h = headers.copy()
        if name == "swapped keys":
            h[[i, i + 1], 0:3] = h[[i + 1, i], 0:3]
        elif name == "equal key twice":
            h[i + 1, 0:3] = h[i, 0:3]
        elif name == "class code 3":
            h[i, 8] |= 3
        elif name == "count off by one":
            h[i, 3 if h[i, 3] else 4] -= 1
        elif name == "offset off by one":
            h[i + 1, 5] += 1
        elif name == "word 7 set":
            h[i, 7] = 1
        return h
    for name in ("swapped keys", "equal key twice", "class code 3", "count off by one", "offset off by one", "word 7 set"):
        assert c_check(broken(name), len(payload)) == -1, name
        assert name.split()[0] in ("swapped", "equal") or b"chunk " in _lib.load().ws_last_error()
    assert c_check(headers, len(payload) + 1) == -1 and c_check(headers, len(payload) - 1) == -1  # a wrong total
    # a count off by one that the offsets follow is still refused: the counts are held to the class map
    h = headers.copy()
    h[i, 4] += 1
    for j in range(i + 1, len(h)):
        first = (int(h[j, 5]) | int(h[j, 6]) << 32) + 512
        h[j, 5], h[j, 6] = first & 0xFFFFFFFF, first >> 32
    assert c_check(h, len(payload) + 512) == -1


def test_check_carries_offsets_beyond_2_to_the_32_words():
    """20 000 chunks of 512 dense bricks: 5.2e9 payload words; the headers alone are 3.2 MB"""
    n = 20000
    h = np.zeros((n, PM.HDR), dtype=np.uint32)
    h[:, 0] = np.arange(n, dtype=np.int32).view(np.uint32)
    h[:, 4] = 512
    h[:, 8:] = 0xAAAAAAAA
    first = np.arange(n, dtype=np.uint64) * np.uint64(512 * 512)
    h[:, 5], h[:, 6] = (first & np.uint64(0xFFFFFFFF)).astype(np.uint32), (first >> np.uint64(32)).astype(np.uint32)
    total = n * 512 * 512
    assert total > 2 ** 32 and int(h[-1, 6]) == 1 and c_check(h, total) == 0
    assert c_check(h, total & 0xFFFFFFFF) == -1  # the total is not taken modulo 2^32 ...
    bad = h.copy()
    bad[-1, 6] = 0  # ... and neither is an offset
    assert c_check(bad, total) == -1
    p = W.PackedMap(h, np.zeros(0, np.uint32), 0)
    assert int(p.offsets[-1]) == (n - 1) * 512 * 512


def test_the_scene_of_many_chunks_is_what_the_model_packs():
    """the stamped stream of pack_scenes equals PM.pack chunk by chunk (N = 130), its keys are spread, its cases weighted"""
    sc = PS.scene(130)
    made = PS.scene_keys(130)
    assert sorted(made) == sc["keys"] and made != sc["keys"] and all(end in made for end in PS.KEY_ENDS) and min(min(k) for k in made[:20]) < 0
    headers, payload, stats = PS.stream(sc)
    want = PM.pack(sc["chunks"], PM.FILL)
    assert headers.tobytes() == want[0].tobytes() and payload.tobytes() == want[1].tobytes() and stats == want[2]
    sub = sc["keys"][1::2]
    hs, ps, ss = PS.stream(sc, sub[::-1])
    want = PM.pack(sc["chunks"], PM.FILL, sub)
    assert hs.tobytes() == want[0].tobytes() and ps.tobytes() == want[1].tobytes() and ss == want[2]
    for n in (130, 1030):
        names = [PS.case_of(i) for i in range(n)]
        assert set(names) == set(CASES) and sum(name in PS.CHEAP for name in names) >= 0.9 * n
        assert all(names[i] in ("random", "two_words") for i in range(19, n, 20)) and names.count("odd_in_fill") >= 2 <= names.count("odd_in_uniform")


def test_check_accepts_a_stream_of_1030_chunks_and_chunks_expand_to_their_source():
    sc = PS.scene(1030)
    headers, payload, stats = PS.stream(sc)
    n = len(headers)
    assert n == 1030 and c_check(headers, len(payload)) == 0 and 10e6 < 4 * len(payload) < 100e6
    assert c_check(headers[:1025], int(headers[1025, 5]) | int(headers[1025, 6]) << 32) == 0 and c_check(headers, len(payload) - 1) == -1
    p = W.PackedMap(headers, payload, int(PM.FILL))
    assert p.stats == tuple(stats) and p.keys == sc["keys"]
    for i in (0, 63, 64, 1023, 1024, n - 1):
        assert p.chunk(i).tobytes() == sc["chunks"][sc["keys"][i]].tobytes(), i


def test_packed_map_file_round_trip(tmp_path):
    headers, payload, stats = model_stream()
    p = W.PackedMap(headers, payload, int(PM.FILL), resolution=64, tau=600)
    assert p.stats == tuple(stats) and p.n_chunks == 12 and p.keys == sorted(PM.case_store()) and not p.on_device
    assert p.ratio == pytest.approx(stats[3] / (12 * 4 * PM.CW)) and 0 < p.ratio < 1
    path = str(tmp_path / "map.wspk")
    p.save(path, note="a test")
    q = W.PackedMap.load(path)
    assert q.headers.tobytes() == headers.tobytes() and q.payload.tobytes() == payload.tobytes() and q.fill == int(PM.FILL)
    assert (q.resolution, q.tau, str(q.meta["note"])) == (64, 600, "a test") and q.stats == p.stats
    with np.load(path) as z:  # a plain uncompressed savez under the name given
        assert sorted(z.files) == sorted(["version", "fill", "headers", "payload", "resolution", "tau", "note"]) and int(z["version"]) == 1
    import zipfile
    assert all(i.compress_type == zipfile.ZIP_STORED for i in zipfile.ZipFile(path).infolist())
    # a file whose stream is broken does not load
    bad = W.PackedMap(headers, payload[:-1], int(PM.FILL))
    bad.save(str(tmp_path / "bad.wspk"))
    with pytest.raises(W.WsError):
        W.PackedMap.load(str(tmp_path / "bad.wspk"))
    for i, key in enumerate(q.keys):
        assert q.chunk(i).tobytes() == PM.case_store()[key].tobytes()


def test_to_and_from_a_host_global_map():
    chunks = PM.case_store()
    value, weight = (int(v) for v in W.unpack_entry(PM.FILL))
    g = W.GlobalMap(value, weight)
    for key, c in chunks.items():
        g.activate_chunk(*key)[:] = c
    p = W.PackedMap.from_global_map(g)
    headers, payload, stats = model_stream()
    assert p.headers.tobytes() == headers.tobytes() and p.payload.tobytes() == payload.tobytes() and p.stats == tuple(stats) and p.fill == int(PM.FILL)
    p.check()
    sub = [(5, 5, 5), (0, 0, 0)]
    ps = W.PackedMap.from_global_map(g, keys=sub)
    hs, pl, _ = PM.pack(chunks, PM.FILL, sub)
    assert ps.headers.tobytes() == hs.tobytes() and ps.payload.tobytes() == pl.tobytes()
    with pytest.raises(W.WsError):
        W.PackedMap.from_global_map(g, keys=[(9, 9, 9)])
    # into a map with another default: the listed chunks are the source's bytes, a chunk that is not listed keeps its own
    h = W.GlobalMap(-77, 3)
    h.activate_chunk(1, 2, 3)[:] = 5
    h.activate_chunk(0, 0, 1)[:] = 6
    p.to_global_map(h)
    assert sorted(h.chunks) == sorted(list(chunks) + [(1, 2, 3)]) and (h.chunks[(1, 2, 3)] == 5).all()
    for key, c in chunks.items():
        assert h.chunks[key].tobytes() == c.tobytes(), key


def test_symbols_are_declared_bound_and_exported():
    L = _lib.load()
    names = {"ws_store_pack": 7, "ws_store_pack_headers_dev": 2, "ws_store_pack_payload_dev": 2, "ws_store_pack_download": 7, "ws_store_unpack": 7,
             "ws_store_unpack_dev": 7, "ws_pack_check": 3, "ws_pack_expand_chunk": 4, "ws_pack_chunk": 7, "ws_debug_store_pack_timing": 3}
    for name, n_params in names.items():
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        ret, params = QM._declared(name)
        assert len(params) == n_params and len(getattr(L, name).argtypes) == n_params, (name, params)
    assert QM._declared("ws_store_pack")[1] == ["ws_store *", "const int32_t *", "size_t", "uint32_t", "size_t *", "uint64_t *", "uint64_t [4]"]
    assert QM._declared("ws_store_unpack")[1] == ["ws_store *", "const uint32_t *", "const uint32_t *", "size_t", "uint64_t", "uint32_t", "uint32_t"]
    assert QM._declared("ws_store_unpack_dev")[1] == QM._declared("ws_store_unpack")[1]
    assert QM._declared("ws_pack_chunk")[1] == ["const uint32_t *", "const int32_t [3]", "uint32_t", "uint32_t *", "uint32_t *", "uint64_t", "uint64_t *"]
    header = QM._header()
    assert "#define WS_PACK_HEADER_WORDS 40" in header and _lib.WS_PACK_HEADER_WORDS == 40 == PM.HDR
    assert "#define WS_PACK_DEFAULT 0u" in header and "#define WS_PACK_EMIT_DIRECT 1u" in header and (_lib.WS_PACK_DEFAULT, _lib.WS_PACK_EMIT_DIRECT) == (0, 1)
