"""ws_store_fuse, ws_store_coarsen, ws_store_changes and MapPyramid on two stores of UNLIKE pools and histories: different chunks per
segment on the two sides (the default of 256 among them), chunks put in a shuffled order between decoys, overwritten, dropped and put
again, so that a slot says nothing about a key's rank and the two stores need different address arithmetic (two_store_scenes.py;
test_two_store_host.py shows on the host what a swapped shift would read).  Every comparison is bit for bit against the numpy models,
which know nothing of slots or segments."""
import numpy as np
import pytest

import changes_model as M
import changes_scenes as CS
import coarsen_model as CM
import fuse_model as F
import fuse_scenes as S
import two_store_scenes as T
from fuse_scenes import MW, RES

pytestmark = pytest.mark.gpu

ids = lambda v: str(v).replace(" ", "")


def stores(pair, name):
    """the two aged stores of a scene, their claims asserted on the device's own pointers"""
    s = T.scene(name)
    out = []
    for which, geometry, seed in (("first", pair[0], T.seeds(name)[0]), ("second", pair[1], T.seeds(name)[1])):
        store, record = T.aged_store(s[which], geometry, seed)
        print(name, which, "segment_chunks", geometry, {k: v for k, v in record.items() if k not in ("freed", "directory")})
        T.check_record(record, len(s[which]), geometry)
        out += [store, record]
    return s, out[0], out[2], out[1], out[3]


@pytest.mark.parametrize("pair,name", [c for c in T.cases("fuse") if c[1] != "fuse_grow"], ids=ids)
def test_fuse(pair, name):
    s, src, dst, _, _ = stores(pair, name)
    want = T.want(name)
    # a count-only run first: the real call's statistics, DST untouched
    st = dst.fuse(src, s["pose"], MW, count_only=True, resolution=RES)
    assert st.as_tuple() == tuple(int(v) for v in want[1]) and F.same((S.read(dst), ()), (s["second"], ()))
    st = dst.fuse(src, s["pose"], MW, resolution=RES)
    assert st.as_tuple() == tuple(int(v) for v in want[1]), (st, want[1])
    assert F.same((S.read(dst), st.as_tuple()), want) and st.averaged + st.set >= 1000
    assert F.same((S.read(src), ()), (s["first"], ()))  # SRC is only read
    src.close(), dst.close()


@pytest.mark.parametrize("pair", [p for p in T.PAIRS if 0 not in p], ids=ids)
def test_fuse_that_adds_a_segment_to_dst(pair):
    """DST has no unused slot left: the chunk the call creates needs a new segment, so the write pass runs on a segment table that
    was replaced inside the call, while it rewrites chunks of the segments before"""
    name = "fuse_grow"
    s, src, dst, _, record = stores(pair, name)
    pad = S.draw(77, False)
    padded = dict(s["second"])
    for i in range(dst.capacity() - dst.count()):
        padded[((1 << 21) + i, 3, -3)] = pad
        dst.put_chunk(((1 << 21) + i, 3, -3), pad)
    before = dst.capacity()
    assert dst.count() == before == record["segments"] << T.shift_of(pair[1])
    want = T.want(name, second=padded)
    st = dst.fuse(src, s["pose"], MW, resolution=RES)
    got = S.read(dst)
    assert st.as_tuple() == tuple(int(v) for v in want[1]) and st.created >= 1 and dst.capacity() > before
    assert F.same((got, st.as_tuple()), want) and F.same((S.read(src), ()), (s["first"], ()))
    assert sum(not np.array_equal(got[k], s["second"][k]) for k in s["second"]) >= 2  # chunks of the earlier segments were rewritten
    src.close(), dst.close()


@pytest.mark.parametrize("pair,name", T.cases("coarsen"), ids=ids)
def test_coarsen(pair, name):
    from warpsense_amd._abi import _i3c
    s, src, dst, _, record = stores(pair, name)
    want, want_stats = T.want(name)
    st = src.coarsen(dst, s["keys"], s["min_observed"])
    print("stats", st, "model", want_stats)
    assert st.as_tuple() == tuple(want_stats) and st.valued >= 1000
    assert CM.same(S.read(dst), want)
    assert CM.same(S.read(src), s["first"])  # SRC is only read
    if name == "coarsen_listed":  # the created chunk lies in a slot another chunk has left
        assert st.created == 1 and dst._L.ws_store_chunk_dev(dst.handle, _i3c((2, 2, 2))) in record["freed"]
    src.close(), dst.close()


@pytest.mark.parametrize("pair,name", T.cases("changes"), ids=ids)
def test_changes(pair, name):
    s, cur, ref, _, _ = stores(pair, name)
    want = T.want(name)
    got = cur.changes(ref, s["pose"], resolution=RES, band=CS.BAND, free_value=CS.FREE, min_weight=1, kinds="both", clusters=True)
    assert got.stats.as_tuple() == tuple(int(v) for v in want[3]), (got.stats, want[3])
    assert M.same((got.records, got.labels, got.clusters, got.stats.as_tuple()), want)
    assert F.same((S.read(cur), ()), (s["first"], ())) and F.same((S.read(ref), ()), (s["second"], ()))  # both are only read
    cur.close(), ref.close()


class TestPyramid:
    def test_levels_of_the_default_pool_over_an_aged_base_of_one_chunk_segments(self):
        import warpsense_amd as W
        import store_scenes as SM
        g = T.pyramid_case()
        read_levels = lambda p: [S.read(p.store(l)) for l in range(p.levels + 1)]
        base, record = T.aged_store(g["base"], 1, 41)
        T.check_record(record, len(g["base"]), 1)
        p = W.MapPyramid(base, 3, RES)
        stats = p.rebuild()
        for l, (got, want) in enumerate(zip(read_levels(p), g["levels"])):
            assert CM.same(got, want), l
        assert [s.chunks for s in stats] == [len(g["levels"][l]) for l in (1, 2, 3)] and stats[0].valued > 1000
        assert p.store(1).capacity() == 256 and base.capacity() == record["segments"]
        vert, face = p.store(2).mesh(p.resolution(2))
        mv, mf = SM.model_store(g["levels"][2], 4 * RES)
        assert vert.tobytes() == mv.tobytes() and face.tobytes() == mf.tobytes() and len(vert) > 20
        p.close(), base.close()

    def test_global_pyramid_with_its_default_pool_over_a_mapping_store_of_two_chunk_segments(self):
        """TSDFMapping.global_pyramid as a run without arguments gets it: the levels in the default pool, the store of the mapping in
        segments of two chunks; after a shift and another scan the refreshed pyramid is the model's again"""
        import warpsense_amd as W
        import store_scenes as SM
        from window_routes import _params
        size = (65, 65, 65)
        store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
        tm = W.TSDFMapping(_params(size), W.LocalMap(*size, SM.TAU, 0), device_global_map=store)
        fill = int(W.pack_entry(SM.TAU, 0))
        tm.update_tsdf(SM.walk_scan(0), pos_rm=SM.WALK[0], up_rm=(0, 0, 32768))
        p = tm.global_pyramid(2, min_observed=4)
        want = CM.pyramid(S.read(store), 2, 4, fill)
        assert CM.same(S.read(p.store(1)), want[1]) and CM.same(S.read(p.store(2)), want[2]) and len(want[1]) > 0
        assert p.store(1).capacity() == 256 and store.capacity() % 2 == 0 and store.capacity() < 256
        tm.shift_map_device(SM.WALK[1])
        tm.update_tsdf(SM.walk_scan(1), pos_rm=SM.WALK[1], up_rm=(0, 0, 32768))
        assert tm.global_pyramid(2, min_observed=4) is p
        want = CM.pyramid(S.read(store), 2, 4, fill)
        assert CM.same(S.read(p.store(1)), want[1]) and CM.same(S.read(p.store(2)), want[2])
        vert, face = tm.global_mesh(level=1)
        mv, mf = SM.model_store(want[1], 2 * SM.RES)
        assert vert.tobytes() == mv.tobytes() and face.tobytes() == mf.tobytes()
        p.close(), store.close()
