"""The C++ drop-in of the reach (tests/cpp/reach_dropin.cpp): MappingNode::reach / global_reach, DeviceGlobalMap::reach / reach_paths and
warpsense::local_map_reach / global_map_reach and their _paths along the walk of test_gpu_store_mesh.test_after_real_use print the counts
and the digests of the bytes the Python route gives; and TSDFMapping.reachable_frontier against the models on a small room with one sealed
pocket, whose frontier cluster must come back unreachable."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import distance_model as DM
import frontier_model as FM
import query_model as QM
import reach_model as RM
import store_scenes as SM
from reach_scenes import sealed_room
from window_routes import _params

pytestmark = pytest.mark.gpu
EDGE = 65
INF = RM.INF


def field_line(cost, info, columns=False):
    ext = list(cost.shape) + [1] * (3 - cost.ndim)
    return [str(cost.size), str(info["seeded"]), str(info["reached"]), *(str(e) for e in ext), "1" if columns else "0", f"{QM.fnv1a(cost.tobytes()):016x}"]


def paths_line(result):
    hdr, rec = result
    return [str(len(hdr)), f"{QM.fnv1a(hdr.tobytes()):016x}", "0" * 16 if rec.size == 0 else f"{QM.fnv1a(rec.tobytes()):016x}"]


def test_cpp_wrappers_give_the_bytes_of_the_python_route(tmp_path):
    import warpsense_amd as W
    scans = [SM.walk_scan(k) for k in range(len(SM.WALK))]
    store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    try:
        tm = W.TSDFMapping(_params((EDGE,) * 3), W.LocalMap(EDGE, EDGE, EDGE, SM.TAU, 0), device_global_map=store)
        for k, pos in enumerate(SM.WALK):
            if k:
                tm.shift_map_device(pos)
            tm.update_tsdf(scans[k], pos_rm=pos, up_rm=(0, 0, 32768))
        exe = build_dropin("reach_dropin", tmp_path)
        np.concatenate(scans).tofile(tmp_path / "scans.bin")
        out = subprocess.run([str(exe), str(tmp_path / "scans.bin"), str(len(scans[0])), str(EDGE), str(SM.RES), str(SM.TAU), str(SM.MW), "2",
                              *(str(c) for pos in SM.WALK for c in pos)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout, out.stderr)
        lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
        pos = np.array(SM.WALK[-1])
        seeds = np.array([pos] + [pos + d * np.eye(3, dtype=np.int64)[k] for k in range(3) for d in (-2, 2)])
        goals = np.array([pos + (5, 5, 0), pos + (-8, 3, 1), pos + (0, -12, 2), pos + (1000, 0, 0), pos], dtype=np.int32)
        seed_mm, one_voxel = seeds * SM.RES, SM.RES / 1000.0
        avg = tm.tsdf().avg_map()
        cost = tm.reach(seed_mm=seed_mm, clearance_m=one_voxel)
        assert tm.last_reach["seeded"] >= 1 and tm.last_reach["reached"] > 1000 and cost.shape == (EDGE,) * 3
        assert lines["window"] == field_line(cost, tm.last_reach)
        hdr, rec = avg.reach_paths(goals, 48)
        assert 0 in hdr["status"] and hdr["status"][3] == 2 and lines["window_paths"] == paths_line((hdr, rec))
        assert lines["window_costs"] == paths_line(avg.reach_paths(goals, 0))
        cols = tm.reach(seed_mm=seed_mm, lo=pos - (20, 20, 3), hi=pos + (25, 12, 3), unknown_free=True, columns=True)
        assert cols.shape == (46, 33) and lines["window_columns"] == field_line(cols, tm.last_reach, True)
        again = avg.reach(seeds)
        assert lines["window_again"] == field_line(again, avg.last_reach, True)
        whole = tm.global_reach(seed_mm=seed_mm, clearance_m=one_voxel, lo=pos - (30, 30, 12), hi=pos + (40, 30, 12))
        assert tm.last_reach["reached"] > 1000 and lines["global"] == field_line(whole, tm.last_reach)
        assert lines["chunks"] == [str(store.count())]
        assert lines["global_paths"] == paths_line(store.reach_paths(goals, 48))
        free = store.reach(seeds, unknown_free=True)
        assert store.last_reach["reached"] > tm.last_reach["reached"] and lines["global_free"] == field_line(free, store.last_reach)
        assert lines["global_free_paths"] == paths_line(store.reach_paths(goals, 16))
    finally:
        store.close()


def test_reachable_frontier_of_a_room_with_a_sealed_pocket():
    import warpsense_amd as W
    box = sealed_room()
    size = box.shape
    lm = W.LocalMap(*size, FM_TAU, 0)
    tm = W.TSDFMapping(_params(size), lm)
    lo, hi = QM.window(size, (0, 0, 0))
    tm.tsdf().avg_map().insert_box(lo, hi, box.reshape(-1))
    res = int(tm.params_.map.resolution)
    seed = lo + (5, 5, 4)
    # the models: frontier with clusters, distance with the range of a one-voxel clearance, reach, lookup at every record
    rec, labels, table = FM.frontier(box, lo)
    dist, _ = DM.model_box(box, 2)
    cost, kept, _ = RM.field(dist, lo, [seed], 1)
    at = RM.lookup(cost, lo, np.stack([rec["x"], rec["y"], rec["z"]], axis=1))
    best = np.array([at[labels == c].min() for c in range(len(table))], dtype=np.uint32)
    pocket = [c for c in range(len(table)) if table["lo"][c][0] >= lo[0] + 15 and table["hi"][c][1] <= lo[1] + 6]
    assert kept == 1 and len(table) == 3 and len(pocket) == 1 and best[pocket[0]] == INF and np.all(np.delete(best, pocket) != INF)
    got = tm.reachable_frontier(seed_mm=seed * res, clearance_m=res / 1000.0, cap_steps=64)
    assert QM.same(got["table"], table) and QM.same(got["cost"], best)
    assert list(got["reachable"]) == [c for c in range(len(table)) if c not in pocket]
    for c in got["reachable"]:
        members = np.flatnonzero((labels == c) & (at == best[c]))
        assert tuple(got["goal"][c]) == tuple(int(rec[n][members[0]]) for n in "xyz")  # the cheapest member, the first among equals
    hw, rw = RM.paths(cost, lo, got["goal"][got["reachable"]], 64)
    assert QM.same(got["headers"], hw) and QM.same(got["paths"], rw) and np.all(hw["status"] == 0) and np.all(hw["written"] == hw["steps"] + 1)
    none = tm.reachable_frontier(seed_mm=(lo + (17, 4, 4)) * res, clearance_m=res / 1000.0)  # from inside the pocket: only its own cluster
    assert list(none["reachable"]) == pocket and none["headers"] is None


FM_TAU = 1000
