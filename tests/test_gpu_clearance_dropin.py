"""The C++ drop-in of the clearance (tests/cpp/clearance_dropin.cpp): MappingNode::score_trajectories / global_score_trajectories,
DeviceGlobalMap::clearance and warpsense::local_map_clearance / global_map_clearance along the walk of
test_gpu_store_mesh.test_after_real_use print the counts and the digests of the bytes the Python route gives over the C ABI; and
TSDFMapping.score_trajectories / global_score_trajectories are held to an explicit distance call followed by the clearance of the
window's wrapper and of the store."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import query_model as QM
import store_scenes as SM
from window_routes import _params

pytestmark = pytest.mark.gpu
EDGE = 65
SOFT, RANGE = 100, 7


def line(c):
    """what clearance_dropin.cpp prints for a ClearanceResult"""
    digest = lambda a: "0" * 16 if a is None or a.size == 0 else f"{QM.fnv1a(a.tobytes()):016x}"
    return [str(len(c.records)), str(0 if c.poses is None else c.poses.size), str(c.best), digest(c.records), digest(c.poses)]


def same(a, b):
    return a.best == b.best and a.records.tobytes() == b.records.tobytes() and (a.poses is None) == (b.poses is None) and \
        (a.poses is None or a.poses.tobytes() == b.poses.tobytes())


def test_cpp_wrappers_and_mapping_methods_give_the_bytes_of_the_c_abi(tmp_path):
    import warpsense_amd as W
    scans = [SM.walk_scan(k) for k in range(len(SM.WALK))]
    store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    try:
        tm = W.TSDFMapping(_params((EDGE,) * 3), W.LocalMap(EDGE, EDGE, EDGE, SM.TAU, 0), device_global_map=store)
        for k, pos in enumerate(SM.WALK):
            if k:
                tm.shift_map_device(pos)
            tm.update_tsdf(scans[k], pos_rm=pos, up_rm=(0, 0, 32768))
        at = np.asarray(SM.WALK[-1], dtype=np.float64) * SM.RES / 1000.0 + 0.025
        poses = W.arc_rollouts((at[0], at[1], at[2], np.pi), [0.4, 0.8, 1.6], np.linspace(-0.9, 0.9, 7), steps=9, dt=0.5)  # back along the walk
        body = W.body_spheres([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [-0.25, 0.0, 0.1]], [0.15, 0.1, 0.12])
        T, P = poses.shape[:2]
        exe = build_dropin("clearance_dropin", tmp_path)
        np.concatenate(scans).tofile(tmp_path / "scans.bin")
        poses.tofile(tmp_path / "poses.bin")
        body.tofile(tmp_path / "body.bin")
        out = subprocess.run([str(exe), str(tmp_path / "scans.bin"), str(len(scans[0])), str(EDGE), str(SM.RES), str(SM.TAU), str(SM.MW), "2",
                              str(tmp_path / "poses.bin"), str(T), str(P), str(tmp_path / "body.bin"), str(len(body)), str(SOFT), str(RANGE),
                              *(str(c) for p in SM.WALK for c in p)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout, out.stderr)
        lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
        avg = tm.tsdf().avg_map()
        soft_m = SOFT / 1000.0
        # the window, columns: the method is a distance call of ceil((largest radius + soft) / res) + 1 voxels, then the wrapper's clearance
        window = tm.score_trajectories(poses, body, soft_m)
        assert tm.last_clearance is window and window.poses is None
        assert 0 < np.count_nonzero(window.records["hits"]) < T and np.any(window.records["outside"] > 0)
        vox = -(-(150 + SOFT) // SM.RES) + 1
        avg.distance(max_dist_vox=vox, columns=True, device=True)
        assert same(window, avg.clearance(poses, body, SOFT))
        assert lines["window"] == line(window)
        volume = tm.score_trajectories(poses, body, soft_m, max_dist_m=RANGE * SM.RES / 1000.0, columns=False, per_pose=True, outside_ok=True)
        assert volume.best >= 0  # (outside samples do not disqualify here)
        avg.distance(max_dist_vox=RANGE, device=True)
        assert same(volume, avg.clearance(poses, body, SOFT, per_pose=True, outside_ok=True)) and lines["window_volume"] == line(volume)
        again = tm.score_trajectories(poses, body, 0.0, refresh=False)  # on the distance result that is there
        assert same(again, avg.clearance(poses, body, 0)) and lines["window_again"] == line(again)
        assert np.all(again.records["cost"] <= volume.records["cost"]) and np.array_equal(again.records["min_margin"], volume.records["min_margin"])
        for bad in (dict(max_dist_m=0.0), dict(max_dist_m=256 * SM.RES / 1000.0)):
            with pytest.raises(W.WsError):
                tm.score_trajectories(poses, body, soft_m, **bad)
        # everything the run has seen: the window goes into the store first
        whole = tm.global_score_trajectories(poses, body, soft_m, per_pose=True)
        assert tm.last_clearance is whole and lines["global"] == line(whole)
        assert lines["chunks"] == [str(store.count())] and store.count() >= 10
        store.distance(max_dist_vox=vox, columns=True, device=True)
        assert same(whole, store.clearance(SM.RES, poses, body, SOFT, per_pose=True))
        assert np.count_nonzero(whole.records["outside"]) < np.count_nonzero(window.records["outside"])  # the store reaches where the window has left
        store.distance(lo=(-20, -40, -30), hi=(70, 10, 30), max_dist_vox=RANGE, unknown_occupied=True, device=True)
        cut = store.clearance(SM.RES, poses, body, SOFT, per_pose=True)
        assert lines["store_box"] == line(cut) and lines["store_ok"] == line(store.clearance(SM.RES, poses, body, SOFT, outside_ok=True))
        assert lines["empty"] == ["0", "0", "-1", "0" * 16, "0" * 16]
    finally:
        store.close()
