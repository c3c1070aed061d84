"""The C++ drop-in of the view gain (tests/cpp/view_gain_dropin.cpp): MappingNode::view_gain / global_view_gain,
DeviceGlobalMap::view_gain and warpsense::local_map_view_gain / global_map_view_gain along the walk of
test_gpu_store_mesh.test_after_real_use print the counts and the digests of the bytes the Python route gives over the C ABI."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import query_model as QM
import store_scenes as SM
from window_routes import _params

pytestmark = pytest.mark.gpu
EDGE = 65
RANGE = 2500


def line(result, best):
    """what view_gain_dropin.cpp prints for records or (records, rays)"""
    rec, rays = result if isinstance(result, tuple) else (result, None)
    digest = lambda a: "0" * 16 if a is None or a.size == 0 else f"{QM.fnv1a(a.tobytes()):016x}"
    return [str(len(rec)), str(0 if rays is None else rays.size), str(best), digest(rec), digest(rays)]


def test_cpp_wrappers_give_the_bytes_of_the_c_abi(tmp_path):
    import warpsense_amd as W
    scans = [SM.walk_scan(k) for k in range(len(SM.WALK))]
    store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    try:
        tm = W.TSDFMapping(_params((EDGE,) * 3), W.LocalMap(EDGE, EDGE, EDGE, SM.TAU, 0), device_global_map=store)
        for k, pos in enumerate(SM.WALK):
            if k:
                tm.shift_map_device(pos)
            tm.update_tsdf(scans[k], pos_rm=pos, up_rm=(0, 0, 32768))
        pos = np.asarray(SM.WALK[-1], dtype=np.int64)
        g = np.random.default_rng(41)
        views = ((pos + g.integers(-30, 31, (9, 3)) * (1, 1, 0)) * SM.RES + 25).astype(np.int32)  # around the last sensor position, in its plane
        views[0] = (np.asarray(SM.WALK[0]) * SM.RES + (200, 25, 25)).astype(np.int32)                # and one where the window has left
        dirs = W.view_fan(8, 65, 40.0)
        exe = build_dropin("view_gain_dropin", tmp_path)
        np.concatenate(scans).tofile(tmp_path / "scans.bin")
        views.tofile(tmp_path / "views.bin")
        dirs.tofile(tmp_path / "dirs.bin")
        out = subprocess.run([str(exe), str(tmp_path / "scans.bin"), str(len(scans[0])), str(EDGE), str(SM.RES), str(SM.TAU), str(SM.MW), "2",
                              str(tmp_path / "views.bin"), str(len(views)), str(tmp_path / "dirs.bin"), str(len(dirs)), str(RANGE),
                              *(str(c) for p in SM.WALK for c in p)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout, out.stderr)
        lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
        avg = tm.tsdf().avg_map()
        window = tm.view_gain(positions_m=views / 1000.0, fan=dirs, max_range_m=RANGE / 1000.0)
        assert window["unknown"].sum() > 1000 and window["free"].sum() > 1000 and window["blocked"].sum() > 10
        assert lines["window"] == line(window, tm.last_view_gain["best_unknown_k2"])
        at_tau = avg.view_gain(views, dirs, RANGE, min_value=SM.TAU, rays=True)
        assert at_tau[0]["blocked"].sum() >= window["blocked"].sum() and lines["window_rays"] == line(at_tau, avg.last_view_gain["best_unknown_k2"])
        p = SM.WALK[-1]
        box = avg.view_gain(views, dirs, RANGE, lo=(p[0] - 10, p[1] - 20, p[2] - 5), hi=(p[0] + 25, p[1] + 12, p[2] + 9), any_weight=True, rays=True)
        assert lines["window_box"] == line(box, avg.last_view_gain["best_unknown_k2"])
        whole = tm.global_view_gain(positions_m=views / 1000.0, fan=dirs, max_range_m=RANGE / 1000.0, rays=True)
        assert whole[0]["free"][0] > window["free"][0]  # the first view stands where the window has left: only the store sees it
        assert lines["global"] == line(whole, tm.last_view_gain["best_unknown_k2"])
        assert lines["chunks"] == [str(store.count())] and store.count() >= 10
        assert lines["store_tau"] == line(store.view_gain(SM.RES, views, dirs, RANGE, min_value=SM.TAU), store.last_view_gain["best_unknown_k2"])
        cut = store.view_gain(SM.RES, views, dirs, RANGE, lo=(-20, -40, -30), hi=(70, 10, 30), any_weight=True, rays=True)
        assert lines["box"] == line(cut, store.last_view_gain["best_unknown_k2"])
        assert lines["empty"] == ["0", "0", "0", "0" * 16, "0" * 16]
    finally:
        store.close()
