"""The C++ drop-in of the ray cast of the device global map (tests/cpp/store_raycast_dropin.cpp): MappingNode::global_raycast along
the walk of test_gpu_store_mesh.test_after_real_use, from the first pose after the window has moved on, prints the digests of the
bytes the Python route gives."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import query_model as QM
import store_scenes as SM
from window_routes import _params

pytestmark = pytest.mark.gpu


def test_cpp_global_raycast_equals_the_python_route(tmp_path):
    import warpsense_amd as W
    from warpsense_amd import synthetic as S
    exe = build_dropin("store_raycast_dropin", tmp_path)
    scans = [SM.walk_scan(k) for k in range(len(SM.WALK))]
    np.concatenate(scans).tofile(tmp_path / "scans.bin")
    pose = np.eye(4)
    pose[:3, 3] = np.asarray(SM.WALK[0], dtype=np.float64) * SM.RES / 1000.0
    origin, dirs = W.TSDFMapping.raycast_rays(pose, S.os1_128_dirs().reshape(-1, 3)[::16])
    assert len(dirs) == 8192 and tuple(origin) == tuple(c * SM.RES for c in SM.WALK[0])
    dirs.astype(np.int32).tofile(tmp_path / "dirs.bin")
    edge, rng = 65, 9000
    out = subprocess.run([str(exe), str(tmp_path / "scans.bin"), str(len(scans[0])), str(tmp_path / "dirs.bin"), str(len(dirs)), str(rng), str(edge),
                          str(SM.RES), str(SM.TAU), str(SM.MW), "2", *(str(c) for pos in SM.WALK for c in pos)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params((edge,) * 3), W.LocalMap(edge, edge, edge, SM.TAU, 0), device_global_map=store)
    for k, pos in enumerate(SM.WALK):
        if k:
            tm.shift_map_device(pos)
        tm.update_tsdf(scans[k], pos_rm=pos, up_rm=(0, 0, 32768))

    def line(cast):
        rec, grad = cast
        hits = int(np.count_nonzero(rec["range_mm"] >= 0))
        return [str(len(rec)), str(hits), f"{QM.fnv1a(rec.tobytes()):016x}", "-" if grad is None else f"{QM.fnv1a(grad.tobytes()):016x}"]

    got = tm.global_raycast(pose, S.os1_128_dirs().reshape(-1, 3)[::16], max_range_mm=rng, gradient=True)
    assert np.count_nonzero(got[0]["range_mm"] >= 0) > 1000 and np.any(got[1] != 0)
    assert lines["global"] == line(got)
    assert lines["chunks"] == [str(store.count())] and store.count() >= 10
    assert lines["any_weight"] == line(tm.global_raycast(pose, S.os1_128_dirs().reshape(-1, 3)[::16], max_range_mm=rng, any_weight=True))
    box = store.raycast(SM.RES, origin, dirs, rng, lo=(-20, -40, -30), hi=(70, 10, 30), gradient=True)
    assert 10 < np.count_nonzero(box[0]["range_mm"] >= 0) < np.count_nonzero(got[0]["range_mm"] >= 0) and lines["box"] == line(box)
    store.close()
