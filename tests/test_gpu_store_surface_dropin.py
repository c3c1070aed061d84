"""The C++ drop-in of the surface cloud of the device global map (tests/cpp/store_surface_dropin.cpp): MappingNode::global_surface and
warpsense::global_map_cloud along the walk of test_gpu_store_mesh.test_after_real_use print the count and the digests of the bytes the
Python route gives."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import query_model as QM
import store_scenes as SM
from window_routes import _params

pytestmark = pytest.mark.gpu


def test_cpp_global_surface_equals_the_python_route(tmp_path):
    import warpsense_amd as W
    exe = build_dropin("store_surface_dropin", tmp_path)
    scans = [SM.walk_scan(k) for k in range(len(SM.WALK))]
    np.concatenate(scans).tofile(tmp_path / "scans.bin")
    edge = 65
    out = subprocess.run([str(exe), str(tmp_path / "scans.bin"), str(len(scans[0])), str(edge), str(SM.RES), str(SM.TAU), str(SM.MW), "2",
                          *(str(c) for pos in SM.WALK for c in pos)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params((edge,) * 3), W.LocalMap(edge, edge, edge, SM.TAU, 0), device_global_map=store)
    for k, pos in enumerate(SM.WALK):
        if k:
            tm.shift_map_device(pos)
        tm.update_tsdf(scans[k], pos_rm=pos, up_rm=(0, 0, 32768))
    rec, mk = tm.global_surface_cloud(marker=True)
    assert len(rec) > 1000
    assert lines["global"] == [str(len(rec)), f"{QM.fnv1a(rec.tobytes()):016x}", f"{QM.fnv1a(mk.tobytes()):016x}"]
    assert lines["chunks"] == [str(store.count())] and store.count() >= 10
    box = store.surface(SM.TAU, SM.RES, lo=(-20, -40, -30), hi=(70, 10, 30), band=SM.TAU // 2)
    assert 100 < len(box) < len(rec) and lines["box"] == [str(len(box)), f"{QM.fnv1a(box.tobytes()):016x}", "0" * 16]
    store.close()
