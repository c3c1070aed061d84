"""The C++ drop-in of the batched registration (tests/cpp/reg_batch_dropin.cpp): register_cloud_batch through compat.hpp equals the
single C++ call bit for bit, and both equal the Python route."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import reg_scenes as B
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


def test_cpp_batch_equals_the_single_cpp_call_and_the_python_route(tmp_path):
    import warpsense_amd as W
    exe = build_dropin("reg_batch_dropin", tmp_path)
    tau, res, mw, edge, max_it = 1000, 50, 640, 129, 60
    pts = S.os1_128_scan(rings=32, azimuths=256, half_extents_mm=(2600.0, 2300.0, 1000.0), seed=21)
    q = B.batch_cloud(pts)
    poses = B.pose_list(len(B.POSES))
    pts.tofile(tmp_path / "scan.bin")
    q.tofile(tmp_path / "cloud.bin")
    np.ascontiguousarray(poses.transpose(0, 2, 1)).tofile(tmp_path / "poses.bin")  # column-major
    out = subprocess.run([str(exe), str(tmp_path / "scan.bin"), str(tmp_path / "cloud.bin"), str(len(pts)), str(edge), str(res), str(tau), str(mw),
                          str(tmp_path / "poses.bin"), str(len(poses)), str(max_it)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    got = [l for l in lines if l[0] == "pose"]
    assert len(got) == len(poses) and ["differ", "0"] in lines and ["empty", "0"] in lines
    # the Python route on the same map
    lm = W.LocalMap(edge, edge, edge, tau, 0)
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=(edge * res / 1000.0,) * 3),
                      W.RegistrationParams(max_iterations=max_it))
    reg = W.TSDFRegistration(params, lm)
    reg.tsdf().update_tsdf(pts, (0, 0, 0), (0, 0, 32768))
    T, it, e, c = reg.register_candidates(q, poses)
    assert len(set(it.tolist())) >= 3 and c[B.FAR_AWAY] == 0
    for k, l in enumerate(got):
        assert [int(v) for v in l[1:5]] == [k, it[k], e[k], c[k]], (k, l[:5])
        bits = np.array([int(v, 16) for v in l[5:]], dtype=np.uint32).reshape(4, 4).T  # printed column-major
        assert np.array_equal(bits, T[k].view(np.uint32)), k
    assert ["best", str(W.batch_best(e, c, len(q) // 2))] in lines
