"""The C++ drop-in of the point sample (include/warpsense_hip/visualization.hpp, app.hpp) against the Python route: the wrappers for the
window and for the store give the same bytes, and AppParams::reject_dynamic the same rejected counts and poses as App(reject_dynamic=True).
Same C ABI underneath, so everything must agree exactly.  tests/cpp/sample_dropin.cpp prints counts and FNV-1a digests."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import query_model as QM
import scan_clouds as T
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = build_dropin("sample_dropin", tmp_path_factory.mktemp("sample_dropin"))
    return str(out)


def line_of(result):
    """what sample_dropin.cpp prints for a (records, counts, gradient | None, selection | None)"""
    rec, counts, grad, sel = result
    h = lambda a: f"{QM.fnv1a(b'' if a is None else a.tobytes()):016x}"
    return [str(len(rec))] + [str(int(c)) for c in counts] + [h(rec), h(grad), str(0 if sel is None else len(sel)), h(sel)]


def test_wrappers_give_the_bytes_of_the_python_route(exe, tmp_path):
    import warpsense_amd as W
    tau, res, mw, edge = 1000, 50, 640, 65
    scan = T.room_scan(0, (0.0, 0.0, 0.0))
    rng = np.random.default_rng(8)
    cluster = (np.asarray(T.CLUSTER_AT) + rng.integers(-100, 101, (200, 3))).astype(np.int32)
    half = (edge // 2 + 3) * res
    points = np.concatenate([scan[:3000], cluster, rng.integers(-half, half, (1500, 3)).astype(np.int32), np.array([[2 ** 30, 0, 0]], dtype=np.int32)]).astype(np.int32)
    scan.tofile(tmp_path / "scan.bin")
    points.tofile(tmp_path / "points.bin")
    out = subprocess.run([exe, "sample", str(tmp_path / "scan.bin"), str(len(scan)), str(edge), str(res), str(tau), str(mw), str(tmp_path / "points.bin"),
                          str(len(points))], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    lm = W.LocalMap(edge, edge, edge, tau, 0)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    t.update_tsdf(scan, (0, 0, 0), (0, 0, 32768))
    a = t.avg_map().sample(points, band_mm=tau // 2, gradient=True, select=("free", "unknown"))
    assert all(int(c) >= 16 for c in a[1][:3]) and np.any(a[2] != 0) and len(a[3]) > 200  # (no INSIDE: the walls are seen from inside the room)
    assert lines["window"] == line_of(a)
    b = t.avg_map().sample(points, any_weight=True, select=("surface",))
    assert lines["window_any"] == line_of(b) and lines["window_any"] != lines["window"]
    store = W.DeviceGlobalMap(tau, 0)
    lo, hi = QM.window(lm.size, lm.pos)
    store.save_box(t, lo, hi)
    c = store.sample(res, points, tau // 2, gradient=True, select=("free", "unknown"))
    assert lines["store"] == line_of(c)
    d = store.sample(res, points, tau, lo=lo, hi=hi, any_weight=True, select=("surface",))
    assert lines["store_box"] == line_of(d) and int(d[1][2]) >= 16
    store.close(), t.close()


def test_reject_dynamic_gives_the_counts_and_poses_of_the_python_app(exe, tmp_path):
    import warpsense_amd as W
    tau, res, mw, edge, shift_m = 1000, 50, 640, 128, 0.6
    clouds = T.app_stream(4)
    n = max(len(c) for c in clouds)
    clouds = [np.concatenate([c, np.repeat(c[-1:], n - len(c), axis=0)]) for c in clouds]  # one size: the first scan padded with a point it has
    np.stack(clouds).tofile(tmp_path / "clouds.bin")
    out = subprocess.run([exe, "app", str(tmp_path / "clouds.bin"), str(len(clouds)), str(n), str(edge), str(res), str(tau), str(mw), str(shift_m),
                          str(tmp_path / "poses.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().splitlines()
    size = (edge, edge, edge // 2)
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(s * res / 1000.0 for s in size), shift=shift_m),
                      W.RegistrationParams(200, 0.1, 0.03))
    app = W.App(params, None, reject_dynamic=True)
    for c in clouds:
        app.cloud_callback(c)
    for k, t in enumerate(app.timings):
        f = lines[k].split()
        assert (int(f[1]), int(f[3]), int(f[5]), int(f[7])) == (k, t["points"], t["rejected"], t["iterations"]), (lines[k], t)
    assert int(lines[len(clouds) - 1].split()[9]) == app.n_updates >= 2
    rejected = [t["rejected"] for t in app.timings]
    assert rejected[0] == 0 and all(r > 0 for r in rejected[1:])
    poses = np.fromfile(tmp_path / "poses.bin", dtype=np.float32).reshape(len(clouds), 4, 4).transpose(0, 2, 1)
    assert np.array_equal(poses, np.stack(app.poses))
    probe = np.array([[25, 25, 25], [2 ** 30, 0, 0]], dtype=np.int32)
    assert lines[len(clouds)].split()[1:] == line_of(app.gpu_.sample(probe, gradient=True, select=W.SAMPLE_CLASSES))
