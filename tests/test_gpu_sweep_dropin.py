"""The C++ drop-in of the motion-compensated pre-processing (tests/cpp/sweep_dropin.cpp): warpsense::sweep_poses and
ScanPreprocessor::preprocess_sweep through compat.hpp give the bytes of the Python calls."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
from scan_clouds import rigid
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu


def test_cpp_sweep_equals_the_python_route(tmp_path):
    import warpsense_amd as W
    exe = build_dropin("sweep_dropin", tmp_path)
    res, k, rings, azimuths = 50, 24, 16, 96
    begin, end = rigid(-150.0, 60.0, 0.0, -4.0), rigid(180.0, 140.0, 10.0, 6.0)
    motion = (np.linalg.inv(begin) @ end).astype(np.float32)
    pose_end = end.astype(np.float32)
    cloud = S.os1_128_sweep(begin, end, rings=rings, azimuths=azimuths, half_extents_mm=(2000.0, 1800.0, 900.0), seed=11, with_time=True)
    cloud.tofile(tmp_path / "cloud.bin")
    np.stack([pose_end.T, motion.T]).astype(np.float32).tofile(tmp_path / "mats.bin")  # column-major
    prefix = str(tmp_path / "out")
    out = subprocess.run([str(exe), str(tmp_path / "cloud.bin"), str(len(cloud)), "4", str(tmp_path / "mats.bin"), str(k), str(azimuths), "1", "3", str(res),
                          prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    poses = W.sweep_poses(pose_end, motion, k)
    got_poses = np.fromfile(prefix + ".poses", dtype=np.float32).reshape(k, 4, 4).transpose(0, 2, 1)
    assert np.array_equal(got_poses.view(np.uint32), poses.view(np.uint32))
    pre = W.ScanPreprocessor(len(cloud))
    by_index = pre.preprocess_sweep(cloud, poses, res, columns=azimuths, ring_major=True).to_host()
    by_time = pre.preprocess_sweep(cloud, poses, res, time_field=3).to_host()
    assert len(by_index) > 1000 and np.array_equal(by_index, W.preprocess_sweep_host(cloud, poses, res, columns=azimuths))
    assert np.fromfile(prefix + ".index", dtype=np.int32).tobytes() == by_index.tobytes()
    assert np.fromfile(prefix + ".time", dtype=np.int32).tobytes() == by_time.tobytes()
    assert ["index", str(len(by_index))] in lines and ["time", str(len(by_time))] in lines
    assert ["again", str(len(by_index))] in lines
