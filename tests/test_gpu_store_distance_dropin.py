"""The C++ drop-in of the distance field of the device global map (tests/cpp/store_distance_dropin.cpp): warpsense::global_map_distance
and DeviceGlobalMap::distance on the seam store of test_gpu_store_distance.py print the digests of the bytes the Python route gives."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_store_distance as SD
import test_gpu_surface as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_global_map_distance_equals_the_python_route(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "the C++ drop-in needs g++"
    exe = tmp_path / "store_distance_dropin"
    lib = os.path.join(ROOT, "warpsense_amd")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}",
                           os.path.join(ROOT, "tests", "cpp", "store_distance_dropin.cpp"), "-o", str(exe), f"-L{lib}", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-lwarpsense_hip", "-lpthread"])
    chunks = SD.seam_chunks()
    with open(tmp_path / "chunks.bin", "wb") as f:
        for key in sorted(chunks):
            f.write(np.asarray(key, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(chunks[key], dtype=np.uint32).tobytes())
    lo, hi = SD.CUT_BOXES[0]
    out = subprocess.run([str(exe), str(tmp_path / "chunks.bin"), str(len(chunks)), str(SD.TAU), "2", *(str(v) for v in lo + hi)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    store = SD.make_store(chunks)
    try:
        def line(rec):
            ext = rec.shape if rec.ndim == 3 else rec.shape + (1,)
            return [str(v) for v in ext] + [str(store.last_sites), f"{G.fnv1a(rec.tobytes()):016x}"]
        assert lines["chunks"] == ["7"]
        rec = store.distance(lo=(-SD.CS,) * 3, hi=(0, 0, SD.CS - 1), max_dist_vox=7)  # (a call in between: the digests are not of a stale result)
        rec = store.distance(max_dist_vox=7)
        assert SD.D.same(rec, SD.seam_model((-SD.CS,) * 3, (SD.CS - 1,) * 3, 7)[0]) and lines["bounding"] == line(rec)
        rec = store.distance(lo=lo, hi=hi, max_dist_vox=40, unknown_occupied=True, any_weight=True)
        assert SD.D.same(rec, SD.seam_model(lo, hi, 40, unknown_occupied=True, any_weight=True)[0]) and lines["box"] == line(rec)
        rec = store.distance(lo=lo, hi=hi, max_dist_vox=20, columns=True)
        assert rec.ndim == 2 and lines["columns"] == line(rec)
    finally:
        store.close()
