"""The C++ drop-in of the distance field of the device global map (tests/cpp/store_distance_dropin.cpp): warpsense::global_map_distance
and DeviceGlobalMap::distance on the seam store of test_gpu_store_distance.py print the digests of the bytes the Python route gives."""
import subprocess

import numpy as np
import pytest

import distance_model as D
from dropin_build import build_dropin
import query_model as QM
import store_distance_scenes as SD

pytestmark = pytest.mark.gpu


def test_cpp_global_map_distance_equals_the_python_route(tmp_path):
    exe = build_dropin("store_distance_dropin", tmp_path)
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
            return [str(v) for v in ext] + [str(store.last_sites), f"{QM.fnv1a(rec.tobytes()):016x}"]
        assert lines["chunks"] == ["7"]
        rec = store.distance(lo=(-SD.CS,) * 3, hi=(0, 0, SD.CS - 1), max_dist_vox=7)  # (a call in between: the digests are not of a stale result)
        rec = store.distance(max_dist_vox=7)
        assert D.same(rec, SD.seam_model((-SD.CS,) * 3, (SD.CS - 1,) * 3, 7)[0]) and lines["bounding"] == line(rec)
        rec = store.distance(lo=lo, hi=hi, max_dist_vox=40, unknown_occupied=True, any_weight=True)
        assert D.same(rec, SD.seam_model(lo, hi, 40, unknown_occupied=True, any_weight=True)[0]) and lines["box"] == line(rec)
        rec = store.distance(lo=lo, hi=hi, max_dist_vox=20, columns=True)
        assert rec.ndim == 2 and lines["columns"] == line(rec)
    finally:
        store.close()
