"""The C++ drop-in of the ground layer (tests/cpp/ground_dropin.cpp): warpsense::global_map_ground / global_map_ground_distance,
DeviceGlobalMap::ground / ground_distance and warpsense::local_map_ground / local_map_ground_distance on the stacked chunks of
test_gpu_ground.py print the digests of the bytes the Python route gives, which are held to the model here."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import ground_model as G
import ground_scenes as S
import query_model as QM
import store_scenes as SM

pytestmark = pytest.mark.gpu


def ground_line(g):
    return [str(v) for v in g.lo] + [str(g.ext[0]), str(g.ext[1])] + [str(int(c)) for c in g.counts] + [f"{QM.fnv1a(np.ascontiguousarray(g.records).tobytes()):016x}"]


def distance_line(rec, sites):
    return [str(rec.shape[0]), str(rec.shape[1]), "1", str(sites), f"{QM.fnv1a(rec.tobytes()):016x}"]


def test_cpp_ground_equals_the_python_route(tmp_path):
    exe = build_dropin("ground_dropin", tmp_path)
    chunks = S.stack_chunks()
    with open(tmp_path / "chunks.bin", "wb") as f:
        for key in sorted(chunks):
            f.write(np.asarray(key, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(chunks[key], dtype=np.uint32).tobytes())
    lo, hi = S.FULL_BOX
    out = subprocess.run([str(exe), str(tmp_path / "chunks.bin"), str(len(chunks)), str(S.TAU), "5", *(str(v) for v in lo + hi)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    assert lines["chunks"] == ["12"]
    store = S.make_store(chunks)
    size, pos, off = (32, 32, 150), (0, 0, 80), (5, 7, 11)
    wlo, whi = QM.window(size, pos)
    t, wlo, whi = S.make_window(size, pos, off, SM.assemble(chunks, wlo, whi))
    try:
        g = store.ground(lo=lo, hi=hi, clear_vox=3)
        assert G.same(g.records, S.stack_model(None, lo, hi, 3)[0]) and lines["store"] == ground_line(g)
        assert lines["store_distance"] == distance_line(store.ground_distance(300, max_dist_vox=5), store.last_sites)
        kw = dict(any_weight=True, unknown_headroom=True, top=True)
        g = store.ground(lo=lo, hi=hi, clear_vox=20, **kw)
        assert G.same(g.records, S.stack_model(None, lo, hi, 20, **kw)[0]) and lines["store_flags"] == ground_line(g)
        assert lines["store_flags_distance"] == distance_line(store.ground_distance(65535, max_dist_vox=40, unknown_occupied=True), store.last_sites)
        g = store.ground(clear_vox=64)
        assert g.records.shape == (128, 128) and lines["bounding"] == ground_line(g)
        avg = t.avg_map()
        a, b = (lo[0], lo[1], wlo[2]), (hi[0], hi[1], whi[2])
        g = avg.ground(lo=a, hi=b, clear_vox=3)
        assert G.same(g.records, S.stack_model(None, a, b, 3)[0]) and lines["window"] == ground_line(g) and int(g.counts[G.GROUND]) > 0
        assert lines["window_distance"] == distance_line(avg.ground_distance(300, max_dist_vox=5), avg.last_sites)
        assert lines["window_flags"] == ground_line(avg.ground(lo=a, hi=b, clear_vox=20, **kw))
        g = avg.ground(clear_vox=64, unknown_headroom=True)
        assert g.records.shape == (32, 32) and lines["window_whole"] == ground_line(g)
    finally:
        store.close()
        t.close()
