"""The C++ drop-in of the frontier (tests/cpp/frontier_dropin.cpp): MappingNode::frontier / global_frontier, DeviceGlobalMap::frontier and
warpsense::local_map_frontier / global_map_frontier along the walk of test_gpu_store_mesh.test_after_real_use print the counts and the
digests of the bytes the Python route gives; and TSDFMapping.global_frontier, whose default box is the chunks' bounding box grown by one
voxel, against the numpy model on the store's chunks."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import frontier_model as FM
import query_model as QM
import store_scenes as SM
from window_routes import _params

pytestmark = pytest.mark.gpu
EDGE = 65


def line(result):
    """what frontier_dropin.cpp prints for records or (records, labels, table)"""
    rec, labels, table = result if isinstance(result, tuple) else (result, None, None)
    digest = lambda a: "0" * 16 if a is None or len(a) == 0 else f"{QM.fnv1a(a.tobytes()):016x}"
    return [str(len(rec)), str(0 if table is None else len(table)), f"{QM.fnv1a(rec.tobytes()):016x}", digest(labels), digest(table)]


@pytest.fixture(scope="module")
def walked():
    """the Python route along the walk: a mapping with a device global map after three scans and two device shifts"""
    import warpsense_amd as W
    scans = [SM.walk_scan(k) for k in range(len(SM.WALK))]
    store = W.DeviceGlobalMap(SM.TAU, 0, segment_chunks=2)
    tm = W.TSDFMapping(_params((EDGE,) * 3), W.LocalMap(EDGE, EDGE, EDGE, SM.TAU, 0), device_global_map=store)
    for k, pos in enumerate(SM.WALK):
        if k:
            tm.shift_map_device(pos)
        tm.update_tsdf(scans[k], pos_rm=pos, up_rm=(0, 0, 32768))
    yield tm, store, scans
    store.close()


def test_cpp_wrappers_give_the_bytes_of_the_c_abi(walked, tmp_path):
    tm, store, scans = walked
    exe = build_dropin("frontier_dropin", tmp_path)
    np.concatenate(scans).tofile(tmp_path / "scans.bin")
    out = subprocess.run([str(exe), str(tmp_path / "scans.bin"), str(len(scans[0])), str(EDGE), str(SM.RES), str(SM.TAU), str(SM.MW), "2",
                          *(str(c) for pos in SM.WALK for c in pos)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    window = tm.frontier(clusters=True)
    assert len(window[0]) > 1000 and len(window[2]) >= 1 and lines["window"] == line(window)
    at_tau = tm.frontier(clusters=True, min_value=SM.TAU)
    assert 0 < len(at_tau[0]) <= len(window[0]) and lines["window_tau"] == line(at_tau)
    pos = SM.WALK[-1]
    box = tm.frontier(lo=(pos[0] - 10, pos[1] - 20, pos[2] - 5), hi=(pos[0] + 25, pos[1] + 12, pos[2] + 9), any_weight=True)
    assert len(box) > 100 and lines["window_box"] == line(box)
    whole = tm.global_frontier(clusters=True)
    assert len(whole[0]) > 1000 and lines["global"] == line(whole)
    assert lines["chunks"] == [str(store.count())] and store.count() >= 10
    assert lines["bounds"] == line(store.frontier(min_value=SM.TAU, clusters=True))
    cut = store.frontier(lo=(-20, -40, -30), hi=(70, 10, 30), clusters=True)
    assert 100 < len(cut[0]) < len(whole[0]) and lines["box"] == line(cut)


def test_global_frontier_is_the_model_on_the_bounding_box_grown_by_one(walked):
    tm, store, scans = walked
    got = tm.global_frontier(clusters=True, min_value=SM.TAU)  # (saves the window into the chunks first)
    chunks = {tuple(int(c) for c in key): store.chunk(key) for key in store.keys()}
    lo, hi = SM.bounding_box(chunks)
    present = SM.assemble({k: np.ones(SM.CW, dtype=np.uint32) for k in chunks}, lo - 1, hi + 1) != 0
    want = FM.frontier(SM.assemble(chunks, lo - 1, hi + 1), lo - 1, SM.TAU, False, present)
    assert len(want[0]) > 1000 and all(QM.same(g, w) for g, w in zip(got, want))
    inner = store.frontier(min_value=SM.TAU, clusters=True)  # the bounding box itself: its faces are no frontier
    want_inner = FM.frontier(SM.assemble(chunks, lo, hi), lo, SM.TAU, False, present[1:-1, 1:-1, 1:-1])
    assert all(QM.same(g, w) for g, w in zip(inner, want_inner)) and len(inner[0]) <= len(got[0])
    assert all(QM.same(g, w) for g, w in zip(tm.global_frontier(lo=lo, hi=hi, clusters=True, min_value=SM.TAU), want_inner))
