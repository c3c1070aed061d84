"""The C++ drop-in of the change detection (tests/cpp/store_changes_dropin.cpp): warpsense::DeviceGlobalMap::changes gives the
statistics and the bytes of records, labels and cluster table of the Python call, for the scene under the identity pose and for the
random maps under a general pose of test_gpu_store_changes.py."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import changes_scenes as T
import fuse_scenes as S
import query_model as QM

pytestmark = pytest.mark.gpu


def dump(chunks, path):
    with open(path, "wb") as f:
        np.array([len(chunks)], dtype=np.int32).tofile(f)
        for key in sorted(chunks):
            np.asarray(key, dtype=np.int32).tofile(f)
            np.asarray(chunks[key], dtype=np.uint32).tofile(f)


def cases():
    s = T.scene()
    yield "scene", s["cur"], s["ref"], np.eye(4), (0, 0, 0), 1
    cur, ref = T.pose_maps()
    yield "general", cur, ref, S.rot(4, -2, 3, (13, -7.4, 4.2)), (32 * S.RES, 64 * S.RES, 32 * S.RES), 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_dropin("store_changes_dropin", tmp_path_factory.mktemp("store_changes_dropin"))


def digest(a):
    return f"{QM.fnv1a(np.ascontiguousarray(a).tobytes()):016x}"


@pytest.mark.parametrize("case", list(cases()), ids=lambda c: c[0])
def test_cpp_changes_equal_the_python_route(exe, tmp_path, case):
    _, cur_chunks, ref_chunks, pose, pivot, mw = case
    dump(cur_chunks, tmp_path / "cur.bin")
    dump(ref_chunks, tmp_path / "ref.bin")
    np.concatenate([np.asarray(pose, dtype=np.float64).reshape(-1), np.asarray(pivot, dtype=np.float64)]).tofile(tmp_path / "pose.bin")
    out = subprocess.run([str(exe), str(tmp_path / "cur.bin"), str(tmp_path / "ref.bin"), str(tmp_path / "pose.bin"), str(S.RES), str(T.BAND), str(T.FREE), str(mw),
                          str(S.TAU)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    cur, ref = S.make_store(cur_chunks), S.make_store(ref_chunks)
    both = cur.changes(ref, pose, pivot, resolution=S.RES, band=T.BAND, free_value=T.FREE, min_weight=mw, clusters=True)
    part = cur.changes(ref, pose, pivot, resolution=S.RES, band=T.BAND, free_value=T.FREE, min_weight=mw, kinds="appeared")
    assert len(both.records) > 100 and len(both.clusters) > 1 and 0 < len(part.records) < len(both.records)
    want = []
    for name, r in (("both", both), ("appeared", part)):
        labels = r.labels if r.labels is not None else np.zeros(0, dtype=np.uint32)
        table = r.clusters if r.clusters is not None else np.zeros(0, dtype=np.uint8)
        want.append([name, *(str(v) for v in r.stats.as_tuple())])
        want.append([name + "_sizes", str(len(r.records)), str(len(labels)), str(len(table)), "%.9g" % r.stats.changed_volume_m3(S.RES)])
        want.append([name + "_digests", digest(r.records), digest(labels), digest(table)])
    assert lines == want
