"""The C++ drop-in of the fuse (tests/cpp/store_fuse_dropin.cpp): warpsense::fuse_pose and DeviceGlobalMap::fuse give the pull
transform, the statistics and the chunk bytes of the Python calls for the identity case and the general pose of
test_gpu_store_fuse.py."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import fuse_model as F
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
    dst, src = S.identity_case()
    yield "identity", dst, src, np.eye(4), (0, 0, 0)
    src, dst = S.sphere_and_floor(), S.sphere_and_floor(shift=(0.4, -0.3, 0.2), weight=35)
    del dst[(0, 0, 0)]
    yield "general", dst, src, S.rot(17, 3, 0, (13, -7, 4)), (200.4, -100.6, 50.0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_dropin("store_fuse_dropin", tmp_path_factory.mktemp("store_fuse_dropin"))


@pytest.mark.parametrize("case", list(cases()), ids=lambda c: c[0])
def test_cpp_fuse_equals_the_python_route(exe, tmp_path, case):
    import warpsense_amd as W
    _, dst_chunks, src_chunks, T, pivot = case
    dump(dst_chunks, tmp_path / "dst.bin")
    dump(src_chunks, tmp_path / "src.bin")
    np.concatenate([np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(pivot, dtype=np.float64)]).tofile(tmp_path / "pose.bin")
    out = subprocess.run([str(exe), str(tmp_path / "dst.bin"), str(tmp_path / "src.bin"), str(tmp_path / "pose.bin"), str(S.RES), str(S.MW), str(S.TAU)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    pose = W.fuse_pose(T, pivot)
    assert lines[0] == ["pose", *(str(int(v)) for v in pose)]
    dst, src = S.make_store(dst_chunks), S.make_store(src_chunks)
    count = dst.fuse(src, T, S.MW, count_only=True, pivot_src_mm=pivot, resolution=S.RES)
    st = dst.fuse(src, T, S.MW, pivot_src_mm=pivot, resolution=S.RES)
    assert lines[1] == ["count", *(str(v) for v in count.as_tuple())] and lines[2] == ["fuse", *(str(v) for v in st.as_tuple())]
    assert count.as_tuple() == st.as_tuple() and st.averaged > 10000
    got = S.read(dst)
    assert lines[3:] == [["chunk", *(str(c) for c in key), f"{QM.fnv1a(got[key].tobytes()):016x}"] for key in sorted(got)] and len(got) > len(dst_chunks)
    assert F.same((got, st.as_tuple()), F.fuse(dst_chunks, src_chunks, pose, S.RES, S.MW, S.FILL))
