"""The C++ drop-in of the coarser levels (tests/cpp/store_coarsen_dropin.cpp): warpsense::parents_of, DeviceGlobalMap::coarsen and
MapPyramid give the parents, the statistics and the chunk bytes of the Python MapPyramid on the sphere-and-floor scene, after a
rebuild and after a refresh over one replaced chunk."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import coarsen_model as CM
import fuse_scenes as S
import query_model as QM

pytestmark = pytest.mark.gpu

LEVELS, MIN_OBSERVED = 2, 6


def dump(chunks, path):
    with open(path, "wb") as f:
        np.array([len(chunks)], dtype=np.int32).tofile(f)
        for key in sorted(chunks):
            np.asarray(key, dtype=np.int32).tofile(f)
            np.asarray(chunks[key], dtype=np.uint32).tofile(f)


def report(name, p, stats):
    lines = []
    for l in range(1, p.levels + 1):
        lines.append([name, "level", str(l), "resolution", str(p.resolution(l)), "stats", *(str(v) for v in stats[l - 1].as_tuple())])
        got = S.read(p.store(l))
        lines += [["chunk", *(str(c) for c in key), f"{QM.fnv1a(got[key].tobytes()):016x}"] for key in sorted(got)]
    return lines


def test_cpp_pyramid_equals_the_python_route(tmp_path):
    import warpsense_amd as W
    exe = build_dropin("store_coarsen_dropin", tmp_path)
    base = dict(S.sphere_and_floor())
    base[(-3, 2, -2)] = S.draw(81, True)
    changed = {(-1, 0, -1): S.draw(82, True)}
    dump(base, tmp_path / "base.bin")
    dump(changed, tmp_path / "changed.bin")
    out = subprocess.run([str(exe), str(tmp_path / "base.bin"), str(tmp_path / "changed.bin"), str(LEVELS), str(MIN_OBSERVED), str(S.RES), str(S.TAU)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    p = W.MapPyramid(S.make_store(base), LEVELS, S.RES, MIN_OBSERVED, segment_chunks=2)
    want = [["parents", *(str(int(v)) for v in W.parents_of(sorted(base)).reshape(-1))]]
    want += report("rebuild", p, p.rebuild())
    p.base.put_chunk((-1, 0, -1), changed[(-1, 0, -1)])
    want += report("refresh", p, p.refresh((-64, 0, -64), (-1, 63, -1)))
    assert lines == want
    after = {**base, **changed}
    for l, model in enumerate(CM.pyramid(after, LEVELS, MIN_OBSERVED, S.FILL)):
        assert CM.same(S.read(p.store(l)), model), l
    p.close()
