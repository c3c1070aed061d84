"""The C++ drop-in of the packed snapshots (tests/cpp/store_pack_dropin.cpp): warpsense::DeviceGlobalMap::pack, clone and unpack give
the statistics and the bytes of the C ABI results the Python route reads, on the store of the brick cases of pack_model.py."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import fuse_scenes as S
import pack_model as PM
import query_model as QM
import two_store_scenes as T

pytestmark = pytest.mark.gpu


def dump(chunks, path):
    with open(path, "wb") as f:
        np.array([len(chunks)], dtype=np.int32).tofile(f)
        for key in sorted(chunks):
            np.asarray(key, dtype=np.int32).tofile(f)
            np.asarray(chunks[key], dtype=np.uint32).tofile(f)


def digest(a):
    return f"{QM.fnv1a(np.ascontiguousarray(a).tobytes()):016x}"


def test_cpp_pack_clone_unpack_equal_the_python_route(tmp_path):
    exe = build_dropin("store_pack_dropin", tmp_path)
    chunks = PM.case_store()
    own = {(7, 7, 7): T.observed(91), (0, 0, 1): T.observed(92)}
    dump(chunks, tmp_path / "src.bin")
    dump(own, tmp_path / "own.bin")
    out = subprocess.run([str(exe), str(tmp_path / "src.bin"), str(tmp_path / "own.bin"), "600"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    src, dst = S.make_store(chunks, fill=(600, 0)), S.make_store(own, fill=(-7, 5), segment_chunks=1)
    some = sorted(chunks)[::2][::-1]
    want = []
    for name, p in (("all", src.pack()), ("part", src.pack(keys=some))):
        want.append([name, str(p.n_chunks), str(p.payload_words), *(str(v) for v in p.stats), "%.9g" % p.ratio])
        want.append([name + "_digests", digest(p.headers), digest(p.payload)])
    model = PM.pack(chunks, PM.FILL, some)
    assert src.pack(keys=some).payload.tobytes() == model[1].tobytes()  # (the Python route is the model's: test_gpu_store_pack.py)
    clone = src.clone()
    want += [["clone", *(str(v) for v in k), digest(clone.chunk(k))] for k in clone.keys()]
    dst.unpack(src.pack(keys=some))
    want += [["unpacked", *(str(v) for v in k), digest(dst.chunk(k))] for k in dst.keys()]
    want.append(["expanded", digest(chunks[sorted(some)[0]])])
    assert lines == want
    assert sorted(dst.keys()) == sorted(set(some) | set(own)) and dst.chunk((7, 7, 7)).tobytes() == own[(7, 7, 7)].tobytes()
