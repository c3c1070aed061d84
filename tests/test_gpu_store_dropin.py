"""The C++ drop-in of the device global map (tests/cpp/store_dropin.cpp): MappingNode::shift_map_device along a walk read from a
file prints the digests of the window and of every chunk that the Python route gives, and so does its write_back."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_store as G
import window_model as M
from test_gpu_map_window import MW, RES, TAU, _default, download

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(words):
    """sum of word[i] * (2 i + 1) modulo 2^64, as store_dropin.cpp computes it"""
    w = np.asarray(words, dtype=np.uint32).reshape(-1).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(np.sum(w * (np.uint64(2) * np.arange(w.size, dtype=np.uint64) + np.uint64(1)), dtype=np.uint64))


class Recorder:
    """a StoreRoute that also writes down what it is asked to do, as the int32 script of store_dropin.cpp"""

    def __init__(self, route):
        self.route, self.script = route, []

    def insert(self, lo, hi, words):
        self.script += [np.array([1], dtype=np.int32), np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32), np.asarray(words, dtype=np.uint32).view(np.int32)]
        self.route.insert(lo, hi, words)

    def shift(self, w, new_pos):
        self.script += [np.array([2], dtype=np.int32), np.asarray(new_pos, dtype=np.int32)]
        self.route.shift(w, new_pos)

    def check(self, w):
        pass  # (test_gpu_store.py holds this route to the model after every step)


def test_cpp_shift_map_device_equals_the_python_route(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "the C++ drop-in needs g++"
    exe = tmp_path / "store_dropin"
    lib = os.path.join(ROOT, "warpsense_amd")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}",
                           os.path.join(ROOT, "tests", "cpp", "store_dropin.cpp"), "-o", str(exe), f"-L{lib}", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-lwarpsense_hip", "-lpthread"])
    size, seed = M.WALKS[0]
    walk = M.make_walk(size, seed)
    rec = Recorder(G.StoreRoute(size, segment_chunks=2))
    w = M.run_walk(size, walk, seed, rec, _default(), check_every=False)
    r = rec.route
    r.check(w)
    chunks = r.finish(w)
    np.concatenate(rec.script + [np.array([0], dtype=np.int32)]).tofile(tmp_path / "walk.bin")
    out = subprocess.run([str(exe), str(tmp_path / "walk.bin"), *(str(s) for s in size), str(RES), str(TAU), str(MW), "2"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    assert ["shifts", str(len(walk))] in lines
    got = download(r.t, 0, int(np.prod(size)))
    want_window = ["window", *(str(int(v)) for v in got.pos_), *(str(int(v)) for v in got.offset_), f"{digest(got.data_):016x}"]
    assert [l for l in lines if l[0] == "window"] == [want_window]
    want_chunks = [["chunk", *(str(v) for v in key), f"{digest(chunks[key]):016x}"] for key in sorted(chunks)]
    assert len(want_chunks) > 4 and [l for l in lines if l[0] == "chunk"] == want_chunks
    # write_back through the store, both sides
    r.tm.write_back()
    host = r.lm.map_.chunks
    assert sorted(host) == sorted(chunks)
    w.store[w.sl(*w.window())] = w.world[w.sl(*w.window())]
    w.check_chunks(host)
    assert [l for l in lines if l[0] == "host"] == [["host", *(str(v) for v in key), f"{digest(host[key]):016x}"] for key in sorted(host)]
    assert ["host_chunks", str(len(host))] in lines
