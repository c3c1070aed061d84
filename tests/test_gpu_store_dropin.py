"""The C++ drop-in of the device global map (tests/cpp/store_dropin.cpp): MappingNode::shift_map_device along a walk read from a
file prints the digests of the window and of every chunk that the Python route gives, and so does its write_back."""
import subprocess

import numpy as np
import pytest

from dropin_build import build_dropin
import window_model as M
from window_routes import MW, RES, TAU, _default, download
import window_routes as G

pytestmark = pytest.mark.gpu


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
    exe = build_dropin("store_dropin", tmp_path)
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
