"""The host-only route of the sliding-window tests (LocalMap against tests/window_model.py) and the chunk keys a box must touch."""
import numpy as np

import window_model as M


TAU = 1000


class HostRoute:
    """LocalMap.shift on a host map with an in-memory GlobalMap"""

    def __init__(self, size):
        import warpsense_amd as W
        self.W = W
        self.lm = W.LocalMap(*size, TAU, 0)
        assert tuple(self.lm.size) == tuple(size), (tuple(self.lm.size), tuple(size))

    def insert(self, lo, hi, words):
        lm = self.lm
        ax = M.ring_axes(lm.size, lm.pos, lm.offset, lo, hi)
        lm.data.reshape(tuple(int(s) for s in lm.size))[np.ix_(*ax)] = words.reshape(tuple(int(v) for v in hi - lo + 1))

    def shift(self, world, new_pos):
        self.lm.shift(new_pos)

    def check(self, w):
        lm = self.lm
        assert np.array_equal(lm.pos, w.pos) and np.array_equal(lm.offset, w.offset()), (lm.pos, w.pos, lm.offset, w.offset())
        assert np.array_equal(lm.data, w.ring()), (lm.data, w.ring())
        w.check_chunks(lm.map_.chunks)


def expected_keys(lo, hi):
    c0, c1 = np.floor_divide(np.asarray(lo, dtype=np.int64), 64), np.floor_divide(np.asarray(hi, dtype=np.int64), 64)
    return np.array([(x, y, z) for x in range(c0[0], c1[0] + 1) for y in range(c0[1], c1[1] + 1) for z in range(c0[2], c1[2] + 1)], dtype=np.int32)
