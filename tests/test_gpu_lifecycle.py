"""The lifecycle of the library's objects: a map, a registration and a scan pre-processor are created, every path that allocates
or grows one of their buffers runs once, and everything is destroyed -- several times over.  What one cycle takes from the device
it must give back: free device memory (hipMemGetInfo, through torch) after a cycle must not lie below the figure after the cycle
before it.

The first cycle is left out of the comparison: it warms the runtime's own pools (code objects, the streams' command buffers).
CYCLES = 5 gives four comparisons and takes about a second.

MARGIN.  The library at the commit before the owning types (every hipFree written out by hand) ran this file unchanged: free
memory after its cycles 1 .. 5 was the same figure to the byte, so its largest cycle-to-cycle drop is 0 bytes (the run is kept in
profiles/ownership_refactor.json).  The smallest buffer a cycle allocates is the 4-byte arrival counter of ws_reg_create.
MARGIN is the sum of the two, so one buffer forgotten per cycle, whichever it is, fails -- as far as the runtime's accounting shows
it: hipMemGetInfo moves in the runtime's own granules, so a leak shows as a multiple of those, never as less than the margin."""
import numpy as np
import pytest

from lifecycle_model import CYCLES, MARGIN
from warpsense_amd import synthetic as S

pytestmark = pytest.mark.gpu

TAU, RES, SIZE = 1000, 50, (96, 96, 48)


def one_cycle(W, pts, cloud_m):
    """create, use every allocating path once, destroy"""
    eye = np.eye(4, dtype=np.float32)
    params = W.Params(W.MapParams(resolution=RES, max_distance=TAU / 1000.0, max_weight=10, size=tuple(s * RES / 1000.0 for s in SIZE)))
    tm = W.TSDFMapping(params, W.LocalMap(*SIZE, TAU, 0))
    reg = W.RegistrationCuda()
    sp = W.ScanPreprocessor(max_points=cloud_m.shape[0])
    try:
        avg, map_dev = tm.tsdf().avg_map(), tm.tsdf().device_map()
        assert sp.preprocess(cloud_m, eye, RES).shape[0] > 0     # host cloud: the input staging grows
        tm.update_tsdf(pts, pose=eye)                            # one update
        q = S.transform_points_mm(pts, S.perturbation(30, 20, 0, 1.5))
        reg.prepare_registration(q)
        _, iterations = reg.register_cloud(map_dev, eye, 20, 0.1, 0.03, RES)   # one registration
        assert iterations > 0
        poses = np.stack([S.perturbation(10.0 * k, 0, 0, 0.5 * k) for k in range(3)])
        T, it, _, c = reg.register_cloud_batch(map_dev, poses, 5, 0.1, 0.03, RES)  # one batch: the record block grows
        assert T.shape == (3, 4, 4) and np.all(it > 0) and np.all(c > 0)
        lo, hi = (-20, -10, -5), (20, 10, 5)
        box = avg.extract_box(lo, hi)                            # the box staging grows
        assert np.any(box != box[0])
        avg.insert_box(lo, hi, box)
        tm.shift_map_async((3, -2, 1))                           # one shift: device and pinned staging grow, stream and event appear
        tm.wait_shift()
        assert avg.surface(marker=True)[0].size > 0              # the four queries, each with all of its buffers
        vert, face = avg.mesh(any_weight=True)
        dirs = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], dtype=np.int32) << 10
        rec, grad = avg.raycast((0, 0, 0), dirs, 4000, any_weight=True, gradient=True)
        assert rec.shape == (4,) and grad.shape == (4, 3)
        assert avg.distance(max_dist_vox=4).shape == tuple(2 * (s // 2) + 1 for s in SIZE)
        assert vert.size > 0 and face.size > 0 and avg.last_hits > 0 and avg.last_sites > 0
        return dict(vertices=int(vert.size), faces=int(face.shape[0]), hits=int(avg.last_hits), sites=int(avg.last_sites))
    finally:
        sp.close()
        reg.close()
        tm.tsdf().close()


def test_cycles_of_create_use_destroy_give_their_memory_back():
    import torch
    import warpsense_amd as W
    pts = S.os1_128_scan(rings=32, azimuths=256, half_extents_mm=(2000.0, 1700.0, 800.0), seed=1)
    cloud_m = (pts.astype(np.float32) / np.float32(1000.0)).astype(np.float32)
    free = []
    for _ in range(CYCLES):
        counts = one_cycle(W, pts, cloud_m)
        W.Context.default().sync()
        torch.cuda.synchronize()
        free.append(int(torch.cuda.mem_get_info()[0]))
    drops = [free[k] - free[k + 1] for k in range(CYCLES - 1)]
    print(f"lifecycle: free bytes after each cycle {free}, drops after the first {drops}, margin {MARGIN}; the last cycle's queries gave {counts}")
    assert max(drops) <= MARGIN, (free, drops)
