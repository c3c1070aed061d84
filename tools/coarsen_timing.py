#!/usr/bin/env python3
"""Timing of ws_store_coarsen on the benchmark map; writes profiles/coarsen_timing.json.

The workload of tools/fuse_timing.py: the 513^3 map of bench.py at 50 mm after two scans goes into a store.  Two cases: level 1
alone (DeviceGlobalMap.coarsen over every parent), and the rebuild of a three-level MapPyramid.  Per case 3 warm-up calls, then 20
timed ones: the medians with minimum and maximum of the plan upload and of the pass (HIP events, ws_debug_store_coarsen_timing; summed
over the levels) and of the call end to end (host clock around the synchronising calls).  Next to them two yardsticks that are not
the code under test: the time of ws_store_get_chunk over all chunks of SRC (the floor of any host route), and the traffic floor, the
bytes of SRC's chunks read once plus DST's chunks written once over the bandwidth of a device-to-device copy of SRC's size measured in
the same run (a copy of N bytes moves 2 N)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import warpsense_amd as W  # noqa: E402
from warpsense_amd import synthetic as S  # noqa: E402

CHUNK_BYTES = 4 * 64 ** 3


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def copy_bandwidth(n_bytes, warmup, calls):
    """bytes moved per second (read + write) by a device-to-device copy of n_bytes, the median of `calls`"""
    import torch
    a, b = torch.empty(n_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    a.fill_(1)
    ms = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return 2.0 * n_bytes / (float(np.median(ms)) * 1e-3), spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=513)
    ap.add_argument("--resolution", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarsen_timing.json"))
    a = ap.parse_args()
    res, tau = a.resolution, 1000
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=10, size=(a.map * res / 1000.0,) * 3))
    store = W.DeviceGlobalMap(tau, 0)
    tm = W.TSDFMapping(params, W.LocalMap(a.map, a.map, a.map, tau, 0, host_voxels=False), device_global_map=store)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (400.0, -300.0, 100.0)]):
        tm.update_tsdf(S.os1_128_scan(sensor_mm=sensor, seed=12345 + k), pos_rm=tuple(int(np.floor(c / res)) for c in sensor), up_rm=(0, 0, 32768))
    tm.global_surface_cloud(device=True)  # the window goes into the store
    keys = store.keys()
    t0 = time.perf_counter()
    for k in keys:
        store.chunk(k)
    t_get = (time.perf_counter() - t0) * 1e3
    bandwidth, copy_ms = copy_bandwidth(len(keys) * CHUNK_BYTES, a.warmup, a.calls)
    out = dict(map=a.map, resolution=res, src_chunks=len(keys), get_chunk_src_ms=t_get, copy_ms=copy_ms, copy_bandwidth_GBps=bandwidth / 1e9, cases={})
    for name, levels in (("level_1", 1), ("three_levels", 3)):
        p = W.MapPyramid(store, levels, res)
        for l in range(1, levels + 1):
            p.store(l).coarsen_timing(1)
        rows = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            stats = p.rebuild()
            wall = (time.perf_counter() - t0) * 1e3
            ms = np.sum([p.store(l).coarsen_timing() for l in range(1, levels + 1)], axis=0)
            if i >= a.warmup:
                rows.append((ms[0], ms[1], wall))
        rows = np.asarray(rows)
        counts = [len(keys)] + [s.chunks for s in stats]
        traffic = sum(counts[l - 1] + counts[l] for l in range(1, levels + 1)) * CHUNK_BYTES
        floor_ms = traffic / bandwidth * 1e3
        kernel = float(np.median(rows[:, 1]))
        out["cases"][name] = dict(chunks_per_level=counts, stats=[s.as_tuple() for s in stats], plan_ms=spread(rows[:, 0]), kernel_ms=spread(rows[:, 1]),
                                  end_to_end_ms=spread(rows[:, 2]), traffic_bytes=traffic, traffic_floor_ms=floor_ms, kernel_over_traffic_floor=kernel / floor_ms,
                                  host_floor_over_end_to_end=t_get / float(np.median(rows[:, 2])))
        p.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
