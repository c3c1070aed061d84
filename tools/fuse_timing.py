#!/usr/bin/env python3
"""Timing of ws_store_fuse on the benchmark map; writes profiles/fuse_timing.json.

The 513^3 map of bench.py after two scans goes into a store and is copied into a second one; the copy is fused back under (a) the
identity and (b) 5 degrees yaw + 2 degrees pitch + (13, -7, 4) mm.  Per case 3 warm-up calls, then 20 timed ones: the medians with
minimum and maximum of the plan upload, the count pass and the write pass (HIP events, ws_debug_store_fuse_timing) and of the call
end to end (host clock around the synchronising call).  Next to them the time of ws_store_get_chunk over all chunks of both stores,
the floor of any host route.  DST keeps what the earlier calls fused into it: the work per call does not depend on the entries."""
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


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def rot(yaw, pitch, t):
    a, b = np.deg2rad([yaw, pitch])
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry, t
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=513)
    ap.add_argument("--resolution", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_timing.json"))
    a = ap.parse_args()
    res, tau = a.resolution, 1000
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=10, size=(a.map * res / 1000.0,) * 3))
    store, copy = W.DeviceGlobalMap(tau, 0), W.DeviceGlobalMap(tau, 0)
    tm = W.TSDFMapping(params, W.LocalMap(a.map, a.map, a.map, tau, 0, host_voxels=False), device_global_map=store)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (400.0, -300.0, 100.0)]):
        tm.update_tsdf(S.os1_128_scan(sensor_mm=sensor, seed=12345 + k), pos_rm=tuple(int(np.floor(c / res)) for c in sensor), up_rm=(0, 0, 32768))
    tm.global_surface_cloud(device=True)  # the window goes into the store
    keys = store.keys()
    t0 = time.perf_counter()
    chunks = [store.chunk(k) for k in keys]
    t_get = time.perf_counter() - t0
    for k, c in zip(keys, chunks):
        copy.put_chunk(k, c)
    t0 = time.perf_counter()
    for k in keys:
        copy.chunk(k)
    t_get += time.perf_counter() - t0
    del chunks
    mw = params.map.max_weight
    out = dict(map=a.map, resolution=res, chunks_per_store=len(keys), get_chunk_both_stores_ms=t_get * 1e3, cases={})
    centre = (0.0, 0.0, 0.0)
    for name, T in (("identity", np.eye(4)), ("yaw5_pitch2_t13_-7_4", rot(5, 2, (13, -7, 4)))):
        store.fuse_timing(1)
        rows = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            st = store.fuse(copy, T, mw, pivot_src_mm=centre, resolution=res)
            wall = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                rows.append((*store.last_fuse_timing, wall))
        store.fuse_timing(0)
        rows = np.asarray(rows)
        out["cases"][name] = dict(stats=st.as_tuple(), plan_ms=spread(rows[:, 0]), count_ms=spread(rows[:, 1]), write_ms=spread(rows[:, 2]),
                                  end_to_end_ms=spread(rows[:, 3]), host_floor_over_end_to_end=t_get * 1e3 / float(np.median(rows[:, 3])))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
