#!/usr/bin/env python3
"""Timing of ws_store_ground on the benchmark map; writes profiles/ground_timing.json.

The store of tools/fuse_timing.py and tools/changes_timing.py: the 513^3 map of bench.py after two scans goes into a store (729
chunks).  ws_store_ground runs over the bounding box of the chunks: 3 warm-up calls, then 20 timed ones, the medians with minimum
and maximum of pass 1 (levels) and pass 2 (steps) (HIP events, ws_debug_store_ground_timing) and of the call end to end (host clock
around the synchronising call); then the bridge ws_store_ground_distance.

Two yardsticks that are not the code under test, in the same run: pass 0 of ws_store_distance(..., WS_DISTANCE_COLUMNS) on the same
store and box, which streams the same chunk bytes with the same walk (ws_debug_store_distance_timing), and a device-to-device copy of
the store's size (a copy reads and writes every byte: the chunks read once take half its time)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warpsense_amd as W  # noqa: E402
from warpsense_amd import synthetic as S  # noqa: E402
from changes_timing import copy_ms  # noqa: E402


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def timed(call, timing, slots, warmup, calls):
    """per timer slot and for the whole call the milliseconds of `calls` calls behind `warmup` untimed ones"""
    timing(1)
    dev, wall = [], []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if i >= warmup:
            dev.append(timing(-1)[:slots])
            wall.append((t1 - t0) * 1000.0)
    timing(0)
    dev = np.asarray(dev, dtype=np.float64)
    return [spread(dev[:, k]) for k in range(slots)], spread(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=513)
    ap.add_argument("--resolution", type=int, default=50)
    ap.add_argument("--clear-vox", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_timing.json"))
    a = ap.parse_args()
    res, tau = a.resolution, 1000
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=10, size=(a.map * res / 1000.0,) * 3))
    store = W.DeviceGlobalMap(tau, 0)
    tm = W.TSDFMapping(params, W.LocalMap(a.map, a.map, a.map, tau, 0, host_voxels=False), device_global_map=store)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (400.0, -300.0, 100.0)]):
        tm.update_tsdf(S.os1_128_scan(sensor_mm=sensor, seed=12345 + k), pos_rm=tuple(int(np.floor(c / res)) for c in sensor), up_rm=(0, 0, 32768))
    tm.global_surface_cloud(device=True)  # the window goes into the store
    n_chunks = store.count()
    store_bytes = n_chunks * 4 * 64 ** 3
    d2d = copy_ms(store_bytes, a.warmup, a.calls)
    read_once_ms = float(np.median(d2d)) / 2.0

    last = {}

    def ground():
        last["g"] = store.ground(clear_vox=a.clear_vox, device=True)
    (pass1, pass2), ground_wall = timed(ground, store.ground_timing, 2, a.warmup, a.calls)
    g = last["g"]
    (bridge0, bridge_x, bridge_y), bridge_wall = timed(lambda: store.ground_distance(256, max_dist_vox=20, device=True), store.distance_timing, 3, a.warmup, a.calls)
    (yard0, yard_x, yard_y), yard_wall = timed(lambda: store.distance(max_dist_vox=20, columns=True, device=True), store.distance_timing, 3, a.warmup, a.calls)
    out = dict(
        map=a.map, resolution=res, chunks=n_chunks, store_bytes=store_bytes, clear_vox=a.clear_vox, warmup=a.warmup, calls=a.calls,
        box=dict(lo=list(g.lo), ext=list(g.ext)), columns=int(g.ext[0]) * int(g.ext[1]), counts=[int(c) for c in g.counts],
        ground=dict(pass1_levels_ms=pass1, pass2_steps_ms=pass2, call_ms=ground_wall),
        ground_distance=dict(pass0_ms=bridge0, x_pass_ms=bridge_x, y_pass_ms=bridge_y, call_ms=bridge_wall),
        yardstick_distance_columns=dict(pass0_ms=yard0, x_pass_ms=yard_x, y_pass_ms=yard_y, call_ms=yard_wall),
        device_copy=dict(ms=spread(d2d), bytes_per_s=store_bytes / (float(np.median(d2d)) * 1e-3), read_once_ms=read_once_ms),
        pass1_over_yardstick=pass1["median"] / yard0["median"],
        pass1_bytes_per_s=store_bytes / (pass1["median"] * 1e-3),
        yardstick_bytes_per_s=store_bytes / (yard0["median"] * 1e-3),
        pass1_over_read_once=pass1["median"] / read_once_ms,
    )
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    store.close()


if __name__ == "__main__":
    main()
