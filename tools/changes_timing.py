#!/usr/bin/env python3
"""Timing of ws_store_changes on the benchmark map; writes profiles/changes_timing.json.

The workload of tools/fuse_timing.py: the 513^3 map of bench.py after two scans goes into a store (CUR) and is copied into a second
one (REF); an 8^3 block of occupied voxels stands at one place of observed free space in REF and at another in CUR (a displaced
object).  CUR is compared with REF under (a) the identity and (b) 5 degrees yaw + 2 degrees pitch + (13, -7, 4) mm.  Per case 3
warm-up calls, then 20 timed ones: the medians with minimum and maximum of the four timer slots (uploads + count pass, scan, emit
pass, clustering; HIP events, ws_debug_store_changes_timing) and of the call end to end (host clock around the synchronising call).

Two yardsticks that are not the code under test, in the same run: ws_store_fuse(..., WS_FUSE_COUNT_ONLY) on the same pair of stores
under the same pose (the same sampling work, its count pass from ws_debug_store_fuse_timing), and the traffic floor: CUR read once
at the rate of a device-to-device copy of CUR's size (a copy reads and writes every byte: half its time)."""
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
from fuse_timing import rot, spread  # noqa: E402


def copy_ms(n_bytes, warmup, calls):
    """device milliseconds of a device-to-device copy of n_bytes (torch events)"""
    import torch
    a, b = torch.empty(n_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    a.zero_()
    ms = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=513)
    ap.add_argument("--resolution", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "changes_timing.json"))
    a = ap.parse_args()
    res, tau = a.resolution, 1000
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=10, size=(a.map * res / 1000.0,) * 3))
    store, copy = W.DeviceGlobalMap(tau, 0), W.DeviceGlobalMap(tau, 0)
    tm = W.TSDFMapping(params, W.LocalMap(a.map, a.map, a.map, tau, 0, host_voxels=False), device_global_map=store)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (400.0, -300.0, 100.0)]):
        tm.update_tsdf(S.os1_128_scan(sensor_mm=sensor, seed=12345 + k), pos_rm=tuple(int(np.floor(c / res)) for c in sensor), up_rm=(0, 0, 32768))
    tm.global_surface_cloud(device=True)  # the window goes into the store
    keys = store.keys()
    best, best_free = None, -1
    for k in keys:
        c = store.chunk(k)
        copy.put_chunk(k, c)
        value, weight = (c & 0xFFFF).astype(np.uint16).view(np.int16), (c >> 16).astype(np.uint16).view(np.int16)
        free = ((value >= tau) & (weight > 0)).reshape(64, 64, 64)
        n_free = int(free[8:16, 8:16, 8:16].sum()) + int(free[24:32, 24:32, 24:32].sum())
        if n_free > best_free:
            best, best_free = k, n_free
    block = np.uint32((20 << 16) | 0)  # value 0, weight 20
    now, before = store.chunk(best).reshape(64, 64, 64), store.chunk(best).reshape(64, 64, 64)
    now[24:32, 24:32, 24:32] = block
    before[8:16, 8:16, 8:16] = block
    store.put_chunk(best, now)
    copy.put_chunk(best, before)
    cur_bytes = len(keys) * 4 * 64 ** 3
    d2d = copy_ms(cur_bytes, a.warmup, a.calls)
    floor_ms = float(np.median(d2d)) / 2.0
    mw = params.map.max_weight
    out = dict(map=a.map, resolution=res, band=res, free_value=tau, chunks_per_store=len(keys), object_chunk=list(best), object_free_voxels=best_free,
               cur_bytes=cur_bytes, d2d_copy_ms=spread(d2d), traffic_floor_ms=floor_ms, cases={})
    centre = (0.0, 0.0, 0.0)
    for name, T in (("identity", np.eye(4)), ("yaw5_pitch2_t13_-7_4", rot(5, 2, (13, -7, 4)))):
        store.changes_timing(1)
        rows = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            r = store.changes(copy, T, centre, resolution=res, band=res, free_value=tau, clusters=True)
            wall = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                rows.append((*store.changes_timing(), wall))
        store.changes_timing(0)
        rows = np.asarray(rows)
        store.fuse_timing(1)
        fuse_rows = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            fs = store.fuse(copy, T, mw, count_only=True, pivot_src_mm=centre, resolution=res)
            wall = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                fuse_rows.append((*store.last_fuse_timing, wall))
        store.fuse_timing(0)
        fuse_rows = np.asarray(fuse_rows)
        count, fuse_count = float(np.median(rows[:, 0])), float(np.median(fuse_rows[:, 1]))
        out["cases"][name] = dict(stats=r.stats.as_tuple(), records=len(r.records), clusters=len(r.clusters),
                                  count_ms=spread(rows[:, 0]), scan_ms=spread(rows[:, 1]), emit_ms=spread(rows[:, 2]), cluster_ms=spread(rows[:, 3]),
                                  end_to_end_ms=spread(rows[:, 4]),
                                  fuse_count_only=dict(stats=fs.as_tuple(), plan_ms=spread(fuse_rows[:, 0]), count_ms=spread(fuse_rows[:, 1]),
                                                       end_to_end_ms=spread(fuse_rows[:, 3])),
                                  count_over_fuse_count=count / fuse_count, count_over_traffic_floor=count / floor_ms,
                                  end_to_end_over_fuse_end_to_end=float(np.median(rows[:, 4])) / float(np.median(fuse_rows[:, 3])))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
