"""Device time of ws_map_distance (map_distance.hip) on the benchmark map, next to the first step of the only route the library
offered for the same purpose before, in one session and interleaved:

  (a) ws_map_distance over the whole window for R = 8, 40, 255 voxels, with and without WS_DISTANCE_COLUMNS: pass 0 and the three
      line passes by HIP events on the context's stream (ws_debug_distance_timing), their sum, and the bytes per second that sum
      stands for, counted as 4 B read + 4 B written per voxel, against the 8 TB/s peak of the HBM;
  (b) ws_map_download of the same map (the host transform over 135 M voxels that would have to follow is not timed).

    python tools/distance_timing.py [--map 512] [--repeats 20] [--warmup 3] [--out profiles/distance_timing.json]

Prints one JSON document (medians and min / max over the repeats)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=512, help="edge of the window in voxels (forced odd: 512 -> 513^3)")
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=5, help="repeats of ws_map_download")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import warpsense_amd as W
    from warpsense_amd import _lib
    from warpsense_amd import synthetic as S
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    tau, mw, res = 1000, 640, args.res
    lm = W.LocalMap(args.map, args.map, args.map, tau, 0, host_voxels=False)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        t.update_tsdf(torch.from_numpy(pts).cuda(), [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor], (0, 0, 32768))
    t.ctx.sync()
    L, h = t._L, t.handle
    n_vox = int(L.ws_map_n_voxels(h))
    ms = (C.c_float * 4)()
    sites = C.c_size_t(0)
    _lib.check(L.ws_debug_distance_timing(h, 1, None), "ws_debug_distance_timing")

    def device_times(R, flags):
        _lib.check(L.ws_map_distance(h, 0, None, None, R, flags, C.byref(sites)), "ws_map_distance")
        _lib.check(L.ws_debug_distance_timing(h, -1, ms), "ws_debug_distance_timing")
        return [float(v) for v in ms], int(sites.value)

    host_buf = np.empty(n_vox, dtype=np.uint32)
    size, pos, off = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)

    def download():
        t0 = time.perf_counter()
        _lib.check(L.ws_map_download(h, 0, size.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                     host_buf.ctypes.data_as(C.c_void_p)), "ws_map_download")
        return time.perf_counter() - t0

    cases = [(R, flags) for R in (8, 40, 255) for flags in (0, _lib.WS_DISTANCE_COLUMNS)]
    for _ in range(args.warmup):
        for R, flags in cases:
            device_times(R, flags)
    dev = {c: [] for c in cases}
    n_sites, dl = {}, []
    for r in range(args.repeats):
        for c in cases:  # interleaved
            tm, ns = device_times(*c)
            dev[c].append(tm)
            n_sites["columns" if c[1] else "voxels"] = ns
        if r < args.host_repeats:
            dl.append(download())
    _lib.check(L.ws_debug_distance_timing(h, 0, None), "ws_debug_distance_timing")

    def case(c):
        a = np.array(dev[c])
        total = a.sum(axis=1)
        out = {"pass0": stats(a[:, 0]), "x_pass": stats(a[:, 1]), "y_pass": stats(a[:, 2]), "z_pass": stats(a[:, 3]), "total": stats(total)}
        if not c[1]:
            bps = 8.0 * n_vox / (float(np.median(total)) * 1e-3)
            out["bytes_per_s_at_8B_per_voxel"] = bps
            out["share_of_8TBps_peak"] = bps / PEAK_BYTES_PER_S
        return out
    doc = {"what": f"ws_map_distance on the whole {int(lm.size[0])}^3 window @ {res} mm after two 131072-point scans, default class rule; HIP events",
           "voxels": n_vox, "map_bytes": 4 * n_vox, "sites": n_sites, "repeats": args.repeats, "warmup": args.warmup,
           "a_distance_device_ms": {f"R={R}{' columns' if flags else ''}": case((R, flags)) for R, flags in cases},
           "b_ws_map_download_s": stats(dl),
           "distance_R40_total_over_download_alone": float(np.median(np.array(dev[(40, 0)]).sum(axis=1))) * 1e-3 / float(np.median(dl))}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
