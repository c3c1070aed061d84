"""Device time of ws_map_raycast (map_raycast.hip) on the benchmark map, next to the one thing the library offered for the same
purpose before, in one session and interleaved:

  (a) ws_map_raycast_dev: 131 072 rays of the OS1-128 pattern from the map's origin, at max_range 10 m / 25 m / the window's
      diagonal, with and without the gradient: the march and the gradient pass by HIP events on the context's stream
      (ws_debug_raycast_timing), the hit share; the whole call end to end from host directions including the download of the
      records (host clock);
  (b) ws_map_download of the same map (the host march that would have to follow is not timed).

    python tools/raycast_timing.py [--map 512] [--repeats 20] [--warmup 3] [--out profiles/raycast_timing.json]

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
    origin, dirs = W.TSDFMapping.raycast_rays(np.eye(4), S.os1_128_dirs())
    dirs_dev = torch.from_numpy(dirs).cuda()
    diagonal = int(np.ceil(np.sqrt(3.0) * int(lm.size[0]) * res))
    ranges = {"10m": 10_000, "25m": 25_000, "diagonal": diagonal}
    ms = (C.c_float * 3)()
    hits = C.c_size_t(0)
    o3 = np.ascontiguousarray(origin, dtype=np.int32)
    _lib.check(L.ws_debug_raycast_timing(h, 1, None), "ws_debug_raycast_timing")

    def device_times(max_range, flags):
        _lib.check(L.ws_map_raycast_dev(h, 0, o3.ctypes.data_as(C.c_void_p), C.c_void_p(dirs_dev.data_ptr()), len(dirs), max_range, flags, C.byref(hits)),
                   "ws_map_raycast_dev")
        _lib.check(L.ws_debug_raycast_timing(h, -1, ms), "ws_debug_raycast_timing")
        return [float(ms[1]), float(ms[2])], int(hits.value)

    def end_to_end(max_range):
        t0 = time.perf_counter()
        rec, _ = t.avg_map().raycast(origin, dirs, max_range)
        return time.perf_counter() - t0

    host_buf = np.empty(n_vox, dtype=np.uint32)
    size, pos, off = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)

    def download():
        t0 = time.perf_counter()
        _lib.check(L.ws_map_download(h, 0, size.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                     host_buf.ctypes.data_as(C.c_void_p)), "ws_map_download")
        return time.perf_counter() - t0

    cases = [(name, rng, flags) for name, rng in ranges.items() for flags in (0, _lib.WS_RAYCAST_GRADIENT)]
    for _ in range(args.warmup):
        for name, rng, flags in cases:
            device_times(rng, flags)
        end_to_end(diagonal)
    dev = {(name, flags): [] for name, _, flags in cases}
    hit_share, e2e, dl = {}, [], []
    for r in range(args.repeats):
        for name, rng, flags in cases:  # interleaved
            tm, nh = device_times(rng, flags)
            dev[(name, flags)].append(tm)
            hit_share[name] = nh / len(dirs)
        e2e.append(end_to_end(diagonal))
        if r < args.host_repeats:
            dl.append(download())
    _lib.check(L.ws_debug_raycast_timing(h, 0, None), "ws_debug_raycast_timing")
    doc = {"what": f"ws_map_raycast_dev on the {int(lm.size[0])}^3 window @ {res} mm after two 131072-point scans: {len(dirs)} rays of the OS1-128 pattern "
                   "from the origin, weight > 0",
           "voxels": n_vox, "map_bytes": 4 * n_vox, "rays": len(dirs), "output_bytes": 16 * len(dirs), "repeats": args.repeats, "warmup": args.warmup,
           "max_range_mm": ranges, "hit_share": hit_share,
           "a_raycast_device_ms": {name: {"march": stats(np.array(dev[(name, 0)])[:, 0]),
                                          "march_with_gradient_flag": stats(np.array(dev[(name, 2)])[:, 0]),
                                          "gradient_pass": stats(np.array(dev[(name, 2)])[:, 1])} for name in ranges},
           "a_raycast_end_to_end_s_host_dirs_and_download_diagonal": stats(e2e),
           "b_ws_map_download_s": stats(dl),
           "download_alone_over_raycast_end_to_end": float(np.median(dl)) / float(np.median(e2e))}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
