"""Time of ws_map_clearance (map_clearance.hip) next to its yardstick, ws_map_reach_lookup_dev on the same number of points, T P K, over
the same distance result in the same process: the lookup does the same scattered 4-byte gather per point with none of the arithmetic.
T = 4096 trajectories (a fan of arc_rollouts: 64 speeds x 64 yaw rates) of P = 32 poses and a body of K = 4 spheres, over a 256 x 256
column map and over a 128^3 volume of a window filled by two scans.  Per case: the wall time of the _dev call (poses in device memory),
of the host call (with its upload) and of the lookup, the three spans by HIP events (ws_debug_clearance_timing: upload, trajectory
pass, best), and the ratio of the _dev call to the lookup.

    python tools/clearance_timing.py [--repeats 20] [--warmup 3] [--out FILE]

Prints one JSON document (medians and min / max over the repeats) and writes it to FILE, profiles/clearance_timing.json by default."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "clearance_timing.json"))
    args = ap.parse_args()
    import torch
    import warpsense_amd as W
    from warpsense_amd import _lib
    from warpsense_amd import synthetic as S
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    tau, mw, res, R, soft = 1000, 640, args.res, 8, 200
    lm = W.LocalMap(257, 257, 129, tau, 0, host_voxels=False)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    sensors = [(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]
    for k, sensor in enumerate(sensors):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        t.update_tsdf(torch.from_numpy(pts).cuda(), [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor], (0, 0, 32768))
    t.ctx.sync()
    L, h, w = t._L, t.handle, t.avg_map()
    seed = np.array([[int(np.floor(np.float32(s) / np.float32(res))) for s in sensors[-1]]], dtype=np.int32)
    start = (sensors[-1][0] / 1000.0, sensors[-1][1] / 1000.0, sensors[-1][2] / 1000.0, 0.0)
    poses = W.arc_rollouts(start, np.linspace(0.1, 1.5, 64), np.linspace(-1.2, 1.2, 64), steps=32, dt=0.1)
    body = W.body_spheres([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [-0.3, 0.0, 0.0], [0.0, 0.0, 0.3]], [0.15, 0.12, 0.12, 0.1])
    T, P, K = poses.shape[0], poses.shape[1], len(body)
    assert (T, P, K) == (4096, 32, 4) and R * res >= 150 + soft
    points = np.ascontiguousarray(W.clearance_centres(poses, body, res).reshape(-1, 3))  # the voxels the call gathers from, in its order
    poses_dev, points_dev = torch.from_numpy(poses).cuda(), torch.from_numpy(points).cuda()
    cost_dev = torch.empty(len(points), dtype=torch.int32, device="cuda")
    ms3, best = (C.c_float * 3)(), C.c_int64(0)
    pp, bp = poses.ctypes.data_as(C.c_void_p), body.ctypes.data_as(C.c_void_p)
    _lib.check(L.ws_debug_clearance_timing(h, 1, None), "ws_debug_clearance_timing")

    def wall(call):
        t0 = time.perf_counter()
        _lib.check(call(), "call")
        return (time.perf_counter() - t0) * 1e3

    def clearance_dev():
        ms = wall(lambda: L.ws_map_clearance_dev(h, C.c_void_p(poses_dev.data_ptr()), T, P, bp, K, soft, 0, C.byref(best)))
        _lib.check(L.ws_debug_clearance_timing(h, -1, ms3), "ws_debug_clearance_timing")
        return [ms] + [float(v) for v in ms3]

    clearance_host = lambda: wall(lambda: L.ws_map_clearance(h, pp, T, P, bp, K, soft, 0, C.byref(best)))
    lookup = lambda: wall(lambda: L.ws_map_reach_lookup_dev(h, C.c_void_p(points_dev.data_ptr()), len(points), 3, C.c_void_p(cost_dev.data_ptr())))

    doc = {"what": f"ws_map_clearance_dev next to ws_map_reach_lookup_dev on T P K = {T * P * K} points over the same distance result, window 257 x 257 x 129 @ "
                   f"{res} mm after two 131072-point scans, max_dist_vox {R}, soft_mm {soft}", "T": T, "P": P, "K": K, "repeats": args.repeats, "warmup": args.warmup}
    c = np.zeros(3, dtype=np.int64)  # the boxes lie around the window's centre; the sensor of the second scan, where the fan starts, is a few voxels from it
    cases = (("columns_256x256", dict(lo=(c[0] - 128, c[1] - 128, c[2] - 4), hi=(c[0] + 127, c[1] + 127, c[2] + 12), columns=True)),
             ("volume_128", dict(lo=tuple(c - 64), hi=tuple(c + 63), columns=False)))
    for name, box in cases:
        rec = w.distance(max_dist_vox=R, device=True, **box)
        w.reach(seed, clear_d2=4, device=True)  # the lookup reads the costs of a reach result over the same box
        for _ in range(args.warmup):
            clearance_dev(), clearance_host(), lookup()
        dev = np.array([clearance_dev() for _ in range(args.repeats)])
        host = [clearance_host() for _ in range(args.repeats)]
        look = [lookup() for _ in range(args.repeats)]
        out = w.clearance(poses_dev, body, soft)
        doc[name] = {"records": int(rec.numel()), "clearance_dev_wall_ms": stats(dev[:, 0]), "upload_ms": stats(dev[:, 1]), "trajectories_ms": stats(dev[:, 2]),
                     "best_ms": stats(dev[:, 3]), "clearance_host_wall_ms": stats(host), "reach_lookup_dev_wall_ms": stats(look),
                     "ratio_dev_wall_to_lookup_wall": float(np.median(dev[:, 0]) / np.median(look)),
                     "samples_per_us_in_the_trajectory_pass": float(T * P * K / (np.median(dev[:, 2]) * 1e3)),
                     "trajectories_with_a_hit": int(np.count_nonzero(out.records["hits"])), "with_outside_samples": int(np.count_nonzero(out.records["outside"])),
                     "best": int(out.best)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
