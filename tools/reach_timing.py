"""Device and host time of ws_map_reach (map_reach.hip) on the benchmark map, next to ws_map_distance of the same box in the same
process: the three spans by HIP events (ws_debug_reach_timing: seeding, all rounds, count), the wall time of the call, the rounds and
the tiles listed per round (ws_debug_reach_active), the records reached, and 64 paths in one launch.  Two cases: the volume at
max_dist_vox 8 with clear_d2 4, and the WS_DISTANCE_COLUMNS cost map.  The seed is the sensor of the second scan.

    python tools/reach_timing.py [--map 512] [--repeats 10] [--warmup 2] [--out profiles/reach_timing.json]

Prints one JSON document (medians and min / max over the repeats)."""
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
    ap.add_argument("--map", type=int, default=512, help="edge of the window in voxels (forced odd: 512 -> 513^3)")
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
    sensors = [(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]
    for k, sensor in enumerate(sensors):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        t.update_tsdf(torch.from_numpy(pts).cuda(), [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor], (0, 0, 32768))
    t.ctx.sync()
    L, h = t._L, t.handle
    seed = np.array([[int(np.floor(np.float32(s) / np.float32(res))) for s in sensors[-1]]], dtype=np.int32)
    ms3, ms4 = (C.c_float * 3)(), (C.c_float * 4)()
    sites, kept, reached, rounds, n = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint32(0), C.c_size_t(0)
    _lib.check(L.ws_debug_distance_timing(h, 1, None), "ws_debug_distance_timing")
    _lib.check(L.ws_debug_reach_timing(h, 1, None), "ws_debug_reach_timing")

    def distance(R, flags):
        _lib.check(L.ws_map_distance(h, 0, None, None, R, flags, C.byref(sites)), "ws_map_distance")
        _lib.check(L.ws_debug_distance_timing(h, -1, ms4), "ws_debug_distance_timing")
        return sum(float(v) for v in ms4)

    def reach(clear_d2):
        t0 = time.perf_counter()
        _lib.check(L.ws_map_reach(h, seed.ctypes.data_as(C.c_void_p), 1, clear_d2, 0, 0, C.byref(kept), C.byref(reached), C.byref(rounds)), "ws_map_reach")
        wall = (time.perf_counter() - t0) * 1e3
        _lib.check(L.ws_debug_reach_timing(h, -1, ms3), "ws_debug_reach_timing")
        return [float(v) for v in ms3] + [wall]

    doc = {"what": f"ws_map_reach on the {int(lm.size[0])}^3 window @ {res} mm after two 131072-point scans, whole window, one seed at the sensor, "
                   "next to ws_map_distance of the same box", "voxels": int(L.ws_map_n_voxels(h)), "repeats": args.repeats, "warmup": args.warmup}
    for name, R, flags, clear_d2 in (("volume_R8_clear4", 8, 0, 4), ("columns_R8_clear4", 8, _lib.WS_DISTANCE_COLUMNS, 4)):
        for _ in range(args.warmup):
            distance(R, flags)
            reach(clear_d2)
        dist = [distance(R, flags) for _ in range(args.repeats)]
        ms = np.array([reach(clear_d2) for _ in range(args.repeats)])
        _lib.check(L.ws_debug_reach_active(h, None, 0, C.byref(n)), "ws_debug_reach_active")
        active = np.zeros(n.value, dtype=np.uint32)
        _lib.check(L.ws_debug_reach_active(h, active.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "ws_debug_reach_active")
        cost = t.avg_map().reach(seed, clear_d2=clear_d2, device=True)
        finite = torch.nonzero(cost.reshape(-1) != -1).reshape(-1)
        goals = np.zeros((64, 3), dtype=np.int32)
        if len(finite):
            pick = finite[torch.linspace(0, len(finite) - 1, 64).long()].cpu().numpy()
            shape = tuple(cost.shape) + (1,) * (3 - cost.dim())
            goals = np.stack(np.unravel_index(pick, shape), axis=1)[:, :3].astype(np.int64)
            lo = np.zeros(3, dtype=np.int32)
            _lib.check(L.ws_map_reach_box(h, lo.ctypes.data_as(C.c_void_p), None, None), "ws_map_reach_box")
            goals = (goals + lo).astype(np.int32)
        t.ctx.sync()
        tp = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            hdr, _ = t.avg_map().reach_paths(goals, 2048)
            tp.append((time.perf_counter() - t0) * 1e3)
        rounds_ms = float(np.median(ms[:, 1]))
        doc[name] = {
            "distance_ms": stats(dist), "seeding_ms": stats(ms[:, 0]), "rounds_ms": stats(ms[:, 1]), "count_ms": stats(ms[:, 2]), "call_wall_ms": stats(ms[:, 3]),
            "host_share_of_call": float(1.0 - np.median(ms[:, :3].sum(axis=1)) / np.median(ms[:, 3])),
            "rounds": int(rounds.value), "ms_per_round": rounds_ms / max(int(rounds.value), 1),
            "active_tiles_per_round": {"min": int(active.min()) if len(active) else 0, "median": float(np.median(active)) if len(active) else 0.0,
                                       "max": int(active.max()) if len(active) else 0, "total": int(active.sum())},
            "records": int(cost.numel()), "seeded": int(kept.value), "reached": int(reached.value),
            "paths_64_wall_ms_cap_2048": stats(tp), "paths_reached": int(np.count_nonzero(hdr["status"] == 0)), "longest_path_steps": int(hdr["steps"].max())}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
