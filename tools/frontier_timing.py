"""Device time of ws_map_frontier (map_frontier.hip) on the benchmark map, next to ws_map_surface of the same box in the same process:
the four stages by HIP events on the context's stream (ws_debug_frontier_timing: count, scan, emit, clustering) against the three of
ws_debug_surface_timing, the records and clusters found, and the clustering's rate in records per second.

    python tools/frontier_timing.py [--map 512] [--repeats 10] [--warmup 2] [--out profiles/frontier_timing.json]

Prints one JSON document (medians and min / max over the repeats)."""
import argparse
import ctypes as C
import json
import os
import sys

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
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        t.update_tsdf(torch.from_numpy(pts).cuda(), [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor], (0, 0, 32768))
    t.ctx.sync()
    L, h = t._L, t.handle
    ms3, ms4 = (C.c_float * 3)(), (C.c_float * 4)()
    n, k = C.c_size_t(0), C.c_size_t(0)
    _lib.check(L.ws_debug_surface_timing(h, 1, None), "ws_debug_surface_timing")
    _lib.check(L.ws_debug_frontier_timing(h, 1, None), "ws_debug_frontier_timing")

    def surface():
        _lib.check(L.ws_map_surface(h, 0, None, None, 0, 0, C.byref(n)), "ws_map_surface")
        _lib.check(L.ws_debug_surface_timing(h, -1, ms3), "ws_debug_surface_timing")
        return [float(v) for v in ms3], int(n.value)

    def frontier(min_value, flags):
        _lib.check(L.ws_map_frontier(h, 0, None, None, min_value, flags, C.byref(n), C.byref(k)), "ws_map_frontier")
        _lib.check(L.ws_debug_frontier_timing(h, -1, ms4), "ws_debug_frontier_timing")
        return [float(v) for v in ms4], int(n.value), int(k.value)

    doc = {"what": f"ws_map_frontier on the {int(lm.size[0])}^3 window @ {res} mm after two 131072-point scans, whole window, next to ws_map_surface",
           "voxels": int(L.ws_map_n_voxels(h)), "repeats": args.repeats, "warmup": args.warmup}
    for _ in range(args.warmup):
        surface()
        frontier(0, _lib.WS_FRONTIER_CLUSTERS)
    surf = np.array([surface()[0] for _ in range(args.repeats)])
    doc["surface_ms"] = {"count": stats(surf[:, 0]), "scan": stats(surf[:, 1]), "emit": stats(surf[:, 2]), "total": stats(surf.sum(axis=1)), "points": surface()[1]}
    for name, min_value in (("min_value_0", 0), ("min_value_tau", tau)):
        runs = [frontier(min_value, _lib.WS_FRONTIER_CLUSTERS) for _ in range(args.repeats)]
        ms = np.array([r[0] for r in runs])
        records, clusters = runs[-1][1], runs[-1][2]
        table = t.avg_map().frontier(min_value=min_value, clusters=True)[2]
        cl = float(np.median(ms[:, 3]))
        doc["frontier_ms_" + name] = {
            "count": stats(ms[:, 0]), "scan": stats(ms[:, 1]), "emit": stats(ms[:, 2]), "clustering": stats(ms[:, 3]), "total": stats(ms.sum(axis=1)),
            "records": records, "clusters": clusters, "largest_cluster": int(table["count"].max()) if len(table) else 0,
            "clustering_records_per_s": records / (cl * 1e-3) if cl > 0 else None,
            "extraction_over_surface": float(np.median(ms[:, :3].sum(axis=1)) / np.median(surf.sum(axis=1)))}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
