"""Device time and wall clock of ws_map_sample / ws_store_sample (map_sample.hip, store_sample.hip) on the benchmark map, next to the two
routes the library offered for the same question before, in one session and interleaved:

  (a) records only            ws_map_sample_dev, 131 072 device-resident points of a benchmark scan
  (b) + gradient              WS_SAMPLE_GRADIENT
  (c) + FREE selection        WS_SAMPLE_SELECT_FREE
  (d) the store twin of (a)   ws_store_sample_dev, with the window saved into the store
  yardsticks                  TSDFMapping.scan_residual on the same points (a ray cast towards every point, records downloaded), and
                              ws_map_extract_box of the scan's bounding box (the numpy that would follow is not timed)

Device times are those of ws_debug_sample_timing (upload, sample pass, select passes); wall clock is that of the call, which
synchronises.  3 warm-up calls, medians of 20 with min .. max.

    python tools/sample_timing.py [--map 512] [--repeats 20] [--warmup 3] [--out profiles/sample_timing.json]"""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import warpsense_amd as W
    from warpsense_amd import _lib
    from warpsense_amd import synthetic as S
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    tau, mw, res = 1000, 640, args.res
    lm = W.LocalMap(args.map, args.map, args.map, tau, 0)
    size = tuple(int(s) for s in lm.size)
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(s * res / 1000.0 for s in size)))
    tm = W.TSDFMapping(params, lm)
    t = tm.tsdf()
    scans = []
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        scans.append(S.os1_128_scan(sensor_mm=sensor, seed=12345 + k))
        t.update_tsdf(torch.from_numpy(scans[k]).cuda(), [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor], (0, 0, 32768))
    t.ctx.sync()
    pts = np.ascontiguousarray(scans[0], dtype=np.int32)
    pts_dev = torch.from_numpy(pts).cuda()
    n = len(pts)
    store = W.DeviceGlobalMap(tau, 0)
    lo, hi = lm.window()
    store.save_box(t, lo, hi)
    t.ctx.sync()
    L, h = t._L, t.handle
    ms = (C.c_float * 3)()
    counts = np.zeros(4, dtype=np.uint64)
    cp = counts.ctypes.data_as(C.c_void_p)
    pp = C.c_void_p(pts_dev.data_ptr())
    _lib.check(L.ws_debug_sample_timing(h, 1, None), "ws_debug_sample_timing")
    _lib.check(L.ws_debug_store_sample_timing(store.handle, 1, None), "ws_debug_store_sample_timing")

    def window(flags):
        t0 = time.perf_counter()
        _lib.check(L.ws_map_sample_dev(h, 0, pp, n, 0, flags, cp), "ws_map_sample_dev")
        wall = time.perf_counter() - t0
        _lib.check(L.ws_debug_sample_timing(h, -1, ms), "ws_debug_sample_timing")
        return [float(ms[0]), float(ms[1]), float(ms[2]), 1000.0 * wall], counts.tolist()

    def store_call():
        t0 = time.perf_counter()
        _lib.check(L.ws_store_sample_dev(store.handle, None, None, pp, n, tau, res, 0, cp), "ws_store_sample_dev")
        wall = time.perf_counter() - t0
        _lib.check(L.ws_debug_store_sample_timing(store.handle, -1, ms), "ws_debug_store_sample_timing")
        return [float(ms[0]), float(ms[1]), float(ms[2]), 1000.0 * wall], counts.tolist()

    def residual():
        t0 = time.perf_counter()
        tm.scan_residual(pts_dev, np.eye(4))
        return 1000.0 * (time.perf_counter() - t0)

    b_lo, b_hi = np.maximum(pts.min(axis=0) // res, lo), np.minimum(pts.max(axis=0) // res, hi)

    def extract():
        t0 = time.perf_counter()
        t.avg_map().extract_box(b_lo, b_hi)
        return 1000.0 * (time.perf_counter() - t0)

    variants = {"a_records": 0, "b_gradient": _lib.WS_SAMPLE_GRADIENT, "c_free_selection": _lib.WS_SAMPLE_SELECT_FREE}
    for _ in range(args.warmup):
        for flags in variants.values():
            window(flags)
        store_call(), residual(), extract()
    got = {name: [] for name in list(variants) + ["d_store_records"]}
    cls = {}
    res_ms, ext_ms = [], []
    for _ in range(args.repeats):  # interleaved
        for name, flags in variants.items():
            tms, cls[name] = window(flags)
            got[name].append(tms)
        tms, cls["d_store_records"] = store_call()
        got["d_store_records"].append(tms)
        res_ms.append(residual())
        ext_ms.append(extract())
    _lib.check(L.ws_debug_sample_timing(h, 0, None), "ws_debug_sample_timing")
    col = lambda name, k: stats(np.array(got[name])[:, k])
    a_wall = float(np.median(np.array(got["a_records"])[:, 3]))
    doc = {"what": f"ws_map_sample_dev / ws_store_sample_dev on the {size[0]}^3 window @ {res} mm after two 131072-point scans: the {n} points of the first "
                   "scan, device-resident, band tau, weight > 0",
           "points": n, "repeats": args.repeats, "warmup": args.warmup, "store_chunks": len(store.keys()), "class_counts": cls,
           "variants_ms": {name: {"upload_device": col(name, 0), "sample_pass_device": col(name, 1), "select_passes_device": col(name, 2),
                                  "call_wall_clock": col(name, 3)} for name in got},
           "scan_residual_wall_clock_ms": stats(res_ms),
           "extract_box_wall_clock_ms": stats(ext_ms), "extract_box_voxels": int(np.prod((b_hi - b_lo + 1).astype(np.int64))),
           "scan_residual_over_a_wall_clock": float(np.median(res_ms)) / a_wall, "extract_box_over_a_wall_clock": float(np.median(ext_ms)) / a_wall}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
