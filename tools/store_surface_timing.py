"""Device time of ws_store_surface (store_surface.hip) on the global map a run leaves behind, next to the numbers it has to be read
against, all in one session and interleaved:

  (a) ws_store_surface on the store after TSDFMapping.global_mesh's save -- the store tools/store_mesh_timing.py builds --: the count
      passes (masks and their totals), the scan and the emit pass by HIP events on the call's stream (ws_debug_store_surface_timing),
      records only and with the marker; the effective bytes per second of the count passes against the store's size (one streaming
      read of every listed chunk: HBM bandwidth is the ceiling); the wall time of the call with its download;
  (b) the only route to the same cloud without it: ws_store_get_chunk over ws_store_keys and the predicate in numpy, by wall time
      (the records are not even assembled: fetch and predicate alone).

The stream is that of DESIGN §8f: python tools/store_surface_timing.py --map 1024 --scans 60 --shift 2.0 --room 10 8 2.5
"""
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
    ap.add_argument("--map", type=int, default=1024)
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--step", type=float, default=0.25)
    ap.add_argument("--shift", type=float, default=2.0)
    ap.add_argument("--room", type=float, nargs=3, default=(10.0, 8.0, 2.5))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=2, help="repeats of (b), interleaved with the first repeats of (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_surface_timing.json"))
    args = ap.parse_args()
    import torch
    import warpsense_amd as W
    from warpsense_amd import _lib
    from warpsense_amd import synthetic as S
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    size_m = args.map * args.res / 1000.0
    params = W.Params(W.MapParams(resolution=args.res, max_distance=1.0, max_weight=10, size=(size_m, size_m, size_m), shift=args.shift),
                      W.RegistrationParams(200, 0.1, 0.03))
    app = W.App(params, None, shift="device")
    he = tuple(1000.0 * r for r in args.room)
    for k in range(args.scans):
        sensor = np.array([1000.0 * args.step * k, 500.0 * args.step * k, 0.0])
        pts = S.os1_128_scan(sensor_mm=tuple(sensor), half_extents_mm=he, seed=1000 + k)
        app.cloud_callback(((pts.astype(np.float64) - sensor) / 1000.0).astype(np.float32))
    W.pause()
    tm, store = app.gpu_, app.gpu_.device_global_map_
    tau = tm.tsdf().tau_
    t0 = time.perf_counter()
    rec = tm.global_surface_cloud()  # the save of global_mesh, then the first call: its buffers are allocated here
    first_call_s = time.perf_counter() - t0
    keys = store.keys()
    L, sh = store._L, store.handle
    ms = (C.c_float * 3)()
    n = C.c_size_t(0)
    _lib.check(L.ws_debug_store_surface_timing(sh, 1, None), "ws_debug_store_surface_timing")

    def device_times(flags):
        _lib.check(L.ws_store_surface(sh, None, None, 0, tau, args.res, flags, C.byref(n)), "ws_store_surface")
        _lib.check(L.ws_debug_store_surface_timing(sh, -1, ms), "ws_debug_store_surface_timing")
        return [float(ms[0]), float(ms[1]), float(ms[2])]

    def end_to_end(marker):
        t0 = time.perf_counter()
        store.surface(tau, args.res, marker=marker)
        return time.perf_counter() - t0

    buf = np.empty(64 ** 3, dtype=np.uint32)
    found = C.c_int32(0)
    key_arr = np.asarray(keys, dtype=np.int32).reshape(-1, 3)

    def host_route():
        """the parent's route: every chunk over PCIe, the predicate on the host; returns (seconds in all, seconds of the fetches, points)"""
        t0 = time.perf_counter()
        fetch, points = 0.0, 0
        for k in key_arr:
            t1 = time.perf_counter()
            _lib.check(L.ws_store_get_chunk(sh, k.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), C.byref(found)), "ws_store_get_chunk")
            fetch += time.perf_counter() - t1
            value = (buf & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32)
            weight = (buf >> 16).astype(np.uint16).view(np.int16)
            points += int(np.count_nonzero((weight > 0) & (np.abs(value) < tau)))
        return time.perf_counter() - t0, fetch, points

    for _ in range(args.warmup):
        device_times(0), device_times(1), end_to_end(False), end_to_end(True)
    rt, mt, e2e, e2e_m, host = [], [], [], [], []
    for r in range(args.repeats):
        rt.append(device_times(0))
        mt.append(device_times(1))
        e2e.append(end_to_end(False))
        e2e_m.append(end_to_end(True))
        if r < args.host_repeats:
            host.append(host_route())
    _lib.check(L.ws_debug_store_surface_timing(sh, 0, None), "ws_debug_store_surface_timing")
    rt, mt, host = np.array(rt), np.array(mt), np.array(host)
    assert all(int(h[2]) == len(rec) for h in host), "the host route counts other points"
    chunk_bytes = len(keys) * 64 ** 3 * 4
    count_ms = float(np.median(rt[:, 0]))
    doc = {
        "what": f"ws_store_surface on the store of {args.scans} scans through a {int(tm.local_map_.size[0])}^3 window @ {args.res} mm (shift {args.shift} m, room "
                f"{list(args.room)} m), default box, band = tau, after global_mesh's save",
        "chunks": len(keys), "chunk_bytes": chunk_bytes, "points": int(len(rec)), "repeats": args.repeats, "warmup": args.warmup,
        "scratch_bytes": (8 * 4096 + 12 * 16) * len(keys), "first_global_surface_cloud_call_s": first_call_s,
        "a_records_device_ms": {"count": stats(rt[:, 0]), "scan": stats(rt[:, 1]), "emit": stats(rt[:, 2]), "total": stats(rt.sum(axis=1))},
        "a_marker_device_ms": {"count": stats(mt[:, 0]), "scan": stats(mt[:, 1]), "emit": stats(mt[:, 2]), "total": stats(mt.sum(axis=1))},
        "a_count_pass_bytes_per_s_against_the_store": chunk_bytes / (count_ms * 1e-3),
        "a_end_to_end_s_with_download": {"records": stats(e2e), "records_and_marker": stats(e2e_m)},
        "b_get_chunk_and_numpy_predicate_s": {"total": stats(host[:, 0]), "fetch_alone": stats(host[:, 1])},
        "host_route_over_store_surface_end_to_end": float(np.median(host[:, 0])) / float(np.median(e2e)),
    }
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
