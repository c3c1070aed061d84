"""Device time of ws_map_surface (map_surface.hip) on the benchmark map, next to the two numbers it has to be read against:

  (a) ws_map_surface: the three launches by HIP events on the context's stream (ws_debug_surface_timing), bytes read and
      written, the resulting TB/s; and the whole call end to end including the download of the records (host clock);
  (b) the only other route to the same answer, interleaved with (a): ws_map_download of the whole window plus the numpy
      predicate and nonzero;
  (c) the project's own dense-stream rate in the same session: integrate_dense_kernel by ws_prof_read(WS_K_INTEGRATE)
      (16 bytes per voxel: two maps read, two written).

    python tools/surface_timing.py [--map 512] [--repeats 20] [--warmup 3] [--out profiles/surface_timing.json]

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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=5, help="repeats of the download + numpy route (seconds each)")
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
    n_cols = int(lm.size[0]) * int(lm.size[1])
    ms = (C.c_float * 3)()
    n = C.c_size_t(0)
    _lib.check(L.ws_debug_surface_timing(h, 1, None), "ws_debug_surface_timing")

    def device_times(flags):
        _lib.check(L.ws_map_surface(h, 0, None, None, 0, flags, C.byref(n)), "ws_map_surface")
        _lib.check(L.ws_debug_surface_timing(h, -1, ms), "ws_debug_surface_timing")
        return [float(ms[0]), float(ms[1]), float(ms[2])]

    host_buf = np.empty(n_vox, dtype=np.uint32)
    size, pos, off = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)

    def host_route():
        t0 = time.perf_counter()
        _lib.check(L.ws_map_download(h, 0, size.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                     host_buf.ctypes.data_as(C.c_void_p)), "ws_map_download")
        t1 = time.perf_counter()
        v = (host_buf & 0xFFFF).astype(np.uint16).view(np.int16)
        w = (host_buf >> 16).astype(np.uint16).view(np.int16)
        idx = np.nonzero((w > 0) & (np.abs(v.astype(np.int32)) < tau))[0]
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, int(idx.size)

    def end_to_end(marker):
        t0 = time.perf_counter()
        out = t.avg_map().surface(marker=marker)
        return time.perf_counter() - t0, len(out[0] if marker else out)

    for _ in range(args.warmup):
        device_times(0)
        device_times(1)
        end_to_end(False)
    rec_t, mk_t, e2e_rec, e2e_mk, dl, npy = [], [], [], [], [], []
    points = host_points = None
    for r in range(args.repeats):
        rec_t.append(device_times(0))
        mk_t.append(device_times(1))
        points = int(n.value)
        e2e_rec.append(end_to_end(False)[0])
        e2e_mk.append(end_to_end(True)[0])
        if r < args.host_repeats:  # interleaved with (a)
            a, b, host_points = host_route()
            dl.append(a)
            npy.append(b)
    assert host_points == points, (host_points, points)
    _lib.check(L.ws_debug_surface_timing(h, 0, None), "ws_debug_surface_timing")

    # (c) the dense integrate stream on this map, same session
    t.set_integrate(W.WS_INTEGRATE_DENSE)
    t.ctx.prof_enable(1 << _lib.WS_K_INTEGRATE)
    for _ in range(args.warmup):
        t.integrate()
    t.ctx.prof_reset()
    dense = []
    for _ in range(args.repeats):
        t.integrate()
        msd, cnt = t.ctx.prof_read(_lib.WS_K_INTEGRATE)
        t.ctx.prof_reset()
        dense.append(msd / max(cnt, 1))
    t.ctx.prof_enable(0)

    rec_t, mk_t = np.array(rec_t), np.array(mk_t)
    map_bytes = 4 * n_vox
    blocks = (n_cols + 15) // 16
    count_bytes = map_bytes + 4 * n_cols + 4 * blocks
    emit_rec_bytes = map_bytes + 4 * n_cols + 8 * blocks + 16 * points
    emit_mk_bytes = emit_rec_bytes + 28 * points
    tbs = lambda b, ms_: b / (ms_ * 1e-3) / 1e12  # noqa: E731
    dense_tbs = tbs(16 * n_vox, float(np.median(dense)))
    count_med, emit_med, emit_mk_med = float(np.median(rec_t[:, 0])), float(np.median(rec_t[:, 2])), float(np.median(mk_t[:, 2]))
    read_tbs = tbs(2 * map_bytes, count_med + emit_med)
    host_total = float(np.median(dl)) + float(np.median(npy))
    doc = {
        "what": f"ws_map_surface on the {int(lm.size[0])}^3 window @ {res} mm after two 131072-point scans, whole window, band = tau",
        "voxels": n_vox, "map_bytes": map_bytes, "points": points, "repeats": args.repeats, "warmup": args.warmup,
        "a_device_ms": {
            "count": stats(rec_t[:, 0]), "scan": stats(rec_t[:, 1]), "emit_records": stats(rec_t[:, 2]), "emit_records_and_marker": stats(mk_t[:, 2]),
            "total_records": stats(rec_t.sum(axis=1)), "total_records_and_marker": stats(mk_t.sum(axis=1)),
            "bytes": {"count": count_bytes, "emit_records": emit_rec_bytes, "emit_records_and_marker": emit_mk_bytes},
            "TBps": {"count": tbs(count_bytes, count_med), "emit_records": tbs(emit_rec_bytes, emit_med),
                     "emit_records_and_marker": tbs(emit_mk_bytes, emit_mk_med), "map_read_over_count_plus_emit": read_tbs}},
        "a_end_to_end_s": {"records_with_download": stats(e2e_rec), "records_and_marker_with_download": stats(e2e_mk)},
        "b_host_route_s": {"ws_map_download": stats(dl), "numpy_predicate_nonzero": stats(npy), "total_median": host_total},
        "b_over_a_end_to_end": host_total / float(np.median(e2e_rec)),
        "c_dense_integrate": {"ms": stats(dense), "bytes": 16 * n_vox, "TBps": dense_tbs},
        "a_read_bandwidth_over_c": read_tbs / dense_tbs,
    }
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
