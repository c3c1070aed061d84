"""Device time of ws_store_mesh (store_mesh.hip) on the global map a run leaves behind, next to the numbers it has to be read
against, all in one session and interleaved:

  (a) ws_store_mesh on the store after TSDFMapping.global_mesh's save: the count passes (bits, cells, quads), the scan and the emit
      passes (vertices, faces) by HIP events on the call's stream (ws_debug_store_mesh_timing);
  (b) ws_map_mesh on the window alone, by its own events: the per-voxel rate of the bits pass on both layouts;
  (c) the parent's only route to the voxels outside the window: the wall time of fetching every chunk with ws_store_get_chunk
      (every host mesher pays this first).

The stream is that of DESIGN §8f: python tools/store_mesh_timing.py --map 1024 --scans 60 --shift 2.0 --room 10 8 2.5
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
    ap.add_argument("--fetch-repeats", type=int, default=3, help="repeats of (c), interleaved with the first repeats of (a) and (b)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_mesh_timing.json"))
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
    t0 = time.perf_counter()
    gv, gf = tm.global_mesh()
    first_call_s = time.perf_counter() - t0
    keys = store.keys()
    lo, hi = tm.local_map_.window()
    inside = [k for k in keys if all(k[d] * 64 + 63 >= lo[d] and k[d] * 64 <= hi[d] for d in range(3))]
    L, sh, mh = store._L, store.handle, tm.tsdf().handle
    ms = (C.c_float * 3)()
    nv, nf = C.c_size_t(0), C.c_size_t(0)
    _lib.check(L.ws_debug_store_mesh_timing(sh, 1, None), "ws_debug_store_mesh_timing")
    _lib.check(L.ws_debug_mesh_timing(mh, 1, None), "ws_debug_mesh_timing")

    def store_times():
        _lib.check(L.ws_store_mesh(sh, None, None, args.res, 0, C.byref(nv), C.byref(nf)), "ws_store_mesh")
        _lib.check(L.ws_debug_store_mesh_timing(sh, -1, ms), "ws_debug_store_mesh_timing")
        return [float(ms[0]), float(ms[1]), float(ms[2])]

    def window_times():
        _lib.check(L.ws_map_mesh(mh, 0, None, None, 0, C.byref(nv), C.byref(nf)), "ws_map_mesh")
        _lib.check(L.ws_debug_mesh_timing(mh, -1, ms), "ws_debug_mesh_timing")
        return [float(ms[0]), float(ms[1]), float(ms[2])], int(nv.value), int(nf.value)

    def end_to_end():
        t0 = time.perf_counter()
        v, f = store.mesh(args.res)
        return time.perf_counter() - t0

    buf = np.empty(64 ** 3, dtype=np.uint32)
    found = C.c_int32(0)
    key_arr = np.asarray(keys, dtype=np.int32).reshape(-1, 3)

    def fetch_all():
        t0 = time.perf_counter()
        for k in key_arr:
            _lib.check(L.ws_store_get_chunk(sh, k.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), C.byref(found)), "ws_store_get_chunk")
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        store_times(), window_times(), end_to_end()
    st, wt, e2e, fetch = [], [], [], []
    for r in range(args.repeats):
        st.append(store_times())
        w, wv, wf = window_times()
        wt.append(w)
        e2e.append(end_to_end())
        if r < args.fetch_repeats:
            fetch.append(fetch_all())
    _lib.check(L.ws_debug_store_mesh_timing(sh, 0, None), "ws_debug_store_mesh_timing")
    _lib.check(L.ws_debug_mesh_timing(mh, 0, None), "ws_debug_mesh_timing")
    st, wt = np.array(st), np.array(wt)
    chunk_voxels = len(keys) * 64 ** 3
    window_voxels = int(np.prod(tm.local_map_.size.astype(np.int64)))
    s_count, w_count = float(np.median(st[:, 0])), float(np.median(wt[:, 0]))
    doc = {
        "what": f"ws_store_mesh on the store of {args.scans} scans through a {int(tm.local_map_.size[0])}^3 window @ {args.res} mm (shift {args.shift} m, room "
                f"{list(args.room)} m), default box, weight > 0, after global_mesh's save",
        "chunks": len(keys), "chunks_overlapping_the_window": len(inside), "chunk_voxels": chunk_voxels, "window_voxels": window_voxels,
        "vertices": int(len(gv)), "faces": int(len(gf)), "repeats": args.repeats, "warmup": args.warmup,
        "scratch_bytes": 29 * 4096 * len(keys), "first_global_mesh_call_s": first_call_s,
        "a_store_mesh_device_ms": {"count": stats(st[:, 0]), "scan": stats(st[:, 1]), "emit": stats(st[:, 2]), "total": stats(st.sum(axis=1)),
                                   "voxels_per_ns_over_count": chunk_voxels / (s_count * 1e6)},
        "a_store_mesh_end_to_end_s_with_download": stats(e2e),
        "b_window_mesh_device_ms": {"count": stats(wt[:, 0]), "scan": stats(wt[:, 1]), "emit": stats(wt[:, 2]), "total": stats(wt.sum(axis=1)),
                                    "vertices": wv, "faces": wf, "voxels_per_ns_over_count": window_voxels / (w_count * 1e6)},
        "store_over_window_voxels_per_ns": (chunk_voxels / s_count) / (window_voxels / w_count),
        "c_fetch_every_chunk_s": stats(fetch),
        "fetch_over_store_mesh_end_to_end": float(np.median(fetch)) / float(np.median(e2e)),
    }
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
