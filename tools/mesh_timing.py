"""Device time of ws_map_mesh (map_mesh.hip) on the benchmark map, next to the numbers it has to be read against, all in one
session and interleaved:

  (a) ws_map_mesh: the count passes (bits, cells, quads), the scan and the emit passes (vertices, faces) by HIP events on the
      context's stream (ws_debug_mesh_timing), bytes and the map-read rate of the count passes; the whole call end to end
      including the download of vertices and faces (host clock);
  (b) ws_map_surface on the same map: count / scan / emit (ws_debug_surface_timing);
  (c) the host route: ws_map_download alone, and download + the numpy model (tests/mesh_model.py) on the room box.

    python tools/mesh_timing.py [--map 512] [--repeats 20] [--warmup 3] [--out profiles/mesh_timing.json]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=512, help="edge of the window in voxels (forced odd: 512 -> 513^3)")
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=5, help="repeats of the download (+ numpy model) route")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import warpsense_amd as W
    from warpsense_amd import _lib
    from warpsense_amd import synthetic as S
    import mesh_model as M
    import query_model as QM
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
    sx, sy, sz = (int(v) for v in lm.size)
    n_words = sx * sy * ((sz + 63) // 64)
    ms = (C.c_float * 3)()
    nv, nf, n = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    _lib.check(L.ws_debug_mesh_timing(h, 1, None), "ws_debug_mesh_timing")
    _lib.check(L.ws_debug_surface_timing(h, 1, None), "ws_debug_surface_timing")

    def mesh_times():
        _lib.check(L.ws_map_mesh(h, 0, None, None, 0, C.byref(nv), C.byref(nf)), "ws_map_mesh")
        _lib.check(L.ws_debug_mesh_timing(h, -1, ms), "ws_debug_mesh_timing")
        return [float(ms[0]), float(ms[1]), float(ms[2])]

    def surface_times():
        _lib.check(L.ws_map_surface(h, 0, None, None, 0, 0, C.byref(n)), "ws_map_surface")
        _lib.check(L.ws_debug_surface_timing(h, -1, ms), "ws_debug_surface_timing")
        return [float(ms[0]), float(ms[1]), float(ms[2])]

    def end_to_end():
        t0 = time.perf_counter()
        v, f = t.avg_map().mesh()
        return time.perf_counter() - t0, len(v), len(f)

    host_buf = np.empty(n_vox, dtype=np.uint32)
    size, pos, off = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    room_lo, room_hi = (-205, -165, -55), (205, 165, 55)  # the synthetic room (10 x 8 x 2.5 m half extents) at 50 mm

    def host_route(with_model):
        t0 = time.perf_counter()
        _lib.check(L.ws_map_download(h, 0, size.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                     host_buf.ctypes.data_as(C.c_void_p)), "ws_map_download")
        t1 = time.perf_counter()
        counts = None
        if with_model:
            box = QM.ring_box(host_buf, size, pos, off, np.asarray(room_lo, dtype=np.int64), np.asarray(room_hi, dtype=np.int64))
            v, f = M.model_box(box, room_lo, res)
            counts = (len(v), len(f))
        return t1 - t0, time.perf_counter() - t1, counts

    for _ in range(args.warmup):
        mesh_times()
        surface_times()
        end_to_end()
    mesh_t, surf_t, e2e, dl, npy = [], [], [], [], []
    room_counts = None
    for r in range(args.repeats):
        mesh_t.append(mesh_times())
        surf_t.append(surface_times())
        e2e.append(end_to_end()[0])
        if r < args.host_repeats:  # interleaved with (a) and (b)
            a, b, c = host_route(with_model=r == 0)
            dl.append(a)
            if c is not None:
                npy.append(b)
                room_counts = c
    room_dev = t.avg_map().mesh(lo=room_lo, hi=room_hi)
    assert room_counts == (len(room_dev[0]), len(room_dev[1])), (room_counts, len(room_dev[0]), len(room_dev[1]))
    vertices, faces = int(nv.value), int(nf.value)
    _lib.check(L.ws_debug_mesh_timing(h, 0, None), "ws_debug_mesh_timing")
    _lib.check(L.ws_debug_surface_timing(h, 0, None), "ws_debug_surface_timing")

    mesh_t, surf_t = np.array(mesh_t), np.array(surf_t)
    map_bytes = 4 * n_vox
    blocks = (n_words + 255) // 256
    # bits: the map in, two planes out; cells: 16 words in (from the L2), one out; quads: ~12 words in, one byte and two totals out
    count_bytes = map_bytes + 16 * n_words + 8 * n_words + n_words + 8 * blocks
    tbs = lambda b, ms_: b / (ms_ * 1e-3) / 1e12  # noqa: E731
    count_med, surf_count_med = float(np.median(mesh_t[:, 0])), float(np.median(surf_t[:, 0]))
    doc = {
        "what": f"ws_map_mesh on the {sx}^3 window @ {res} mm after two 131072-point scans, whole window, weight > 0",
        "voxels": n_vox, "map_bytes": map_bytes, "vertices": vertices, "faces": faces, "repeats": args.repeats, "warmup": args.warmup,
        "launches": {"count": 3, "scan": 1, "emit": 2},
        "a_mesh_device_ms": {"count": stats(mesh_t[:, 0]), "scan": stats(mesh_t[:, 1]), "emit": stats(mesh_t[:, 2]), "total": stats(mesh_t.sum(axis=1)),
                             "count_bytes_written_and_map_read": count_bytes, "map_read_TBps_over_count": tbs(map_bytes, count_med),
                             "output_bytes": 16 * vertices + 12 * faces},
        "a_mesh_end_to_end_s_with_download": stats(e2e),
        "b_surface_device_ms": {"count": stats(surf_t[:, 0]), "scan": stats(surf_t[:, 1]), "emit": stats(surf_t[:, 2]), "points": int(n.value),
                                "map_read_TBps_over_count": tbs(map_bytes, surf_count_med)},
        "mesh_count_over_surface_count": count_med / surf_count_med,
        "c_host_route_s": {"ws_map_download": stats(dl), "numpy_model_on_the_room_box": stats(npy), "room_box": [room_lo, room_hi],
                           "room_vertices_faces": room_counts},
        "download_alone_over_mesh_end_to_end": float(np.median(dl)) / float(np.median(e2e)),
    }
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
