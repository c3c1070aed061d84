"""Device time of ws_store_raycast (store_raycast.hip) on the global map a run leaves behind, next to the numbers it has to be read
against, all in one session and interleaved:

  (a) from the LAST pose, 131 072 OS1-128 rays: march and gradient pass of ws_store_raycast by HIP events on the call's stream
      (ws_debug_store_raycast_timing), and ws_map_raycast on the window from the same pose and range by its own events: hit share
      and time per ray of both;
  (b) the same rays from the FIRST pose, which the window has left: ws_store_raycast end to end, against the only other route to
      that answer: ws_store_load_box of the box around the first pose into a second map plus ws_map_raycast on it, end to end,
      the second map's allocation reported apart.

The library under test is the one WS_HIP_LIB names (a -DWS_STORE_RAY_NO_JUMP variant of `python -m warpsense_amd.build --variant`,
measured in runs that alternate with the shipped build); --merge joins the runs' files into profiles/store_raycast_timing.json.
The stream is that of DESIGN §8f: python tools/store_raycast_timing.py --map 1024 --scans 60 --shift 2.0 --room 10 8 2.5
"""
import argparse
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


def merge(files, out):
    runs = [json.load(open(f)) for f in files]
    doc = {"what": runs[0]["what"], "runs_in_session_order": runs}
    with open(out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(out)


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
    ap.add_argument("--label", default="shipped")
    ap.add_argument("--merge", nargs="+", default=None, metavar="FILE", help="join the files of several runs into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_raycast_timing.json"))
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    import torch
    import warpsense_amd as W
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
    poses = []
    for P in (app.poses[-1], app.poses[0]):
        P = P.astype(np.float64).copy()
        P[:3, 3] /= 1000.0
        poses.append(P)
    last, first = poses
    dirs = S.os1_128_dirs()
    tm.global_raycast(last, dirs)  # the window into the chunks, once
    o_last, d = W.TSDFMapping.raycast_rays(last, dirs)
    o_first, _ = W.TSDFMapping.raycast_rays(first, dirs)
    d_dev = torch.from_numpy(d).cuda()
    rng = tm._global_range_mm(o_first)
    avg = tm.tsdf().avg_map()
    store.raycast_timing(1)
    tm.tsdf()._L.ws_debug_raycast_timing(tm.tsdf().handle, 1, None)

    def store_cast(o):
        store.raycast(args.res, o, d_dev, rng, gradient=True)
        return list(store.raycast_timing(-1))[1:], store.last_hits

    def window_cast(o):
        import ctypes as C
        avg.raycast(o, d_dev, rng, gradient=True)
        ms = (C.c_float * 3)()
        tm.tsdf()._L.ws_debug_raycast_timing(tm.tsdf().handle, -1, ms)
        return [float(ms[1]), float(ms[2])], avg.last_hits

    # the other route to the first pose's answer: a second map around it, loaded from the store
    t0 = time.perf_counter()
    lm2 = W.LocalMap(*(int(s) for s in tm.local_map_.size), int(params.map.tau), 0, host_voxels=False)
    lm2.pos[:] = np.floor_divide(o_first, args.res)
    t2 = W.TSDFCuda(lm2.device_map(), int(params.map.tau), int(params.map.max_weight), args.res)
    W.pause()
    alloc_s = time.perf_counter() - t0
    lo2, hi2 = lm2.window()

    def second_map_route():
        t0 = time.perf_counter()
        store.load_box(t2, lo2, hi2)
        rec, _ = t2.avg_map().raycast(o_first, d_dev, rng, gradient=True)
        return time.perf_counter() - t0, t2.avg_map().last_hits

    def store_route():
        t0 = time.perf_counter()
        store.raycast(args.res, o_first, d_dev, rng, gradient=True)
        return time.perf_counter() - t0, store.last_hits

    for _ in range(args.warmup):
        store_cast(o_last), window_cast(o_last), store_cast(o_first), second_map_route(), store_route()
    a_s, a_w, b_s, b_e2e, b_other = [], [], [], [], []
    for _ in range(args.repeats):
        ms, hits_last = store_cast(o_last)
        a_s.append(ms)
        ms, hits_window = window_cast(o_last)
        a_w.append(ms)
        ms, hits_first = store_cast(o_first)
        b_s.append(ms)
        s, hits_other = second_map_route()
        b_other.append(s)
        b_e2e.append(store_route()[0])
    a_s, a_w, b_s = np.array(a_s), np.array(a_w), np.array(b_s)
    n = len(d)
    doc = {
        "what": f"ws_store_raycast, {n} OS1-128 rays, on the store of {args.scans} scans through a {int(tm.local_map_.size[0])}^3 window @ {args.res} mm "
                f"(shift {args.shift} m, room {list(args.room)} m), range {rng} mm, with gradient",
        "label": args.label, "library": os.path.basename(os.environ.get("WS_HIP_LIB", "shipped")), "chunks": store.count(), "repeats": args.repeats, "warmup": args.warmup,
        "a_last_pose": {"store_march_ms": stats(a_s[:, 0]), "store_gradient_ms": stats(a_s[:, 1]), "store_hit_share": hits_last / n,
                        "store_ns_per_ray": 1e6 * float(np.median(a_s[:, 0])) / n,
                        "window_march_ms": stats(a_w[:, 0]), "window_gradient_ms": stats(a_w[:, 1]), "window_hit_share": hits_window / n,
                        "window_ns_per_ray": 1e6 * float(np.median(a_w[:, 0])) / n},
        "b_first_pose": {"store_march_ms": stats(b_s[:, 0]), "store_gradient_ms": stats(b_s[:, 1]), "store_hit_share": hits_first / n,
                         "store_end_to_end_s_with_download": stats(b_e2e),
                         "second_map_load_box_plus_raycast_end_to_end_s": stats(b_other), "second_map_hit_share": hits_other / n,
                         "second_map_allocation_s": alloc_s, "second_map_bytes": 2 * 4 * int(np.prod(tm.local_map_.size.astype(np.int64)))},
    }
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
