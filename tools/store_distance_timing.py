"""Device time of ws_store_distance (store_distance.hip) next to ws_map_distance (map_distance.hip) on the same voxels, in one
session and interleaved: the benchmark window after two scans, saved whole into a device global map; the box is the window.

  Per pass by HIP events on the context's stream (ws_debug_distance_timing, ws_debug_store_distance_timing), for R = 8, 40, 255 voxels
  with and without WS_DISTANCE_COLUMNS.  The x, y and z passes are the same kernels on the same planes for both sources; pass 0 differs:
  the window's reads follow the ring, the store's are 256-byte aligned runs of its chunks, found through the call's chunk table
  (whose upload lies in front of the first event).  The yardstick is the window's figure of this session.

    python tools/store_distance_timing.py [--map 512] [--repeats 20] [--warmup 3] [--out profiles/store_distance_timing.json]

Prints one JSON document (medians and min / max over the repeats)."""
import argparse
import ctypes as C
import json
import os
import sys

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
    lm = W.LocalMap(args.map, args.map, args.map, tau, 0, host_voxels=False)
    t = W.TSDFCuda(lm.device_map(), tau, mw, res)
    for k, sensor in enumerate([(0.0, 0.0, 0.0), (180.0, -120.0, 40.0)]):
        pts = S.os1_128_scan(sensor_mm=sensor, seed=12345 + k)
        t.update_tsdf(torch.from_numpy(pts).cuda(), [int(np.floor(np.float32(s) / np.float32(res))) for s in sensor], (0, 0, 32768))
    store = W.DeviceGlobalMap(tau, 0)
    lo, hi = lm.window()
    store.save_box(t, lo, hi)
    t.ctx.sync()
    L, h, hs = t._L, t.handle, store.handle
    a, b = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    ms = (C.c_float * 4)()
    sites = C.c_size_t(0)
    _lib.check(L.ws_debug_distance_timing(h, 1, None), "ws_debug_distance_timing")
    _lib.check(L.ws_debug_store_distance_timing(hs, 1, None), "ws_debug_store_distance_timing")

    def window_times(R, flags):
        _lib.check(L.ws_map_distance(h, 0, pa, pb, R, flags, C.byref(sites)), "ws_map_distance")
        _lib.check(L.ws_debug_distance_timing(h, -1, ms), "ws_debug_distance_timing")
        return [float(v) for v in ms], int(sites.value)

    def store_times(R, flags):
        _lib.check(L.ws_store_distance(hs, pa, pb, R, flags, C.byref(sites)), "ws_store_distance")
        _lib.check(L.ws_debug_store_distance_timing(hs, -1, ms), "ws_debug_store_distance_timing")
        return [float(v) for v in ms], int(sites.value)

    cases = [(R, flags) for R in (8, 40, 255) for flags in (0, _lib.WS_DISTANCE_COLUMNS)]
    for _ in range(args.warmup):
        for c in cases:
            window_times(*c), store_times(*c)
    win, sto = {c: [] for c in cases}, {c: [] for c in cases}
    n_sites = {}
    for r in range(args.repeats):
        for c in cases:  # interleaved: window, store, window, ...
            tw, nw = window_times(*c)
            ts, ns = store_times(*c)
            assert nw == ns, (c, nw, ns)
            win[c].append(tw), sto[c].append(ts)
            n_sites["columns" if c[1] else "voxels"] = ns
    # the same bytes from both sources (fill_entry has weight 0 and every chunk the box overlaps is present)
    n = C.c_size_t(0)
    same = {}
    for c in ((8, 0), (8, _lib.WS_DISTANCE_COLUMNS)):
        window_times(*c), store_times(*c)
        pw, ps = L.ws_map_distance_dev(h, C.byref(n)), L.ws_store_distance_dev(hs, C.byref(n))
        shape = (int(n.value),)
        same["columns" if c[1] else "voxels"] = bool(torch.equal(W._abi._device_tensor(pw, shape, "<i4", t), W._abi._device_tensor(ps, shape, "<i4", store)))
    _lib.check(L.ws_debug_distance_timing(h, 0, None), "ws_debug_distance_timing")
    _lib.check(L.ws_debug_store_distance_timing(hs, 0, None), "ws_debug_store_distance_timing")

    def passes(times):
        v = np.array(times)
        return {"pass0": stats(v[:, 0]), "x_pass": stats(v[:, 1]), "y_pass": stats(v[:, 2]), "z_pass": stats(v[:, 3]), "total": stats(v.sum(axis=1))}

    def case(c):
        w, s = passes(win[c]), passes(sto[c])
        return {"window": w, "store": s, "store_over_window_median": {k: (s[k]["median"] / w[k]["median"] if w[k]["median"] > 0 else None) for k in w}}
    n_vox = int(np.prod(np.asarray(hi, dtype=np.int64) - np.asarray(lo, dtype=np.int64) + 1))
    doc = {"what": f"ws_map_distance and ws_store_distance on the whole {int(lm.size[0])}^3 window @ {res} mm after two 131072-point scans, the window "
                   "saved whole into the store, default class rule, interleaved in one session; device ms by HIP events",
           "voxels": n_vox, "chunks": store.count(), "sites": n_sites, "same_bytes": same, "repeats": args.repeats, "warmup": args.warmup,
           "cases": {f"R={R}{' columns' if flags else ''}": case((R, flags)) for R, flags in cases}}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    store.close()


if __name__ == "__main__":
    main()
