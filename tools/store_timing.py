"""Device and scan-path time of a map shift through the device global map (ws_shift_device, map_store.hip) next to the asynchronous
host route (TSDFMapping.shift_map_async: ws_shift_begin + the revisit uploads of _shift_enter) on the same window and steps, and of
write_back through both.

    python tools/store_timing.py [--map 1025] [--step 40] [--out profiles/store_timing.json] [--no-write-back]

Per direction (x, y, z, diagonal) three shifts: out into fresh space, back (a revisit: the entering slab is loaded from chunks that
exist), and out again (every chunk exists).  Device times are HIP events around the save and the load launches
(ws_debug_store_timing); wall clock is the duration of the call on the scan path.  bytes = 8 per leaving voxel + 8 per entering
voxel (each is read once and written once); a save into new chunks also writes the rest of those chunks."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_RATE_TBS = 6.29  # measured float4 copy on this device class


def sequence(step):
    s = step
    out = []
    for name, d in (("x", (s, 0, 0)), ("y", (0, s, 0)), ("z", (0, 0, s)), ("diagonal", (s, s, s))):
        out += [(name, "fresh", d), (name, "back", (0, 0, 0)), (name, "again", d), (name, "home", (0, 0, 0))]
    return out


def slab_voxels(size, a, b):
    """voxels that leave (= that enter) when the window moves from a to b, axis by axis"""
    n = 0
    for k in range(3):
        if a[k] != b[k]:
            n += abs(b[k] - a[k]) * int(np.prod([size[j] for j in range(3) if j != k]))
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=1025)
    ap.add_argument("--step", type=int, default=40)
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "store_timing.json"))
    ap.add_argument("--no-write-back", action="store_true")
    args = ap.parse_args()
    import warpsense_amd as W

    tau = 1000
    size_m = args.map * args.res / 1000.0
    params = W.Params(W.MapParams(resolution=args.res, max_distance=1.0, max_weight=10, size=(size_m,) * 3))
    rows = []

    def run(route):
        lm = W.LocalMap(args.map, args.map, args.map, tau, 0, host_voxels=False)
        size = [int(v) for v in lm.size]
        store = W.DeviceGlobalMap(tau, 0) if route == "device" else None
        tm = W.TSDFMapping(params, lm, device_global_map=store)
        shift = tm.shift_map_device if route == "device" else tm.shift_map_async
        if store is not None:
            store.reserve(6 * ((size[0] + 63) // 64 + 1) ** 2 + 64)  # no shift below allocates
            store.timing(1)
        else:
            tm.reserve_shift(args.step)
        # warm-up: one step out and back along -x (kernels loaded, staging touched), not part of the table
        for p in ((-args.step, 0, 0), (0, 0, 0)):
            shift(p)
            tm.wait_shift()
            W.pause()
        pos = (0, 0, 0)
        for name, kind, new_pos in sequence(args.step):
            W.pause()
            t0 = time.perf_counter()
            shift(new_pos)
            wall = time.perf_counter() - t0
            t1 = time.perf_counter()
            tm.wait_shift()
            W.pause()
            settled = time.perf_counter() - t1
            vox = slab_voxels(size, pos, new_pos)
            row = {"route": route, "direction": name, "kind": kind, "voxels_per_slab_set": vox, "scan_path_wall_ms": 1000.0 * wall,
                   "until_settled_ms": 1000.0 * settled}
            if store is not None:
                save_ms, load_ms = store.timing()
                row.update({"device_save_ms": save_ms, "device_load_ms": load_ms, "bytes": 16 * vox,
                            "device_tb_per_s": 16 * vox / ((save_ms + load_ms) * 1e-3) / 1e12 if save_ms + load_ms > 0 else None,
                            "chunks": store.count()})
            rows.append(row)
            print(json.dumps(row), flush=True)
            pos = new_pos
        wb = None
        if not args.no_write_back:
            W.pause()
            t0 = time.perf_counter()
            tm.write_back()
            wb = time.perf_counter() - t0
            print(json.dumps({"route": route, "write_back_s": wb, "host_chunks": len(lm.map_.chunks)}), flush=True)
        tm.tsdf().close()
        if store is not None:
            store.close()
        return wb

    wb_device = run("device")
    wb_host = run("async")
    doc = {"what": f"map shifts of {args.step} voxels on a {args.map}^3 window: device global map (ws_shift_device) and the asynchronous host route "
                   "(ws_shift_begin + revisit uploads on the scan path, slabs filed by a worker) on the same steps; HIP events and wall clock",
           "float4_copy_tb_per_s": COPY_RATE_TBS, "rows": rows,
           "write_back_s": {"device_global_map": wb_device, "host_route": wb_host}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
