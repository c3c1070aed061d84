"""Device time and call time of the scan pre-processing with one pose per scan (ws_scan_preprocess_dev) and with one pose per time bin
(ws_scan_preprocess_sweep_dev), on one device-resident cloud of 128 x 1024 points, interleaved in one session.

    python tools/sweep_timing.py [--bins 1024] [--reps 20] [--warmup 3] [--out profiles/sweep_timing.json] [--only-plain]

Variants: (a) plain; (b) sweep, ring-major (a wave's 64 lanes read 64 rows of the pose table); (c) sweep, column-major (one or two
rows per wave); (d) sweep, bins from a per-point time.  The same points in every variant (the column-major cloud is the ring-major one
transposed).  device_ms: HIP events on the library's stream around everything the call enqueues (memsets, the upload of the table, the
four launches, the read-back of the count); call_ms: wall clock of the call, which ends with a stream synchronise.  --only-plain runs
(a) alone, e.g. against another build of the library (WS_HIP_LIB)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--only-plain", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "sweep_timing.json"))
    args = ap.parse_args()
    import torch
    import warpsense_amd as W
    from warpsense_amd import synthetic as S

    rings, az = S.RINGS, S.AZIMUTHS
    begin, end = np.eye(4), np.eye(4)
    begin[:3, 3] = (1000.0, 500.0, 0.0)
    a = np.deg2rad(6.0)
    end[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    end[:3, 3] = (1250.0, 625.0, 0.0)
    ring_major = S.os1_128_sweep(begin, end, half_extents_mm=(22000.0, 16000.0, 2500.0), seed=1000, with_time=True)  # (131072, 4)
    col_major = np.ascontiguousarray(ring_major.reshape(rings, az, 4).transpose(1, 0, 2)).reshape(-1, 4)
    ctx = W.Context.default()
    ctx.use_torch_stream()
    pre = W.ScanPreprocessor(rings * az, ctx)
    d_ring, d_col = torch.from_numpy(ring_major).cuda(), torch.from_numpy(col_major).cuda()
    pose = end.astype(np.float32)
    variants = {"a_plain": lambda: pre.preprocess(d_ring, pose, args.res)}
    if not args.only_plain:
        poses = W.sweep_poses(end, np.linalg.inv(begin) @ end, args.bins)
        variants.update({
            "b_sweep_ring_major": lambda: pre.preprocess_sweep(d_ring, poses, args.res, columns=az, ring_major=True),
            "c_sweep_column_major": lambda: pre.preprocess_sweep(d_col, poses, args.res, columns=az, ring_major=False),
            "d_sweep_by_time": lambda: pre.preprocess_sweep(d_ring, poses, args.res, time_field=3),
        })
    dev = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    points = {}
    for rep in range(args.warmup + args.reps):
        for name, fn in variants.items():  # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            out = fn()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            points[name] = len(out)
            if rep >= args.warmup:
                dev[name].append(e0.elapsed_time(e1))
                wall[name].append(1000.0 * (t1 - t0))
    rows = {k: {"points_out": points[k], "device_ms": stats(dev[k]), "call_ms": stats(wall[k])} for k in variants}
    if not args.only_plain:  # the same points, whichever way the cloud is laid out or the bins are found
        by = {k: set(map(tuple, fn().to_host().tolist())) for k, fn in variants.items() if k != "a_plain"}
        assert by["b_sweep_ring_major"] == by["c_sweep_column_major"] == by["d_sweep_by_time"]
    doc = {"what": f"scan pre-processing of {rings * az} device-resident points at {args.res} mm, {args.bins} poses per sweep; {args.warmup} warm-up calls, "
                   f"medians of {args.reps} with min and max, variants interleaved; HIP events around the call and wall clock of the call",
           "library": os.environ.get("WS_HIP_LIB") or "in-tree build", "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(doc, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
