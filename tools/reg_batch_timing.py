"""Wall and device time of ws_register_cloud_batch (reg_batch_kernel) next to the route the library offered for the same job
before -- K calls of ws_register_cloud, one after the other -- on the same handle, same poses, same process, interleaved:

  clouds of 16 384 and 131 072 points of the benchmark scene (synthetic OS1-128 scan in the 513^3 map @ 50 mm, the cloud moved by
  synthetic.perturbation()); K in {1, 4, 16, 64, 256, 512} start poses on a small lattice around the identity; per case the median
  over the repeats of (a) the wall time of one batch call, (b) the device time of its kernel (the context's WS_K_REG profiling
  class, HIP events), (c) the wall time of the K sequential calls; the break-even K; and (a), (b) for the kernel's variants
  (WS_REG_BATCH_VARIANT in the environment when the handle is created: 0 = all points streamed, 1 = two points per lane in
  registers with their voxel cache).

    python tools/reg_batch_timing.py [--map 512] [--repeats 5] [--warmup 1] [--out profiles/reg_batch_timing.json]

Prints one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
KS = (1, 4, 16, 64, 256, 512)
CLOUDS = (16384, 131072)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def lattice(k):
    """k start poses: the identity, then offsets of 20 mm / 0.25 degrees around it (all inside the basin of the benchmark's registration)"""
    from warpsense_amd import synthetic as S
    out = []
    for i in range(k):
        a, b, c = i % 5 - 2, (i // 5) % 5 - 2, (i // 25) % 21 - 10
        out.append(S.perturbation(20.0 * a, 20.0 * b, 0.0, 0.25 * c) if i else np.eye(4, dtype=np.float32))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=512)
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-k-sequential", type=int, default=512, help="largest K for which the K sequential calls are timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import warpsense_amd as W
    from warpsense_amd import _lib
    from warpsense_amd import synthetic as S
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    tau, mw, res = 1000, 640, args.res
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64, size=tuple(args.map * res / 1000.0 for _ in range(3))))
    lm = W.LocalMap(args.map, args.map, args.map, tau, 0, host_voxels=False)
    ctx = W.Context.default()
    tsdf = W.TSDFCuda(lm.device_map(), tau, mw, res, ctx)
    points = S.os1_128_scan()
    tsdf.update_tsdf(torch.from_numpy(points).cuda(), (0, 0, 0), (0, 0, 32768))
    ctx.sync()
    moved = S.transform_points_mm(points, S.perturbation())
    rp = params.registration
    prm = (rp.max_iterations, rp.it_weight_gradient, rp.epsilon, res)
    regs = {}
    for variant in (0, 1):
        os.environ["WS_REG_BATCH_VARIANT"] = str(variant)
        regs[variant] = W.RegistrationCuda(tsdf.device_map(), ctx)
    del os.environ["WS_REG_BATCH_VARIANT"]
    default_variant = 1  # what the library launches when the environment says nothing
    ctx.prof_enable(1 << _lib.WS_K_REG)

    def batch(reg, poses):
        ctx.prof_reset()
        t0 = time.perf_counter()
        T, it, e, c = reg.register_cloud_batch(tsdf.device_map(), poses, *prm)
        wall = time.perf_counter() - t0
        ms, n = ctx.prof_read(_lib.WS_K_REG)
        assert n == 1
        return wall, ms * 1e-3, T, it

    def sequential(reg, poses):
        t0 = time.perf_counter()
        out = [reg.register_cloud(tsdf.device_map(), P, *prm) for P in poses]
        return time.perf_counter() - t0, out

    doc = {"what": f"ws_register_cloud_batch against K sequential ws_register_cloud calls, {int(lm.size[0])}^3 map @ {res} mm, one 131072-point scan integrated, "
                   f"max_iterations {prm[0]}, it_weight_gradient {prm[1]}, epsilon {prm[2]}; seconds",
           "repeats": args.repeats, "warmup": args.warmup, "workgroup": "512 lanes (1024: the compiler spills 83-198 vector registers to scratch, not built)",
           "variant": "batch_*: two points per lane in registers with their voxel cache, the others streamed (the default); batch_streamed_*: every point streamed",
           "clouds": {}}
    for n_pts in CLOUDS:
        cloud = moved[:: len(moved) // n_pts][:n_pts]
        for reg in regs.values():
            reg.prepare_registration(cloud)
        rows = {}
        for k in KS:
            poses = lattice(k)
            seq_on = k <= args.max_k_sequential
            w = {0: [], 1: []}
            d = {0: [], 1: []}
            sq = []
            its = None
            for r in range(args.warmup + args.repeats):
                for variant, reg in regs.items():  # interleaved
                    wall, dev, T, it = batch(reg, poses)
                    if r >= args.warmup:
                        w[variant].append(wall)
                        d[variant].append(dev)
                    its = it
                if seq_on:
                    ctx.prof_enable(0)  # (events around every one of the K x 1 launches would be charged to the yardstick)
                    wall, out = sequential(regs[default_variant], poses)
                    ctx.prof_enable(1 << _lib.WS_K_REG)
                    if r >= args.warmup:
                        sq.append(wall)
                    assert all(np.array_equal(o[0], T[i]) and o[1] == its[i] for i, o in enumerate(out)), "batch != single"
            row = {"iterations_min_median_max": [int(its.min()), float(np.median(its)), int(its.max())],
                   "batch_wall_s": stats(w[default_variant]), "batch_kernel_s": stats(d[default_variant]),
                   "batch_streamed_wall_s": stats(w[0]), "batch_streamed_kernel_s": stats(d[0])}
            if sq:
                row["sequential_wall_s"] = stats(sq)
                row["sequential_over_batch"] = float(np.median(sq) / np.median(w[default_variant]))
            rows[str(k)] = row
            print(n_pts, k, json.dumps(row), flush=True)
        even = [k for k in KS if "sequential_over_batch" in rows[str(k)] and rows[str(k)]["sequential_over_batch"] > 1.0]
        doc["clouds"][str(n_pts)] = {"K": rows, "break_even_K": (min(even) if even else None)}
    ctx.prof_enable(0)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
