#!/usr/bin/env python3
"""bench.py — scans/s of the warpsense hot path (TSDF update + Point-to-TSDF registration) on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full                 (+ every figure beyond the timed steps, see below)
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR     (+ what the last timed step computed, as .npy files)
    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: starts the N ranks itself, self_launch)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One step = one synthetic OS1-128 scan (131 072 points) through
    TSDFCuda::update_tsdf  (ray-march scatter + integrate into the 513^3 map @ 50 mm)  and
    TSDFRegistration::register_cloud (Gauss-Newton to convergence against that map),
with the scan already resident in HBM.  N > 1: every rank keeps a replica of the map and applies the full
scan; the registration points are sharded by index and the ranks' 44-word normal equations meet every iteration
-- device to device through mailboxes in each other's HBM (the resident loop of ws_register_cloud_peers; RCCL
all-reduce per iteration as the fallback) — total work is fixed, so "scaling" is "strong".
The same line also carries `replica_scans_per_s`: N independent sensor streams, one per GPU (weak scaling, the
deployment DESIGN.md §6 recommends for clouds of this size), clearly labelled and never used as `value`.

Rank 0 prints ONE JSON line (see the driver contract).  A plain run sets up, warms up, times the steps and prints it; everything
else the benchmark measures runs only with --full, after the timed steps: per-class kernel times and the roofline, the
dense-equivalent leg, the registration loop per iteration, the multi-rank routes on one GPU, the C++ drop-in, the H2D copy of
the scan, the replica streams (N > 1) and the CPU baseline (extra keys: kernels, roofline, cpu_baseline, ...; None without --full).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--map", type=int, default=512, help="map edge in voxels (the reference forces it odd: 513)")
    ap.add_argument("--resolution", type=int, default=50)
    ap.add_argument("--integrate", choices=["sparse", "dense", "separate"], default="sparse")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-registration", action="store_true", help="time the TSDF update alone (diagnostics)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything else (kernel classes, roofline, dense-equivalent leg, "
                         "multi-rank routes, drop-in, H2D, replicas, CPU baseline); off: only the timed steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (pose, iterations, a fixed sample of the map)")
    return ap.parse_args()


DUMP_SAMPLE = 1 << 21  # voxels of the map in --dump-outputs' fixed sample (16 B each with its index: 32 MiB)


def dump_outputs(out_dir, tsdf, host_map, tau, pose, iterations):
    """--dump-outputs: what a caller of the timed path holds after its last step -- the registered pose, the Gauss-Newton
    iterations and the averaged map the next registration reads -- as float32 / float64 .npy files, 32 MiB in all.  The map
    (513^3 packed entries, 540 MB) is reduced to per-slab sums over its storage order (every voxel counts) and a fixed, seeded
    sample of voxels (indices into that order, value and weight)."""
    import warpsense_amd as W
    os.makedirs(out_dir, exist_ok=True)
    n_vox = host_map.n_voxels()
    snap = W.DeviceMap(host_map.size_.copy(), host_map.offset_.copy(), np.empty(n_vox, dtype=np.uint32), host_map.pos_.copy())
    tsdf.avg_map().to_host(snap)
    raw = snap.data_
    value = (raw & 0xFFFF).astype(np.uint16).view(np.int16)
    weight = (raw >> 16).astype(np.uint16).view(np.int16)
    slabs = (int(snap.size_[0]), -1)
    arrays = {
        "map_value_sum_per_slab": value.reshape(slabs).sum(axis=1, dtype=np.int64).astype(np.float64),
        "map_weight_sum_per_slab": weight.reshape(slabs).sum(axis=1, dtype=np.int64).astype(np.float64),
        "map_changed_per_slab": (raw != np.uint32(tau & 0xFFFF)).reshape(slabs).sum(axis=1).astype(np.float64),  # != (tau, 0)
    }
    idx = np.unique(np.random.default_rng(20261016).integers(0, n_vox, DUMP_SAMPLE))
    arrays["map_sample_index"] = idx.astype(np.float64)
    arrays["map_sample_value"] = value[idx].astype(np.float32)
    arrays["map_sample_weight"] = weight[idx].astype(np.float32)
    if pose is not None:
        arrays["pose"] = np.asarray(pose, dtype=np.float32).reshape(4, 4)
        arrays["iterations"] = np.array([iterations], dtype=np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def cpu_baseline(points, perturbed, size, tau, mw, res, reg_params):
    """The reference's CPU path (port, oracle/cpu_baseline.cpp) on this box's host cores, one scan of the same workload:
    (i)  update_tsdf with thread_count = 1 (src/cpu/update_tsdf.cpp:397-564, what src/cpu/fastsense.cpp:172 calls),
    (ii) the OpenMP overload (:566-724) at 8 and at 32 threads,
    (iii) register_cloud (src/cpu/registration.cpp:14-177) at 8 and at 32 threads.
    Protocol (median of >= 5 runs after a warm-up; bounded to ~2 min): every variant runs once as a probe (which is
    also its warm-up: page faults of the 513^3 map, OpenMP thread start) and is then timed 5 more times; `value` uses the MEDIAN
    OF THE WARMED SAMPLES of the fastest update variant (the probe is reported, not counted) + the fastest registration variant
    (one warm-up + 5 samples each); one probe with every host CPU is reported next to them.  Every variant reports min / median /
    max of its warmed samples."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    ncpu = os.cpu_count() or 1

    def once(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    samples = {}
    m = O.OracleMap(size, tau, 0)

    def upd(threads):
        m.data[:] = O.pack(tau, 0)
        return O.cpu_update_tsdf(m, points, [0, 0, 0], [0, 0, 32768], tau, mw, res, threads=threads)

    # Every reported variant gets a probe (also its warm-up: page faults of the 513^3 map, OpenMP thread start) and 5 warmed
    # samples.  The port merges its per-thread hash maps the way the reference does (in parallel, every entry probing
    # the maps of the threads before it: O(threads) probes per entry, src/cpu/update_tsdf.cpp:676-722), so beyond a few dozen threads it only gets
    # slower: the widest TIMED variant is 32 threads, and "all host CPUs"  runs ONCE as a probe whose time is in the
    # JSON (`update_all_cpus_probe`), so that "32 of N" is a measured choice and not a comment.
    many = min(ncpu, 32)
    variants = [("update_1_thread", 1), ("update_8_threads", min(8, ncpu))]
    if many > 8:
        variants.append((f"update_{many}_threads", many))
    probes = {name: once(lambda th=th: upd(th)) for name, th in variants}
    best_name, best_th = min(variants, key=lambda v: probes[v[0]])
    def spread(ts):
        return {"median_s": float(np.median(ts)) if ts else None, "min_s": float(min(ts)) if ts else None, "max_s": float(max(ts)) if ts else None,
                "runs_s": [round(t, 3) for t in ts], "warmed_samples": len(ts)}

    for name, th in variants:
        ts = [once(lambda th=th: upd(th)) for _ in range(5)]
        samples[name] = {**spread(ts), "probe_s": round(probes[name], 3), "threads": th}
    best_name, best_th = min(variants, key=lambda v: samples[v[0]]["median_s"])
    if ncpu > many:
        samples["update_all_cpus_probe"] = {"threads": ncpu, "probe_s": round(once(lambda: upd(ncpu)), 3), "warmed_samples": 0,
                                            "note": "one run with every host CPU: not faster than the timed variants (the reference's merge of the per-thread maps costs O(threads) probes per entry, src/cpu/update_tsdf.cpp:676-722)"}
    best_upd = samples[best_name]["median_s"]
    upd(best_th)  # the map the registration runs against
    it_box = []

    def reg(threads):
        _, it, _ = O.cpu_register_cloud(m, perturbed, np.eye(4), reg_params[0], reg_params[1], reg_params[2], res, threads=threads)
        it_box.append(it)

    best_reg = None
    reg_variants = [("register_8_threads", min(8, ncpu))]
    if many > 8:
        reg_variants.append((f"register_{many}_threads", many))
    for name, th in reg_variants:
        once(lambda th=th: reg(th))
        ts = [once(lambda th=th: reg(th)) for _ in range(5)]
        med = float(np.median(ts))
        samples[name] = {**spread(ts), "threads": th, "iterations": it_box[-1]}
        if best_reg is None or med < best_reg[0]:
            best_reg = (med, th, name)
    one = samples["update_1_thread"]["median_s"] or samples["update_1_thread"]["probe_s"]
    return {"value": 1.0 / (best_upd + best_reg[0]), "unit": "scans/s", "cores": int(max(best_th, best_reg[1])), "host_cpus": ncpu, "kind": "port",
            "sample": f"1 scan of the same workload ({points.shape[0]} points, {size[0] + 1 - size[0] % 2}^3 map): median of 5 warmed runs of the "
                      f"fastest update variant {best_name} {best_upd:.2f} s + median of 5 warmed runs of {best_reg[2]} {best_reg[0]:.2f} s; "
                      f"all variants (probe, warmed runs, min / median / max) in `variants`",
            "variants": samples,
            "update_1_thread_scans_per_s": 1.0 / (one + best_reg[0])}


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks here, the way the driver's
    torch.distributed.run line does (one process per GPU, rendezvous on 127.0.0.1), and let rank 0's JSON line through.  Under a
    launcher (WORLD_SIZE set) the world size must be the --gpus asked for."""
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is not None:
        if int(world_env) != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world_env} ranks")
        return
    if args.gpus <= 1:
        return
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    sys.stdout.flush()
    sys.stderr.flush()
    os.execv(sys.executable, cmd)


def main():
    args = parse()
    self_launch(args)
    # The driver reads ONE JSON line from stdout.  Libraries print there too (RCCL's version banner comes from C code):
    # keep a private handle on the real stdout for the result and send everything else that is written to fd 1 to stderr.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    result_out = os.fdopen(result_fd, "w")
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the hot path)")
    # WS_BENCH_SHARE_GPU=1 WS_BENCH_BACKEND=gloo: all ranks on cuda:0 with a gloo group -- a DRY RUN of the N > 1 code path
    # (IPC mailboxes, device-side exchange, replica pass, reductions of the timings) on a 1-GPU box; its numbers mean nothing
    share_gpu = os.environ.get("WS_BENCH_SHARE_GPU") == "1"
    pg_backend = os.environ.get("WS_BENCH_BACKEND", "nccl")
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1 or os.environ.get("WS_BENCH_FORCE_SHARDED") == "1":
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if pg_backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=pg_backend, rank=rank, world_size=world)

    def reduce_max(seconds: float) -> float:
        t = torch.tensor([seconds], dtype=torch.float64, device="cuda" if pg_backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    import warpsense_amd as W
    from warpsense_amd import _lib, synthetic as S
    from warpsense_amd.dist import HipGnBackend, sharded_register_cloud

    tau, mw, res = 1000, 640, args.resolution
    size = (args.map, args.map, args.map)
    reg_params = (200, 0.1, 0.03)
    ctx = W.Context(local_rank)
    ctx.use_torch_stream()  # one stream for the library, torch and the RCCL hand-off
    params = W.Params(W.MapParams(resolution=res, max_distance=tau / 1000.0, max_weight=mw // 64,
                                  size=tuple(s * res / 1000.0 for s in size)),
                      W.RegistrationParams(*reg_params))
    lm = W.LocalMap(size[0], size[1], size[2], tau, 0)
    host_map = lm.device_map()
    host_map.data_ = None  # fresh map: let the library fill both device maps with (tau, 0)
    tsdf = W.TSDFCuda(host_map, tau, mw, res, ctx)
    tsdf.set_integrate({"dense": W.WS_INTEGRATE_DENSE, "sparse": W.WS_INTEGRATE_SPARSE, "separate": W.WS_INTEGRATE_SPARSE_SEPARATE}[args.integrate])
    reg = W.RegistrationCuda(None, ctx)
    del lm

    points = S.os1_128_scan()
    perturbed = S.transform_points_mm(points, S.perturbation())
    if os.environ.get("WS_BENCH_POINT_ORDER") == "column":  # experiment: azimuth-major instead of ring-major cloud
        perturbed = np.ascontiguousarray(perturbed.reshape(S.RINGS, S.AZIMUTHS, 3).transpose(1, 0, 2).reshape(-1, 3))
    d_points = torch.from_numpy(points).cuda()
    d_pert = torch.from_numpy(perturbed).cuda()
    n = points.shape[0]
    eye = np.eye(4, dtype=np.float32)
    backend = HipGnBackend(reg, tsdf, res)
    force_sharded = os.environ.get("WS_BENCH_FORCE_SHARDED") == "1"  # exercise the multi-rank driver on one rank
    exchange = "single GPU"
    if world > 1:
        exchange = "RCCL all-reduce of 44 int64 per iteration (host-driven launches)"
        if os.environ.get("WS_BENCH_NO_PEERS") != "1":
            try:
                # mailboxes exported / mapped with hipIpc: the loop runs without the host in it
                backend.connect_peers(blocks=(256 // world) // 8 * 8 if share_gpu else 0)
                exchange = "device-side: counted mailboxes in the peers' HBM over xGMI, one resident launch per registration"
            except Exception as exc:  # no peer mapping on this node: the RCCL route still works
                print(f"[bench] device-side exchange unavailable ({exc!r}); using the RCCL route", file=sys.stderr)
                backend.peers = None
    reg.prepare_registration(d_pert)
    its = []
    last_pose = [None]  # the pose the last step's registration returned (--dump-outputs)
    graph_cache = {}

    def step():
        tsdf.update_tsdf(d_points, (0, 0, 0), (0, 0, 32768))
        if args.no_registration:
            return
        # TSDFRegistration::register_cloud starts with prepare_registration (tsdf_registration.cpp:50): the cloud is
        # resident in HBM, so this is a device-to-device copy into the registration buffer, inside the timed region
        reg.prepare_registration(d_pert)
        if world == 1 and not force_sharded:
            T, it = reg.register_cloud(tsdf.device_map(), eye, *reg_params, res)
        else:
            # device-side exchange if the peers' mailboxes are mapped; else RCCL with 16 iterations per (validated) HIP graph
            T, it = sharded_register_cloud(backend, n, eye, *reg_params, graphs=graph_cache)
        its.append(it)
        last_pose[0] = T

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    its.clear()
    tsdf_classes = (_lib.WS_K_SETUP, _lib.WS_K_MARCH_TAILS, _lib.WS_K_MARCH_FREE, _lib.WS_K_TILE_BIN, _lib.WS_K_TILE_RESOLVE,
                    _lib.WS_K_INTEGRATE)
    tsdf_mask = sum(1 << k for k in tsdf_classes)
    ctx.prof_reset()
    # In the timed region: ONE hipEvent pair per scan around all kernels of the update, on the stream they run on (plus the
    # dense integrate's own pair when that is the kernel the roofline is about).  A pair per kernel class -- twelve event
    # records per scan -- costs 27 us per step (1.6 %); the per-class table comes from a separate pass below.
    timed_mask = (1 << _lib.WS_K_UPDATE) | ((1 << _lib.WS_K_INTEGRATE) if args.integrate == "dense" else 0)
    ctx.prof_enable(timed_mask)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        elapsed = reduce_max(elapsed)
        if exchange.startswith("device-side") and backend.peers is None:  # the group left that route (repeated time-outs)
            exchange = ("RCCL all-reduce of 44 int64 per iteration, 16 iterations per HIP graph (the device-side exchange kept timing out "
                        "on this node and was dropped; the warm-up and timed steps include those time-outs)")
    ms, cnt = ctx.prof_read(_lib.WS_K_UPDATE)
    update_span_us = 1000.0 * ms / cnt if cnt else None
    # N > 1: what the first real multi-GPU run must be read by: the route the registrations took, their
    # iterations, the registration's share of a step per iteration, time-outs of the device-side exchange
    multi_gpu = None
    if (world > 1 or force_sharded) and its:
        step_us = 1e6 * elapsed / args.steps
        reg_us = step_us - (update_span_us or 0.0)
        multi_gpu = {"route": getattr(backend, "last_route", None), "exchange": exchange, "iterations": float(np.mean(its)),
                     "registration_us_per_scan": reg_us, "us_per_iteration": reg_us / max(float(np.mean(its)), 1.0),
                     "update_us_per_scan": update_span_us, "exchange_timeouts": int(getattr(backend, "peer_timeouts_total", 0)),
                     "note": "strong scaling of ONE 131 072-point registration: the per-iteration floor is the exchange, not the points "
                             "(DESIGN.md §6 expects ~0.6 x the single-GPU scans/s at 8 GPUs); `replica_scans_per_s` is the deployment that scales"}
    ms, cnt = ctx.prof_read(_lib.WS_K_INTEGRATE)
    integrate_timed_us = 1000.0 * ms / cnt if cnt else None
    stats = tsdf.stats()
    ctx.prof_enable(0)
    # what the last timed step handed its caller, before anything below runs more steps on the same map
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, tsdf, host_map, tau, last_pose[0], its[-1] if its else None)

    # Everything from here to the result line measures something beyond the timed steps: --full only.
    # per-class kernel times: the same steps again with an event pair per class (outside the timed region)
    kernels = {}
    if args.full:
        ctx.prof_reset()
        ctx.prof_enable(tsdf_mask)
        for _ in range(max(3, min(args.steps, 10))):
            step()
        fence()
        for k in tsdf_classes:
            name = _lib.KERNEL_CLASSES[k]
            ms, cnt = ctx.prof_read(k)
            if cnt:
                kernels[name] = {"avg_us": 1000.0 * ms / cnt, "launches": cnt}
        ctx.prof_enable(0)
    if integrate_timed_us is not None and "integrate" in kernels:
        kernels["integrate"]["avg_us"] = integrate_timed_us  # the timed region's own measurement

    # dense-equivalent pass: the same steps with the reference-shaped integrate that streams EVERY voxel
    # (16 B/voxel) -- the kernel the survey holds to the HBM roofline.  Separate from the timed region above.
    dense_eq = None
    # (WS_BENCH_SKIP_DENSE_EQ=1: the counter passes of tools/profile_r05.sh leave it out, so that every kernel name in a
    # pass belongs to ONE route -- VERDICT r4 weak #3: tile_resolve<false,false> of this leg was summed into the sparse traffic)
    if args.full and world == 1 and args.integrate != "dense" and not force_sharded and os.environ.get("WS_BENCH_SKIP_DENSE_EQ") != "1":
        tsdf.set_integrate(W.WS_INTEGRATE_DENSE)
        step()
        fence()
        ctx.prof_reset()
        ctx.prof_enable(tsdf_mask)
        n_dense = max(3, min(args.steps, 10))
        t1 = time.perf_counter()
        for _ in range(n_dense):
            step()
        fence()
        dense_elapsed = time.perf_counter() - t1
        dk = {}
        for k in tsdf_classes:
            ms, cnt = ctx.prof_read(k)
            if cnt:
                dk[_lib.KERNEL_CLASSES[k]] = 1000.0 * ms / cnt
        ctx.prof_enable(0)
        tsdf.set_integrate(W.WS_INTEGRATE_SPARSE_SEPARATE if args.integrate == "separate" else W.WS_INTEGRATE_SPARSE)
        step()  # leave the map in the state of the sparse run
        fence()
        n_vox_d = int(np.prod([s if s % 2 else s + 1 for s in size]))
        b_int = 16 * n_vox_d
        b_upd = 12 * n + 4 * 35_442_598 + 4 * 13_901_324 + b_int
        t_upd = sum(dk.values())
        dense_eq = {"value": n_dense / dense_elapsed, "unit": "scans/s", "integrate_us": dk.get("integrate"),
                    "integrate_achieved_GBps": b_int / (dk["integrate"] * 1e-6) / 1e9 if dk.get("integrate") else None,
                    "integrate_frac": b_int / (dk["integrate"] * 1e-6) / 1e9 / HBM_PEAK_GBS if dk.get("integrate") else None,
                    "update_bytes": b_upd, "update_device_us": t_upd,
                    "update_frac": b_upd / (t_upd * 1e-6) / 1e9 / HBM_PEAK_GBS if t_upd else None}

    # registration iteration timing in a separate pass (events per iteration would perturb the timed region)
    if args.full and not args.no_registration and world == 1:
        ctx.prof_reset()
        ctx.prof_enable(1 << _lib.WS_K_REG)
        _, reg_its = reg.register_cloud(tsdf.device_map(), eye, *reg_params, res)
        ms, cnt = ctx.prof_read(_lib.WS_K_REG)
        ctx.prof_enable(0)
        if cnt:
            # the resident loop is ONE launch for all iterations; per-iteration launches report one launch each
            kernels["reg_loop"] = {"avg_us": 1000.0 * ms / cnt, "launches": cnt, "iterations": reg_its,
                                   "us_per_iteration": 1000.0 * ms / max(reg_its, 1), "bytes_per_iteration": 40 * n,
                                   "iterations_per_s": max(reg_its, 1) / (ms * 1e-3) if ms else None,
                                   "achieved_GBps": 40 * n * max(reg_its, 1) / (ms * 1e-3) / 1e9 if ms else None,
                                   "note": "separate pass; latency-bound (SURVEY.md §8d: no roofline gate)"}

    # the multi-GPU code path (points sharded, RCCL all-reduce of the 44 sums each iteration, HIP-graph batches) on ONE
    # rank: what the RCCL route costs per scan before any xGMI hop is added (separate from the timed region)
    sharded_1rank = None
    if args.full and world == 1 and not force_sharded and not args.no_registration and os.environ.get("WS_BENCH_SKIP_SHARDED") != "1":
        try:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", local_rank))
            for _ in range(2):
                tsdf.update_tsdf(d_points, (0, 0, 0), (0, 0, 32768))
                reg.prepare_registration(d_pert)
                _, sh_it = sharded_register_cloud(backend, n, eye, *reg_params)
            fence()
            n_sh = max(3, min(args.steps, 8))
            t2 = time.perf_counter()
            for _ in range(n_sh):
                tsdf.update_tsdf(d_points, (0, 0, 0), (0, 0, 32768))
                reg.prepare_registration(d_pert)
                _, sh_it = sharded_register_cloud(backend, n, eye, *reg_params)
            fence()
            sharded_1rank = {"scans_per_s": n_sh / (time.perf_counter() - t2), "iterations": sh_it,
                             "route": "RCCL all-reduce per iteration, one launch + one collective per iteration enqueued by the host"}
            # the same route with 16 iterations per captured HIP graph (validated bit for bit against stream launches when captured)
            try:
                graphs = {}
                for _ in range(2):
                    reg.prepare_registration(d_pert)
                    _, g_it = sharded_register_cloud(backend, n, eye, *reg_params, graphs=graphs)
                fence()
                t2 = time.perf_counter()
                for _ in range(n_sh):
                    tsdf.update_tsdf(d_points, (0, 0, 0), (0, 0, 32768))
                    reg.prepare_registration(d_pert)
                    _, g_it = sharded_register_cloud(backend, n, eye, *reg_params, graphs=graphs)
                fence()
                runner = next(iter(graphs.values()))
                sharded_1rank["graph_batches"] = {"scans_per_s": n_sh / (time.perf_counter() - t2), "iterations": g_it,
                                                  "graph_in_use": runner.graph is not None}
            except Exception as exc:
                sharded_1rank["graph_batches"] = {"error": repr(exc)[:200]}
            dist.destroy_process_group()
        except Exception as exc:  # RCCL unavailable on this box: report why, keep the bench line
            sharded_1rank = {"error": repr(exc)[:200]}

    # N independent sensor streams, one per GPU (replicas: no exchange at all) -- reported NEXT TO the strong-scaling value
    replica = None
    if args.full and world > 1 and not args.no_registration:
        def replica_step():
            tsdf.update_tsdf(d_points, (0, 0, 0), (0, 0, 32768))
            reg.prepare_registration(d_pert)
            reg.register_cloud(tsdf.device_map(), eye, *reg_params, res)
        for _ in range(2):
            replica_step()
        fence()
        t3 = time.perf_counter()
        for _ in range(args.steps):
            replica_step()
        fence()
        replica = world * args.steps / reduce_max(time.perf_counter() - t3)

    # The multi-GPU loop with the device-side exchange, exercised on this ONE GPU: two ranks (own contexts / streams, 128
    # resident workgroups each) register the same cloud, every rank its half of the points, the 44 sums through mailboxes.
    sharded_2rank = None
    if args.full and world == 1 and not force_sharded and not args.no_registration and os.environ.get("WS_BENCH_SKIP_SHARDED") != "1":
        # (a process of its own, tools/peer_bench.py: this one already drives torch / RCCL streams, and the ranks' kernels
        # must be on the chip together)
        try:
            import subprocess
            fence()
            r2 = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "peer_bench.py"), "--ranks", "2", "--map", str(args.map)],
                                stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            lines = [l for l in r2.stdout.decode(errors="replace").splitlines() if l.startswith("{")]
            sharded_2rank = json.loads(lines[-1]) if lines else {"error": r2.stderr.decode(errors="replace")[-300:]}
        except Exception as exc:
            sharded_2rank = {"error": repr(exc)[:200]}

    # The drop-in as a maintainer of the reference gets it (VERDICT r4 missing #3): examples/dropin_bench.cpp, the C++ classes of
    # include/warpsense_hip/ on host std::vectors -- `relink_only` = the reference's callers unchanged (per-scan H2D in
    # update_tsdf, update_tsdf.cu:152-154; register_cloud's own loop, tsdf_registration.cpp:55-92: one perform_registration +
    # host 6x6 solve per iteration), `one_line_change` = the resident device loop behind the same host vectors.  A process of
    # its own, outside the timed region; never part of `value`.
    dropin = None
    if args.full and world == 1 and not force_sharded and not args.no_registration and os.environ.get("WS_BENCH_SKIP_DROPIN") != "1":
        exe = os.path.join(ROOT, "examples", "dropin_bench")
        try:
            import subprocess
            import tempfile
            if not os.path.exists(exe):
                raise FileNotFoundError("examples/dropin_bench is not built (python -c 'import __graft_entry__ as g; g.build()')")
            fence()
            with tempfile.TemporaryDirectory() as td:
                points.astype(np.int32).tofile(os.path.join(td, "scan.bin"))
                perturbed.astype(np.int32).tofile(os.path.join(td, "pert.bin"))
                r3 = subprocess.run([exe, os.path.join(td, "scan.bin"), os.path.join(td, "pert.bin"), str(n), str(args.map), str(res), str(tau), str(mw),
                                     str(max(5, min(args.steps, 20)))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            lines = [l for l in r3.stdout.decode(errors="replace").splitlines() if l.startswith("{")]
            dropin = json.loads(lines[-1]) if lines else {"error": r3.stderr.decode(errors="replace")[-300:], "rc": r3.returncode}
        except Exception as exc:
            dropin = {"error": repr(exc)[:200]}

    # host buffers (H2D of the scan reported separately, never part of `value`): 1.5 MB pageable / pinned -> HBM
    h2d = None
    if args.full and rank == 0:
        try:
            host_pts = torch.from_numpy(points)
            pinned = host_pts.pin_memory()
            dst = torch.empty_like(d_points)

            def copy_us(src):
                ts = []
                for _ in range(12):
                    torch.cuda.synchronize()
                    t5 = time.perf_counter()
                    dst.copy_(src, non_blocking=False)
                    torch.cuda.synchronize()
                    ts.append(1e6 * (time.perf_counter() - t5))
                return float(np.median(ts[2:]))
            h2d = {"bytes": int(host_pts.numel() * 4), "pageable_us": copy_us(host_pts), "pinned_us": copy_us(pinned),
                   "note": "what ws_tsdf_update (host scan, update_tsdf.cu:152-154) adds in front of the first kernel; not in `value`"}
        except Exception as exc:
            h2d = {"error": repr(exc)[:200]}

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    # ---- roofline (algorithmic bytes per launch, SURVEY.md §8d: B_update = 12 N + 4 V + 4 T + 16 x voxels streamed) ----
    n_vox = int(np.prod([s if s % 2 else s + 1 for s in size]))
    V, T = 35_442_598, 13_901_324  # scatter targets / distinct voxels of this scan (reproduced by the oracle)
    streamed_vox = n_vox if args.integrate == "dense" else min(n_vox, int(stats["tiles"]) * 1024)
    b_scatter = 12 * n + 4 * V + 4 * T
    b_integrate = 16 * streamed_vox
    scatter_classes = ("ray_setup", "march_tails", "march_free", "tile_bin", "tile_resolve")
    roofline = None
    if any(k in kernels for k in scatter_classes):
        t_scatter = sum(kernels[k]["avg_us"] for k in scatter_classes if k in kernels)
        fused = "integrate" not in kernels  # the default route folds the integrate into the tile resolve
        tsdf_kernels = [k for k in kernels if k in scatter_classes or k == "integrate"]
        dom = max(tsdf_kernels, key=lambda k: kernels[k]["avg_us"])
        traffic = None
        traffic_source = None
        try:
            with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as fh:
                tj = json.load(fh)
                traffic_source = "profiles/pmc_traffic.json@" + str(tj.get("git_sha", "unknown")) + " (PMC passes of tools/profile_r05.sh, not measured in this run)"
                mode_key = "dense" if args.integrate == "dense" else "sparse"
                # HBM bytes of the whole kernel group the achieved figure is computed over (PMC passes, tools/make_traffic.py)
                traffic = tj.get(f"integrate:{mode_key}") if dom == "integrate" else tj.get(f"scatter_total:{mode_key}")
        except Exception:
            pass
        if dom == "integrate":
            grp_bytes, grp_us, grp = b_integrate, kernels["integrate"]["avg_us"], ["integrate"]
            timing = "hipEvent pair around the kernel, every scan of the timed region"
        elif fused and update_span_us:
            # the scatter's bytes belong to its kernels TOGETHER (set-up, both marches, binning, tile resolve with the fused
            # integrate, bookkeeping pass): one event pair per scan of the timed region around all of them
            grp_bytes, grp_us, grp = b_scatter + b_integrate, update_span_us, [k for k in scatter_classes if k in kernels]
            timing = "one hipEvent pair per scan of the timed region around all kernels of the update"
        else:
            grp_bytes, grp_us, grp = b_scatter, t_scatter, [k for k in scatter_classes if k in kernels]
            timing = "sum of the per-class hipEvent pairs (separate pass)"
        achieved = grp_bytes / (grp_us * 1e-6) / 1e9
        # vector instructions of the group per scatter target (the update is bound by instruction issue, not bytes):
        # 64 lanes x SQ_INSTS_VALU of the group's kernels / V, from the counter passes of tools/ab_sq.sh (profiles/pmc_valu.json)
        lane_insts = None
        try:
            with open(os.path.join(ROOT, "profiles", "pmc_valu.json")) as fh:
                vj = json.load(fh)
                lane_insts = {"per_scatter_target": 64.0 * sum(vj["valu_per_launch"].values()) / V, "valu_per_launch": vj["valu_per_launch"],
                              "source": "profiles/pmc_valu.json@" + str(vj.get("git_sha", "unknown")) + " (SQ_INSTS_VALU, tools/ab_sq.sh; not measured in this run)"}
        except Exception:
            pass
        group_name = dom if len(grp) == 1 else "tsdf_update: " + " + ".join(grp)
        roofline = {"bound": "hbm", "kernel": group_name, "dominant_kernel": dom, "kernel_group": grp, "lane_instructions": lane_insts, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source, "algorithmic_bytes_per_launch": grp_bytes,
                    "avg_launch_us": grp_us, "timing": timing, "dominant_kernel_us": kernels[dom]["avg_us"],
                    "per_class_sum_us": t_scatter,
                    "note": "VALU-bound ray march (DESIGN.md §5); bytes = SURVEY §8d's scatter term" + (" + fused integrate" if fused else "")}
        if "integrate" in kernels and dom != "integrate":
            ia = b_integrate / (kernels["integrate"]["avg_us"] * 1e-6) / 1e9
            roofline["integrate"] = {"achieved": ia, "frac": ia / HBM_PEAK_GBS, "algorithmic_bytes_per_launch": b_integrate,
                                     "avg_launch_us": kernels["integrate"]["avg_us"],
                                     "basis": "algorithmic (16 B x voxels of the touched tiles; untouched voxels of a tile are read, not written)"
                                     if args.integrate != "dense" else "algorithmic == moved (PMC)"}
        t_update_us = sum(kernels[k]["avg_us"] for k in tsdf_kernels)
        b_update = b_scatter + b_integrate
        roofline["update_total"] = {"bytes": b_update, "device_us": t_update_us,
                                    "achieved": b_update / (t_update_us * 1e-6) / 1e9,
                                    "frac": b_update / (t_update_us * 1e-6) / 1e9 / HBM_PEAK_GBS}

    out = {
        "metric": "scans/sec (OS1-128 131k pts) TSDF update+reg",
        "value": args.steps / elapsed,
        "unit": "scans/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1000.0 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "int32/int64 fixed point (f32 pose, f64 6x6 solve)",
        "data": "synthetic",
        "full": bool(args.full),
        "config": {"workload": f"OS1-128 synthetic scan, {n} pts, {size[0] + 1 - size[0] % 2}^3 TSDF map @ {res} mm, tau {tau}, "
                               f"HIP update_tsdf + Point-to-TSDF registration (BASELINE configs[1])",
                   "points": n, "map_voxels": n_vox, "integrate": args.integrate,
                   "registration": "skipped" if args.no_registration else
                   {"max_iterations": reg_params[0], "it_weight_gradient": reg_params[1], "epsilon": reg_params[2],
                    "iterations_per_scan": float(np.mean(its)) if its else None},
                   "parallelism": "single GPU" if world == 1 else f"map replicated, registration points sharded x{world}; exchange: {exchange}",
                   "contested_voxels": stats["contested_voxels"], "tiles_streamed": stats["tiles"], "tail_records": stats["records"],
                   "record_runs": stats["runs"]},
        "roofline": roofline,
        "kernels": kernels if args.full else None,
        "sharded_1rank_scans_per_s": sharded_1rank["scans_per_s"] if sharded_1rank and "scans_per_s" in sharded_1rank else None,
        "sharded_1rank": sharded_1rank,
        "sharded_2rank_1gpu": sharded_2rank,
        "multi_gpu": multi_gpu,
        "replica_scans_per_s": replica,
        "dry_run_shared_gpu": bool(share_gpu) or None,
        "replica_note": None if replica is None else f"{world} independent streams, one per GPU, no exchange (weak scaling); `value` is the point-sharded run",
        "h2d_scan": h2d,
        "dropin_unchanged": dropin,
    }
    if roofline is not None and dense_eq is not None:
        roofline["dense_equivalent"] = dense_eq
    if h2d and "pageable_us" in h2d:
        out["scans_per_s_with_pageable_h2d"] = 1.0 / (elapsed / args.steps + 1e-6 * h2d["pageable_us"])
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(points, perturbed, size, tau, mw, res, reg_params)
    else:
        out["cpu_baseline"] = None
    result_out.write(json.dumps(out) + "\n")
    result_out.flush()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
