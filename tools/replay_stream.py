"""Replay a synthetic OS1-128 stream through warpsense_amd.App (BASELINE.json configs[2]: 10 Hz stream, 1024^3
sliding TSDF map @ 5 cm, one MI355X): sensor clouds in float metres -> device pre-processing -> TSDF update
(when the sensor moved > 0.3 m) -> Point-to-TSDF registration -> pose -> map shift (device-side slabs).

    python tools/replay_stream.py --map 1024 --scans 30 [--h5 /tmp/stream.h5] [--async-shift | --device-global-map] [--surface-ply DIR [--surface-every N]] [--mesh-ply DIR] [--global-packed FILE.wspk]
                                   [--raycast-ply DIR] [--distance-npy DIR [--distance-m M]] [--global-distance-npy FILE [--global-distance-m M]]
                                   [--moving-sweeps] [--deskew] [--frontier-ply DIR] [--global-frontier-ply FILE] [--reach-ply DIR [--reach-clearance-m M]]
                                   [--ground-npy DIR [--ground-height-m M]] [--rollouts-csv FILE [--rollouts-radius-m M]]

Prints one JSON line: scans/s over the stream and the mean per-stage times (the reference's RuntimeEvaluator
forms "preprocess", "tsdf", "registration", "total")."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def relocalize_after_kidnap(app, cloud, args, true_position_mm):
    """The tracked pose is lost: put a wrong one in its place, register the scan (in the sensor frame) from every pose of the lattice
    around it in one launch, take the best, report, and hand the recovered pose back to the tracker."""
    import warpsense_amd as W
    a = np.deg2rad(args.kidnap_yaw)
    wrong = app.pose_.astype(np.float64)
    wrong[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ wrong[:3, :3]
    wrong[0, 3] += 1000.0 * args.kidnap_offset[0]
    wrong[1, 3] += 1000.0 * args.kidnap_offset[1]
    app.pose_ = wrong.astype(np.float32)
    pts = app.pre_.preprocess(cloud, np.eye(4, dtype=np.float32), app.params_.map.resolution)  # the scan where the sensor is the origin
    t0 = time.perf_counter()
    radius, step, yaw_range, yaw_step = args.kidnap_lattice
    pose, best, table = app.gpu_.relocalize(pts, app.pose_, radius, step, yaw_range, yaw_step)
    dt = time.perf_counter() - t0
    app.pose_ = pose.astype(np.float32)
    out = {"scan": args.kidnap, "candidates": int(len(table["e"])), "chosen": int(best), "seconds": dt,
           "chosen_start_error_mm": float(np.linalg.norm(table["start"][best][:3, 3] - true_position_mm)),
           "wrong_pose_error_mm": float(np.linalg.norm(wrong[:3, 3] - true_position_mm)),
           "recovered_pose_error_mm": float(np.linalg.norm(pose[:3, 3] - true_position_mm)),
           "recovered_yaw_error_deg": float(np.rad2deg(np.arctan2(pose[1, 0], pose[0, 0]))),
           "iterations": int(table["iterations"][best]), "mean_error": float(table["e"][best]) / max(int(table["c"][best]), 1)}
    print(f"kidnap at scan {args.kidnap}: candidate {best} of {out['candidates']} in {1000.0 * dt:.1f} ms, "
          f"{out['recovered_pose_error_mm']:.1f} mm / {out['recovered_yaw_error_deg']:.2f} deg from the true pose "
          f"(the wrong pose: {out['wrong_pose_error_mm']:.1f} mm / {args.kidnap_yaw:.2f} deg)", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=1024)
    ap.add_argument("--res", type=int, default=50)
    ap.add_argument("--scans", type=int, default=30)
    ap.add_argument("--step", type=float, default=0.25, help="sensor motion per scan in metres (along x, half of it along y)")
    ap.add_argument("--shift", type=float, default=5.0, help="map shift distance in metres (map/shift)")
    ap.add_argument("--room", type=float, nargs=3, default=(22.0, 16.0, 2.5), help="half extents of the room in metres")
    ap.add_argument("--h5", default=None)
    ap.add_argument("--hz", type=float, default=0.0, help="pace the stream: scan k is handed over no earlier than k/hz seconds after the first "
                    "(0 = back to back; the sensor of configs[2] delivers 10 Hz, and the slab filing of an asynchronous shift "
                    "has the time between two shifts of a paced stream to finish)")
    ap.add_argument("--async-shift", action="store_true", help="map shift off the scan path (TSDFMapping.shift_map_async)")
    ap.add_argument("--device-global-map", action="store_true", help="the global map in device memory (DeviceGlobalMap): shifts are device-to-device "
                    "copies (TSDFMapping.shift_map_device), the host map and its file are written from the chunks at the end")
    ap.add_argument("--surface-ply", default=None, metavar="DIR", help="write the marker cloud of the window (publish_local_map, selected on the "
                    "device: TSDFMapping.surface_cloud) as binary little-endian PLY (xyz + rgb) into DIR")
    ap.add_argument("--mesh-ply", default=None, metavar="DIR", help="write a triangle mesh of the window (surface nets on the device: "
                    "TSDFMapping.surface_mesh) as binary little-endian PLY into DIR, after every N-th scan like --surface-ply")
    ap.add_argument("--global-mesh-ply", default=None, metavar="FILE", help="after the last scan: the mesh of the WHOLE run, window and every chunk that "
                    "has left it, from the device global map (TSDFMapping.global_mesh, ws_store_mesh); needs --device-global-map")
    ap.add_argument("--global-packed", default=None, metavar="FILE", help="after the last scan: the WHOLE run, window and every chunk that has left it, as a "
                    "packed snapshot (.wspk; TSDFMapping.save_global_packed, ws_store_pack); needs --device-global-map")
    ap.add_argument("--global-mesh-level", type=int, default=0, metavar="L", help="the level of detail of --global-mesh-ply: 0 the map's resolution, L the "
                    "store coarsened L times (voxels of 2^L times the edge; TSDFMapping.global_pyramid, ws_store_coarsen)")
    ap.add_argument("--global-surface-ply", default=None, metavar="FILE", help="after the last scan: the surface cloud of the WHOLE run, window and every "
                    "chunk that has left it, from the device global map (TSDFMapping.global_surface_cloud, ws_store_surface) as PLY; needs "
                    "--device-global-map")
    ap.add_argument("--frontier-ply", default=None, metavar="DIR", help="after every TSDF update: the clustered frontier of the window (TSDFMapping.frontier, "
                    "ws_map_frontier) as binary little-endian PLY (xyz + mask + cluster) into DIR")
    ap.add_argument("--reach-ply", default=None, metavar="DIR", help="after every TSDF update: the paths from the sensor to the reachable frontier clusters of the "
                    "window (TSDFMapping.reachable_frontier: ws_map_distance, ws_map_reach, ws_map_frontier, ws_map_reach_lookup_dev, ws_map_reach_paths) as "
                    "binary little-endian PLY (vertices with path number and cost, edges) into DIR")
    ap.add_argument("--reach-clearance-m", type=float, default=0.2, metavar="M", help="... that keep M metres from the obstacles")
    ap.add_argument("--ground-npy", default=None, metavar="DIR", help="after every TSDF update: the ground layer of the window (TSDFMapping.ground, ws_map_ground) "
                    "into DIR as ground_height_NNNNN.npy (millimetres, float64, NaN without a level) and ground_class_NNNNN.npy (uint8: 0 unknown, 1 ground, 2 blocked, "
                    "3 void), shaped (nx, ny) like the window")
    ap.add_argument("--ground-height-m", type=float, default=1.0, metavar="M", help="... under M metres of headroom (at most 64 voxels)")
    ap.add_argument("--next-view-csv", default=None, metavar="FILE", help="after every TSDF update: the next best view among the reachable frontier clusters of the "
                    "window (TSDFMapping.next_best_view: reachable_frontier, ws_map_view_gain, rank_views) as one line of FILE: scan number, the winner's goal "
                    "voxel x y z, its path cost, its unknown_k2, the number of candidates (-1 -1 -1, 4294967295 and 0 without a candidate); the "
                    "clearance is --reach-clearance-m")
    ap.add_argument("--next-view-range-m", type=float, default=5.0, metavar="M", help="... with rays of M metres")
    ap.add_argument("--rollouts-csv", default=None, metavar="FILE", help="after every TSDF update: the best of a fan of constant-curvature rollouts from the current "
                    "pose over the window's column distance (arc_rollouts, TSDFMapping.score_trajectories, ws_map_clearance) as one line of FILE: scan number, "
                    "the best trajectory (-1 without one), its speed and yaw rate, its cost and smallest margin in mm, the trajectories with a hit, the fan's size")
    ap.add_argument("--rollouts-radius-m", type=float, default=0.3, metavar="M", help="... for a body of one sphere of M metres, with as much again as soft range")
    ap.add_argument("--global-frontier-ply", default=None, metavar="FILE", help="after the last scan: the clustered frontier of the WHOLE run from the device "
                    "global map (TSDFMapping.global_frontier, ws_store_frontier) as PLY; needs --device-global-map")
    ap.add_argument("--global-raycast-ply", default=None, metavar="FILE", help="after the last scan: the predicted scan from the pose of the FIRST scan, "
                    "which the window has left, through the device global map (TSDFMapping.global_raycast, ws_store_raycast) as PLY, and its hit "
                    "share printed next to that of the window's raycast from the same pose; needs --device-global-map")
    ap.add_argument("--raycast-ply", default=None, metavar="DIR", help="after every registered scan: the ray cast of the map from the registered pose "
                    "(TSDFMapping.raycast, the OS1-128 pattern, hits with normals) as binary little-endian PLY into DIR, and the median absolute "
                    "scan_residual of the scan printed")
    ap.add_argument("--distance-npy", default=None, metavar="DIR", help="after every TSDF update: the 2-D cost map of the window (TSDFMapping.distance_field, "
                    "columns=True: per (x, y) column the squared distance in voxels to the nearest column with an occupied voxel, and its class) as "
                    "a uint32 .npy into DIR")
    ap.add_argument("--distance-m", type=float, default=2.0, metavar="M", help="... clamped at M metres")
    ap.add_argument("--global-distance-npy", default=None, metavar="FILE", help="after the last scan: the 2-D cost map of the WHOLE run (TSDFMapping."
                    "global_distance_field, ws_store_distance, columns=True) over the x, y bounding box of the chunks of the device global map and the "
                    "z range of the window, the band of --distance-npy, as a uint32 .npy; needs --device-global-map")
    ap.add_argument("--global-distance-m", type=float, default=2.0, metavar="M", help="... clamped at M metres")
    ap.add_argument("--surface-every", type=int, default=10, metavar="N", help="... after every N-th scan")
    ap.add_argument("--kidnap", type=int, default=0, metavar="N", help="at scan N (1-based) replace the tracked pose by a wrong one (--kidnap-offset, "
                    "--kidnap-yaw), re-localise with TSDFRegistration.relocalize on a pose lattice around it (one launch for all candidates), "
                    "print the chosen candidate and its distance to the stream's true pose, and go on tracking from it")
    ap.add_argument("--kidnap-offset", type=float, nargs=2, default=(0.8, -0.4), metavar=("DX", "DY"), help="... offset of the wrong pose in metres")
    ap.add_argument("--kidnap-yaw", type=float, default=20.0, metavar="DEG", help="... and its yaw error")
    ap.add_argument("--kidnap-lattice", type=float, nargs=4, default=(1.2, 0.4, 30.0, 10.0), metavar=("RADIUS_M", "STEP_M", "YAW_RANGE", "YAW_STEP"))
    ap.add_argument("--moving-sweeps", action="store_true", help="the sensor moves WHILE it turns: scan k is a sweep taken between the true poses of "
                    "scan k - 1 and scan k (synthetic.os1_128_sweep; the first one stands), instead of a snapshot from the pose of scan k")
    ap.add_argument("--deskew", action="store_true", help="App(deskew='constant-velocity'): one pose per firing column, the motion during a sweep "
                    "taken from the last two registered poses")
    ap.add_argument("--reject-dynamic", action="store_true", help="App(reject_dynamic=True): the points of a scan that the map holds as observed free "
                    "space are dropped on the device before the update and the registration; prints the number dropped per scan")
    args = ap.parse_args()
    if args.global_mesh_ply and not args.device_global_map:
        ap.error("--global-mesh-ply requires --device-global-map")
    if args.global_packed and not args.device_global_map:
        ap.error("--global-packed requires --device-global-map")
    if args.global_mesh_level < 0 or (args.global_mesh_level and not args.global_mesh_ply):
        ap.error("--global-mesh-level is a level >= 0 and requires --global-mesh-ply")
    if args.global_surface_ply and not args.device_global_map:
        ap.error("--global-surface-ply requires --device-global-map")
    if args.global_frontier_ply and not args.device_global_map:
        ap.error("--global-frontier-ply requires --device-global-map")
    if args.global_raycast_ply and not args.device_global_map:
        ap.error("--global-raycast-ply requires --device-global-map")
    if args.global_distance_npy and not args.device_global_map:
        ap.error("--global-distance-npy requires --device-global-map")
    import warpsense_amd as W
    from warpsense_amd import synthetic as S

    size_m = args.map * args.res / 1000.0
    params = W.Params(W.MapParams(resolution=args.res, max_distance=1.0, max_weight=10, size=(size_m, size_m, size_m), shift=args.shift),
                      W.RegistrationParams(200, 0.1, 0.03))
    t0 = time.perf_counter()
    app = W.App(params, args.h5, async_shift=args.async_shift, shift="device" if args.device_global_map else None,
                deskew="constant-velocity" if args.deskew else None, reject_dynamic=args.reject_dynamic)
    t_setup = time.perf_counter() - t0
    he = tuple(1000.0 * r for r in args.room)
    clouds = []
    for k in range(args.scans):
        sensor = np.array([1000.0 * args.step * k, 500.0 * args.step * k, 0.0])
        if args.moving_sweeps:
            T0, T1 = np.eye(4), np.eye(4)
            T0[:3, 3] = (1000.0 * args.step * max(k - 1, 0), 500.0 * args.step * max(k - 1, 0), 0.0)
            T1[:3, 3] = sensor
            clouds.append(S.os1_128_sweep(T0, T1, half_extents_mm=he, seed=1000 + k))
            continue
        pts = S.os1_128_scan(sensor_mm=tuple(sensor), half_extents_mm=he, seed=1000 + k)
        clouds.append(((pts.astype(np.float64) - sensor) / 1000.0).astype(np.float32))
    W.pause()
    t1 = time.perf_counter()
    busy = 0.0
    surface = {"files": 0, "points": 0, "seconds": 0.0}
    mesh = {"files": 0, "vertices": 0, "faces": 0, "seconds": 0.0}
    if args.surface_ply:
        os.makedirs(args.surface_ply, exist_ok=True)
    frontier = {"files": 0, "records": 0, "clusters": 0, "seconds": 0.0}
    if args.frontier_ply:
        os.makedirs(args.frontier_ply, exist_ok=True)
    reach = {"files": 0, "clusters": 0, "reachable": 0, "rounds": 0, "seconds": 0.0}
    if args.reach_ply:
        os.makedirs(args.reach_ply, exist_ok=True)
    ground = {"files": 0, "ground": 0, "blocked": 0, "void": 0, "seconds": 0.0}
    if args.ground_npy:
        os.makedirs(args.ground_npy, exist_ok=True)
    next_view = {"lines": 0, "candidates": 0, "seconds": 0.0}
    next_view_file = None
    if args.next_view_csv:
        next_view_file = open(args.next_view_csv, "w")
        next_view_file.write("scan,goal_x,goal_y,goal_z,path_cost,unknown_k2,candidates\n")
    rollouts = {"lines": 0, "trajectories": 0, "with_a_best": 0, "seconds": 0.0}
    rollouts_file = None
    if args.rollouts_csv:
        rollouts_file = open(args.rollouts_csv, "w")
        rollouts_file.write("scan,best,speed_mps,yaw_rate_rps,cost,min_margin_mm,hit_trajectories,trajectories\n")
        fan_speeds, fan_rates = np.linspace(0.25, 1.5, 6), np.linspace(-0.8, 0.8, 17)
        fan_body = W.body_spheres([[0.0, 0.0, 0.0]], args.rollouts_radius_m)
    updates_seen = 0
    if args.mesh_ply:
        os.makedirs(args.mesh_ply, exist_ok=True)
    raycast = {"files": 0, "hits": 0, "median_abs_residual_mm": [], "seconds": 0.0}
    if args.raycast_ply:
        os.makedirs(args.raycast_ply, exist_ok=True)
    distance = {"files": 0, "site_columns": 0, "seconds": 0.0}
    if args.distance_npy:
        os.makedirs(args.distance_npy, exist_ok=True)
    updates_seen = app.n_updates
    kidnap = None
    for k, c in enumerate(clouds):
        if args.hz > 0.0:
            wait = t1 + k / args.hz - time.perf_counter()
            if wait > 0.0:
                time.sleep(wait)
        tb = time.perf_counter()
        if args.kidnap and k + 1 == args.kidnap:
            kidnap = relocalize_after_kidnap(app, c, args, np.array([1000.0 * args.step * k, 500.0 * args.step * k, 0.0]))
        app.cloud_callback(c)
        busy += time.perf_counter() - tb
        if args.frontier_ply and app.n_updates > updates_seen:  # after every update of the map
            ts = time.perf_counter()
            rec, labels, table = app.gpu_.frontier(clusters=True)
            frontier["records"] = W.write_frontier_ply(os.path.join(args.frontier_ply, f"frontier_{k + 1:05d}.ply"), rec, args.res, labels)
            frontier["clusters"] = int(len(table))
            frontier["files"] += 1
            frontier["seconds"] += time.perf_counter() - ts
        if args.reach_ply and app.n_updates > updates_seen:  # after every update of the map: where the robot can go from where it is
            ts = time.perf_counter()
            pose_m = app.pose_.astype(np.float64).copy()
            pose_m[:3, 3] /= 1000.0  # (the app keeps millimetres)
            got = app.gpu_.reachable_frontier(pose=pose_m, clearance_m=args.reach_clearance_m, cap_steps=4096)
            if got["headers"] is not None:
                W.write_path_ply(os.path.join(args.reach_ply, f"reach_{k + 1:05d}.ply"), got["headers"], got["paths"], args.res)
                reach["files"] += 1
            reach["clusters"], reach["reachable"], reach["rounds"] = int(len(got["table"])), int(len(got["reachable"])), int(app.gpu_.last_reach["rounds"])
            reach["seconds"] += time.perf_counter() - ts
        if args.ground_npy and app.n_updates > updates_seen:  # after every update of the map: where the robot can stand
            ts = time.perf_counter()
            g = app.gpu_.ground(robot_height_m=args.ground_height_m)
            np.save(os.path.join(args.ground_npy, f"ground_height_{k + 1:05d}.npy"), g.height_mm(args.res))
            np.save(os.path.join(args.ground_npy, f"ground_class_{k + 1:05d}.npy"), g.cls)
            ground["ground"], ground["blocked"], ground["void"] = int(g.counts[1]), int(g.counts[2]), int(g.counts[3])
            ground["files"] += 1
            ground["seconds"] += time.perf_counter() - ts
        if next_view_file is not None and app.n_updates > updates_seen:  # after every update of the map: where to look next
            ts = time.perf_counter()
            pose_m = app.pose_.astype(np.float64).copy()
            pose_m[:3, 3] /= 1000.0  # (the app keeps millimetres)
            nbv = app.gpu_.next_best_view(pose=pose_m, clearance_m=args.reach_clearance_m, max_range_m=args.next_view_range_m)
            win = nbv["winner"]
            goal = nbv["goal"][win] if win >= 0 else (-1, -1, -1)
            cost = int(nbv["cost"][win]) if win >= 0 else 0xFFFFFFFF
            gain = int(nbv["records"]["unknown_k2"][nbv["order"][0]]) if win >= 0 else 0
            next_view_file.write(f"{k + 1},{int(goal[0])},{int(goal[1])},{int(goal[2])},{cost},{gain},{len(nbv['candidates'])}\n")
            next_view["lines"] += 1
            next_view["candidates"] = int(len(nbv["candidates"]))
            next_view["seconds"] += time.perf_counter() - ts
        if rollouts_file is not None and app.n_updates > updates_seen:  # after every update of the map: which way to drive
            ts = time.perf_counter()
            pose_m = app.pose_.astype(np.float64).copy()
            pose_m[:3, 3] /= 1000.0  # (the app keeps millimetres)
            fan = W.arc_rollouts(pose_m, fan_speeds, fan_rates, steps=20, dt=0.2)
            sc = app.gpu_.score_trajectories(fan, fan_body, soft_m=args.rollouts_radius_m)
            b = sc.best
            speed, rate = (fan_speeds[b // len(fan_rates)], fan_rates[b % len(fan_rates)]) if b >= 0 else (0.0, 0.0)
            cost, margin = (int(sc.records["cost"][b]), int(sc.records["min_margin"][b])) if b >= 0 else (0, 0)
            rollouts_file.write(f"{k + 1},{b},{speed:.3f},{rate:.3f},{cost},{margin},{int(np.count_nonzero(sc.records['hits']))},{len(fan)}\n")
            rollouts["lines"] += 1
            rollouts["trajectories"] = int(len(fan))
            rollouts["with_a_best"] += int(b >= 0)
            rollouts["seconds"] += time.perf_counter() - ts
        updates_seen = app.n_updates
        if args.surface_ply and (k + 1) % max(args.surface_every, 1) == 0:
            ts = time.perf_counter()
            _, marker = app.gpu_.surface_cloud(marker=True)
            surface["points"] = W.write_surface_ply(os.path.join(args.surface_ply, f"surface_{k + 1:05d}.ply"), marker)
            surface["files"] += 1
            surface["seconds"] += time.perf_counter() - ts
        if args.mesh_ply and (k + 1) % max(args.surface_every, 1) == 0:
            ts = time.perf_counter()
            mesh["vertices"], mesh["faces"] = W.write_mesh_ply(os.path.join(args.mesh_ply, f"mesh_{k + 1:05d}.ply"), *app.gpu_.surface_mesh())
            mesh["files"] += 1
            mesh["seconds"] += time.perf_counter() - ts
        if args.distance_npy and app.n_updates != updates_seen:
            updates_seen = app.n_updates
            ts = time.perf_counter()
            np.save(os.path.join(args.distance_npy, f"costmap_{k + 1:05d}.npy"), app.gpu_.distance_field(max_dist_m=args.distance_m, columns=True))
            distance["site_columns"] = app.gpu_.tsdf().avg_map().last_sites
            distance["files"] += 1
            distance["seconds"] += time.perf_counter() - ts
        if args.raycast_ply:
            ts = time.perf_counter()
            pose_m = app.pose_.astype(np.float64)
            pose_m[:3, 3] /= 1000.0  # (the app keeps its translation in millimetres)
            raycast["hits"] = W.write_raycast_ply(os.path.join(args.raycast_ply, f"raycast_{k + 1:05d}.ply"), *app.gpu_.raycast(pose_m, gradient=True))
            resid = app.gpu_.scan_residual(app.preprocess(c), pose_m)  # the scan at the registered pose, where it lies on the device
            med = float(np.nanmedian(np.abs(resid))) if np.any(~np.isnan(resid)) else None
            print(f"scan {k + 1}: raycast hits {raycast['hits']}, median |scan residual| {med} mm", file=sys.stderr)
            raycast["median_abs_residual_mm"].append(med)
            raycast["files"] += 1
            raycast["seconds"] += time.perf_counter() - ts
    W.pause()
    t2 = time.perf_counter()
    global_mesh = None
    if args.global_mesh_ply:
        tg = time.perf_counter()
        gv, gf = app.gpu_.global_mesh(level=args.global_mesh_level)
        tg = time.perf_counter() - tg
        os.makedirs(os.path.dirname(os.path.abspath(args.global_mesh_ply)), exist_ok=True)
        W.write_mesh_ply(args.global_mesh_ply, gv, gf)
        global_mesh = {"file": args.global_mesh_ply, "vertices": int(len(gv)), "faces": int(len(gf)), "chunks": app.gpu_.device_global_map_.count(), "call_s": tg,
                       "level": args.global_mesh_level}
        route = "save_box + ws_store_mesh + download" if not args.global_mesh_level else "save_box + ws_store_coarsen per level + ws_store_mesh + download"
        print(f"global mesh (level {args.global_mesh_level}): {len(gv)} vertices, {len(gf)} faces from {global_mesh['chunks']} chunks in {1000.0 * tg:.2f} ms ({route})",
              file=sys.stderr)
    global_packed = None
    if args.global_packed:
        tg = time.perf_counter()
        os.makedirs(os.path.dirname(os.path.abspath(args.global_packed)), exist_ok=True)
        gp = app.gpu_.save_global_packed(args.global_packed)
        tg = time.perf_counter() - tg
        global_packed = {"file": args.global_packed, "chunks": gp.n_chunks, "bricks_default_uniform_dense": list(gp.stats[:3]), "bytes": int(gp.stats[3]),
                         "ratio": gp.ratio, "call_s": tg}
        print(f"global packed: {gp.n_chunks} chunks, {gp.stats[3] / 1e6:.1f} MB, ratio {gp.ratio:.4f} in {1000.0 * tg:.2f} ms (save_box + ws_store_pack + download + file)",
              file=sys.stderr)
    global_surface = None
    if args.global_surface_ply:
        tg = time.perf_counter()
        _, gm = app.gpu_.global_surface_cloud(marker=True)
        tg = time.perf_counter() - tg
        os.makedirs(os.path.dirname(os.path.abspath(args.global_surface_ply)), exist_ok=True)
        points = W.write_surface_ply(args.global_surface_ply, gm)
        global_surface = {"file": args.global_surface_ply, "points": int(points), "chunks": app.gpu_.device_global_map_.count(), "call_s": tg}
        print(f"global surface: {points} points from {global_surface['chunks']} chunks in {1000.0 * tg:.2f} ms (save_box + ws_store_surface + download)",
              file=sys.stderr)
    global_frontier = None
    if args.global_frontier_ply:
        tg = time.perf_counter()
        rec, labels, table = app.gpu_.global_frontier(clusters=True)
        tg = time.perf_counter() - tg
        os.makedirs(os.path.dirname(os.path.abspath(args.global_frontier_ply)), exist_ok=True)
        W.write_frontier_ply(args.global_frontier_ply, rec, args.res, labels)
        goals = W.frontier_goals(table, args.res, min_size=10)
        global_frontier = {"file": args.global_frontier_ply, "records": int(len(rec)), "clusters": int(len(table)), "clusters_of_10_or_more": int(len(goals[1])),
                           "chunks": app.gpu_.device_global_map_.count(), "call_s": tg}
        print(f"global frontier: {len(rec)} records in {len(table)} clusters from {global_frontier['chunks']} chunks in {1000.0 * tg:.2f} ms "
              "(save_box + ws_store_frontier + download)", file=sys.stderr)
    global_distance = None
    if args.global_distance_npy:
        tg = time.perf_counter()
        store = app.gpu_.device_global_map_
        wlo, whi = app.hdf5_local_map_.window()
        keys = np.asarray(store.keys() + [tuple(int(v) // 64 for v in wlo), tuple(int(v) // 64 for v in whi)], dtype=np.int64)
        lo = (int(keys[:, 0].min()) * 64, int(keys[:, 1].min()) * 64, int(wlo[2]))
        hi = (int(keys[:, 0].max()) * 64 + 63, int(keys[:, 1].max()) * 64 + 63, int(whi[2]))
        cost = app.gpu_.global_distance_field(lo=lo, hi=hi, max_dist_m=args.global_distance_m, columns=True)
        tg = time.perf_counter() - tg
        os.makedirs(os.path.dirname(os.path.abspath(args.global_distance_npy)), exist_ok=True)
        np.save(args.global_distance_npy, cost)
        global_distance = {"file": args.global_distance_npy, "lo": lo, "hi": hi, "columns": [int(v) for v in cost.shape], "site_columns": int(store.last_sites),
                           "chunks": store.count(), "call_s": tg}
        print(f"global cost map: {cost.shape[0]} x {cost.shape[1]} columns, {store.last_sites} site columns from {global_distance['chunks']} chunks in "
              f"{1000.0 * tg:.2f} ms (save_box + ws_store_distance + download)", file=sys.stderr)
    global_raycast = None
    if args.global_raycast_ply:
        first = app.poses[0].astype(np.float64).copy()
        first[:3, 3] /= 1000.0  # (the app keeps its translation in millimetres)
        tg = time.perf_counter()
        rec, grad = app.gpu_.global_raycast(first, gradient=True)
        tg = time.perf_counter() - tg
        rng = app.gpu_._global_range_mm(np.rint(first[:3, 3] * 1000.0))
        rec_w, _ = app.gpu_.raycast(first, max_range_mm=rng)
        os.makedirs(os.path.dirname(os.path.abspath(args.global_raycast_ply)), exist_ok=True)
        hits = W.write_raycast_ply(args.global_raycast_ply, rec, grad)
        share, share_w = hits / len(rec), float(np.count_nonzero(rec_w["range_mm"] >= 0)) / len(rec_w)
        global_raycast = {"file": args.global_raycast_ply, "rays": int(len(rec)), "hit_share": share, "window_hit_share": share_w, "range_mm": rng,
                          "chunks": app.gpu_.device_global_map_.count(), "call_s": tg}
        print(f"global raycast from the first pose: hit share {share:.3f} (the window's raycast from the same pose: {share_w:.3f}), "
              f"{global_raycast['chunks']} chunks, {1000.0 * tg:.2f} ms (save_box + ws_store_raycast + download)", file=sys.stderr)
    if args.reject_dynamic:
        for k, t in enumerate(app.timings):
            print(f"scan {k + 1}: rejected {t['rejected']} of {t['points'] + t['rejected']} points in {1000.0 * t['reject']:.2f} ms", file=sys.stderr)
    stages = {}
    for key in ("preprocess", "tsdf", "registration", "total"):
        vals = [t[key] for t in app.timings if key in t]
        stages[key + "_ms"] = 1000.0 * float(np.mean(vals)) if vals else None
    true_last = np.array([1000.0 * args.step * (args.scans - 1), 500.0 * args.step * (args.scans - 1), 0.0])
    if next_view_file is not None:
        next_view_file.close()
    if rollouts_file is not None:
        rollouts_file.close()
    t3 = time.perf_counter()
    app.terminate()
    t4 = time.perf_counter()
    print(f"final position error against the ground truth: {float(np.linalg.norm(app.poses[-1][:3, 3] - true_last)):.1f} mm", file=sys.stderr)
    print(json.dumps({"workload": f"{args.scans} synthetic OS1-128 scans (131072 pts), {args.map}^3 sliding map @ {args.res} mm, App replay",
                      "args": {"step_m": args.step, "shift_m": args.shift, "room_m": list(args.room), "h5": bool(args.h5), "hz": args.hz, "moving_sweeps": bool(args.moving_sweeps),
                               "deskew": bool(args.deskew)},
                      "scans_per_s": args.scans / (t2 - t1), "stream_s": t2 - t1, "callback_busy_s": busy, "setup_s": t_setup, **stages,
                      "tsdf_updates": app.n_updates, "map_shifts": app.n_shifts, "async_shift": bool(args.async_shift), "device_global_map": bool(args.device_global_map),
                      "slowest_scan_ms": 1000.0 * float(max(t["total"] for t in app.timings[2:])),
                      "scans_over_100ms": int(sum(1 for t in app.timings[2:] if t["total"] > 0.1)),
                      "points_after_preprocess": float(np.mean([t["points"] for t in app.timings])),
                      "iterations_mean": float(np.mean([t["iterations"] for t in app.timings])),
                      "final_position_error_mm": float(np.linalg.norm(app.poses[-1][:3, 3] - true_last)),
                      "terminate_write_back_s": t4 - t3, "h5": args.h5,
                      "surface_ply": surface if args.surface_ply else None,
                      "mesh_ply": mesh if args.mesh_ply else None,
                      "global_mesh_ply": global_mesh,
                      "global_surface_ply": global_surface,
                      "global_packed": global_packed,
                      "frontier_ply": frontier if args.frontier_ply else None,
                      "reach_ply": reach if args.reach_ply else None,
                      "ground_npy": ground if args.ground_npy else None,
                      "next_view_csv": next_view if args.next_view_csv else None,
                      "rollouts_csv": rollouts if args.rollouts_csv else None,
                      "global_frontier_ply": global_frontier,
                      "global_raycast_ply": global_raycast,
                      "global_distance_npy": global_distance,
                      "raycast_ply": raycast if args.raycast_ply else None,
                      "distance_npy": distance if args.distance_npy else None,
                      "kidnap": kidnap}))


if __name__ == "__main__":
    main()
