"""ROS-free replay node: the sequencing of warpsense::App (src/warpsense/app.cpp:30-176) over a stream of sensor
clouds, with the whole scan -> pose pipeline on the device.

    app = App(params, "/tmp/map.h5")
    for cloud in clouds:                      # (n, >=3) float32, metres, sensor frame
        app.cloud_callback(cloud)             # preprocess -> update_tsdf (if moved) -> register_cloud -> pose
    app.terminate()                           # write the local map back to the global map file

What ROS provided is passed in explicitly: the IMU pre-transform of `imu_acc_.acc_transform(stamp)` is the optional
`pretransform` argument (identity = no IMU), and the map-shift thread of TSDFMapping::map_shift
(tsdf_mapping.cpp:97-136) runs synchronously after every scan instead of polling a one-slot pose buffer, which makes
a replay deterministic.
"""
from __future__ import annotations

import time

import numpy as np

from .api import (DeviceGlobalMap, GlobalMap, LocalMap, Params, ScanPreprocessor, TSDFRegistration, sweep_poses, to_map)


class App:
    def __init__(self, params: Params, filename: str | None = None, ctx=None, max_points: int = 128 * 1024, async_shift: bool = False, shift: str | None = None,
                 deskew: str | None = None, sweep_bins: int | None = None, reject_dynamic: bool = False):
        # reject_dynamic: the points of a scan that the averaged map holds as FREE at the scan's pose (TSDFMapping.sample: observed
        # free space at least tau in front of any surface -- the sign of a moving object) are dropped on the device before the update
        # and the registration; timings[i]["rejected"] counts them.  An empty map is UNKNOWN everywhere: the first scan drops nothing
        # deskew: None -- every point of a scan is transformed with the one pose of the scan (the reference); "constant-velocity" --
        # one pose per time bin of the sweep (ScanPreprocessor.preprocess_sweep, `sweep_bins` of them, default 1024), the motion
        # during the sweep taken to be the pose change between the last two scans
        # shift: "sync" (TSDFMapping.shift_map), "async" (shift_map_async, what async_shift=True selects) or "device": the global map
        # lives in device memory (DeviceGlobalMap), shifts are device-to-device copies (shift_map_device) and terminate() writes the
        # host global map and its file from the chunks
        # async_shift: TSDFMapping.shift_map_async — the window moves on the device inside the scan that triggers it and
        # the leaving slabs are filed into the global map by a worker thread (same maps and poses as the synchronous route)
        if shift not in (None, "sync", "async", "device"):
            raise ValueError(f"App: shift must be 'sync', 'async' or 'device', not {shift!r}")
        if deskew not in (None, "constant-velocity"):
            raise ValueError(f"App: deskew must be None or 'constant-velocity', not {deskew!r}")
        self.deskew_ = deskew
        self.reject_dynamic_ = bool(reject_dynamic)
        self.sweep_bins_ = 1024 if sweep_bins is None else int(sweep_bins)
        self.async_shift_ = bool(async_shift) if shift is None else shift == "async"
        self.device_shift_ = shift == "device"
        m = params.map
        self.params_ = params
        # app.cpp:33-41: global map (file), local map around the origin, the GPU mapping/registration object
        self.hdf5_global_map_ = GlobalMap(m.tau, m.initial_weight, filename=filename, map_params=m if filename else None)
        self.hdf5_local_map_ = LocalMap(m.size[0], m.size[1], m.size[2], m.tau, m.initial_weight, self.hdf5_global_map_)
        self.device_global_map_ = DeviceGlobalMap(m.tau, m.initial_weight, ctx=ctx) if self.device_shift_ else None
        self.gpu_ = TSDFRegistration(params, self.hdf5_local_map_, ctx, device_global_map=self.device_global_map_)
        self.pre_ = ScanPreprocessor(max_points, ctx)
        if self.async_shift_:
            self.gpu_.reserve_shift(int(np.ceil(m.shift * 1000.0 / m.resolution)))
        self.pose_ = np.eye(4, dtype=np.float32)            # mm
        self.last_tsdf_pose_ = np.eye(4, dtype=np.float32)
        self.last_shift_pose_ = np.eye(4, dtype=np.float32)
        self.initialized_ = False
        self.shifted_ = False
        self.poses = []       # pose_ after every scan
        self.timings = []     # per scan: dict of seconds (the reference's RuntimeEvaluator forms)
        self.n_updates = 0
        self.n_shifts = 0

    def preprocess(self, cloud, sweep_motion=None, sweep=None):
        """App::preprocess (app.cpp:119-148) -> points resident on the device.  With sweep_motion (the sensor's pose at the end of
        the sweep in its frame at the beginning, 4x4, mm) or deskew="constant-velocity": one pose per time bin, the sweep ending at
        the current pose.  sweep: the bin rule, a dict of preprocess_sweep's keywords (columns, ring_major, time_field, t_begin,
        t_end); default by index, ring-major, `sweep_bins` columns."""
        if sweep_motion is None and self.deskew_ == "constant-velocity":
            sweep_motion = self.last_motion()
        if sweep_motion is None:
            return self.pre_.preprocess(cloud, self.pose_, self.params_.map.resolution)
        rule = {"columns": self.sweep_bins_, "ring_major": True} if sweep is None else dict(sweep)
        return self.pre_.preprocess_sweep(cloud, sweep_poses(self.pose_, sweep_motion, self.sweep_bins_), self.params_.map.resolution, **rule)

    def last_motion(self):
        """the pose change between the last two scans, inv(pose[-2]) @ pose[-1] (the identity for the first two scans)"""
        if len(self.poses) < 2:
            return np.eye(4, dtype=np.float32)
        a, b = self.poses[-2].astype(np.float64), self.poses[-1].astype(np.float64)
        m = np.eye(4)
        for i in range(3):  # R_a^T R_b and R_a^T (t_b - t_a), summed in index order (same as include/warpsense_hip/app.hpp)
            for j in range(3):
                m[i, j] = sum(a[k, i] * b[k, j] for k in range(3))
            m[i, 3] = sum(a[k, i] * (b[k, 3] - a[k, 3]) for k in range(3))
        return m.astype(np.float32)

    def update_pose_estimate(self, transform):
        """app.cpp:172-176."""
        T = np.asarray(transform, dtype=np.float32)
        f = np.float32
        R = np.zeros((3, 3), dtype=np.float32)
        for i in range(3):  # float32 products summed in index order (same as include/warpsense_hip/app.hpp)
            for j in range(3):
                acc = f(0)
                for k in range(3):
                    acc = f(acc + f(T[i, k] * self.pose_[k, j]))
                R[i, j] = acc
        self.pose_[:3, :3] = R
        self.pose_[:3, 3] += T[:3, 3]

    def map_shift(self):
        """One turn of TSDFMapping::map_shift (tsdf_mapping.cpp:104-127) for the current pose."""
        d = np.linalg.norm(self.last_shift_pose_[:3, 3] / np.float32(1000) - self.pose_[:3, 3] / np.float32(1000))
        if d >= self.params_.map.shift:
            self.last_shift_pose_ = self.pose_.copy()
            if self.device_shift_:
                self.gpu_.shift_map_device(to_map(self.pose_, self.params_.map.resolution))
            elif self.async_shift_:
                self.gpu_.shift_map_async(to_map(self.pose_, self.params_.map.resolution))
            else:
                self.gpu_.shift_map(to_map(self.pose_, self.params_.map.resolution))
            self.shifted_ = True
            self.n_shifts += 1

    def cloud_callback(self, cloud, pretransform=None, sweep_motion=None, sweep=None):
        """App::cloud_callback (app.cpp:65-117); sweep_motion / sweep: see preprocess."""
        t = {}
        t0 = time.perf_counter()
        scan_points = self.preprocess(cloud, sweep_motion, sweep)
        t["preprocess"] = time.perf_counter() - t0
        if self.reject_dynamic_:
            tr = time.perf_counter()
            # The kept points ALIAS the sample buffer of the mapping until its next sample(): nothing else (scan_consistency from
            # another thread, say) may sample this mapping before the update and the registration below have taken them
            _, counts, _, scan_points = self.gpu_.sample(scan_points, select=("unknown", "surface", "inside"), device=True)
            t["reject"] = time.perf_counter() - tr
            t["rejected"] = int(counts[1])
        distance_tsdf = np.linalg.norm(self.last_tsdf_pose_[:3, 3] / np.float32(1000) - self.pose_[:3, 3] / np.float32(1000))
        if not self.initialized_ or distance_tsdf > 0.3 or self.shifted_:
            self.initialized_ = True
            self.last_tsdf_pose_ = self.pose_.copy()
            t1 = time.perf_counter()
            self.gpu_.update_tsdf(scan_points, pose=self.pose_)
            t["tsdf"] = time.perf_counter() - t1
            self.shifted_ = False
            self.n_updates += 1
        pre = np.eye(4, dtype=np.float32) if pretransform is None else np.asarray(pretransform, dtype=np.float32)
        t2 = time.perf_counter()
        transform = self.gpu_.register_cloud(scan_points, pre)
        t["registration"] = time.perf_counter() - t2
        self.update_pose_estimate(transform)
        if self.hdf5_global_map_.filename() is not None:
            self.hdf5_global_map_.write_pose(self.pose_, 1000.0)
        self.map_shift()
        t["total"] = time.perf_counter() - t0
        t["points"] = len(scan_points)
        t["iterations"] = self.gpu_.last_iterations
        self.poses.append(self.pose_.copy())
        self.timings.append(t)
        return self.pose_

    def terminate(self):
        """App::terminate (app.cpp:192-224): write the map; here straight from the device map."""
        self.gpu_.wait_shift()
        if self.initialized_:
            self.gpu_.write_back()
        self.hdf5_global_map_.close()
