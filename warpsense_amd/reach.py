"""The reach queries of TSDFMapping (mapping.py mixes them in): distance call with a fitting range, then the reach; and the frontier
clusters the robot can get to."""
from __future__ import annotations

import numpy as np

from ._lib import WsError
from .records import FRONTIER_CLUSTER, REACH_UNREACHABLE


class ReachQueries:
    """TSDFMapping.reach, global_reach and reachable_frontier; uses the mapping's params_, mutex_, tsdf_, device_global_map_,
    _max_dist_vox and _window_in_store."""

    def _reach_seeds(self, seed_mm, pose):
        """the seed voxels of a reach: `seed_mm` ((n, 3) map-frame millimetres) or the translation of `pose` (4 x 4, metres), floor-divided
        by the resolution like every point of the map"""
        if (seed_mm is None) == (pose is None):
            raise WsError("reach: give seed_mm or pose, not both and not neither")
        mm = np.rint(np.asarray(pose, dtype=np.float64).reshape(4, 4)[:3, 3] * 1000.0) if seed_mm is None else np.asarray(seed_mm, dtype=np.float64)
        return np.floor_divide(mm.reshape(-1, 3).astype(np.int64), int(self.params_.map.resolution)).astype(np.int32)

    def _clearance(self, clearance_m):
        """(max_dist_vox of the distance call, clear_d2) for a clearance in metres: whole voxels by the rule of distance_field, and a
        field that reaches one voxel further, so that the clamp never hides a voxel that keeps the clearance"""
        vox = max(self._max_dist_vox(clearance_m), 0)
        if vox > 254:
            raise WsError("reach: the clearance must stay below 255 voxels")
        return vox + 1, vox * vox

    def reach(self, seed_mm=None, pose=None, clearance_m=0.0, lo=None, hi=None, unknown_free=False, unknown_occupied=False, columns=False, max_rounds=0,
              device=False):
        """How far every voxel of the box (None: the window) is from the robot along free space that keeps `clearance_m` from the
        obstacles: the distance call with a fitting range, then DeviceMapMemWrapper.reach on avg_map(), under the mapping's lock like a
        reader.  The seeds are seed_mm ((n, 3) map-frame millimetres) or the translation of `pose`.  Returns the uint32 costs shaped
        like the box ((nx, ny) with columns); reach_mm(cost, resolution) gives millimetres; last_reach keeps seeded, reached, rounds."""
        seeds = self._reach_seeds(seed_mm, pose)
        vox, clear_d2 = self._clearance(clearance_m)
        with self.mutex_:
            avg = self.tsdf_.avg_map()
            avg.distance(lo=lo, hi=hi, max_dist_vox=vox, unknown_occupied=unknown_occupied, columns=columns, device=True)
            cost = avg.reach(seeds, clear_d2=clear_d2, unknown_free=unknown_free, max_rounds=max_rounds, device=device)
            self.last_reach = avg.last_reach
            return cost

    def global_reach(self, seed_mm=None, pose=None, clearance_m=0.0, lo=None, hi=None, unknown_free=False, unknown_occupied=False, columns=False,
                     max_rounds=0, device=False):
        """reach() over everything the run has seen: the window goes into the chunks of device_global_map exactly as in global_mesh, then
        DeviceGlobalMap.distance and DeviceGlobalMap.reach (the box None: the bounding box of the chunks)."""
        if self.device_global_map_ is None:
            raise WsError("global_reach: this TSDFMapping has no device_global_map")
        seeds = self._reach_seeds(seed_mm, pose)
        vox, clear_d2 = self._clearance(clearance_m)
        with self._window_in_store("global_reach") as store:
            store.distance(lo=lo, hi=hi, max_dist_vox=vox, unknown_occupied=unknown_occupied, columns=columns, device=True)
            cost = store.reach(seeds, clear_d2=clear_d2, unknown_free=unknown_free, max_rounds=max_rounds, device=device)
            self.last_reach = store.last_reach
            return cost

    def reachable_frontier(self, seed_mm=None, pose=None, clearance_m=0.0, min_value=0, unknown_free=False, cap_steps=0, max_rounds=0):
        """Which frontier clusters of the window the robot can get to, and how: the clustered frontier, the reach from the seeds, the
        costs at ALL frontier records by reach_lookup on the records as they lie in device memory, then on the host (the table is
        small) per cluster its cheapest reached member, and with cap_steps > 0 the paths to those members.
        Returns a dict: `table` (FRONTIER_CLUSTER rows), `cost` (uint32 per cluster, 0xFFFFFFFF: no member can be reached), `goal`
        ((k, 3) int32 world voxels of the cheapest members; of the first member where none is reached), `headers` and `paths`
        (reach_paths of the goals of the reachable clusters, in table order; None without cap_steps) and `reachable` (their indices)."""
        seeds = self._reach_seeds(seed_mm, pose)
        vox, clear_d2 = self._clearance(clearance_m)
        with self.mutex_:
            avg = self.tsdf_.avg_map()
            avg.distance(max_dist_vox=vox, device=True)
            avg.reach(seeds, clear_d2=clear_d2, unknown_free=unknown_free, max_rounds=max_rounds, device=True)
            self.last_reach = avg.last_reach
            rec_dev, labels_dev, table_dev = avg.frontier(min_value=min_value, clusters=True, device=True)
            cost = avg.reach_lookup(rec_dev).cpu().numpy().view(np.uint32)  # one cost per record, made on the device
            rec, labels = rec_dev.cpu().numpy(), labels_dev.cpu().numpy().view(np.uint32)
            table = np.ascontiguousarray(table_dev.cpu().numpy()).view(FRONTIER_CLUSTER).reshape(-1)
            k = len(table)
            best = np.full(k, REACH_UNREACHABLE, dtype=np.uint32)
            np.minimum.at(best, labels, cost)
            # the cheapest member of a cluster; among equals the first in record order
            order = np.lexsort((np.arange(len(cost)), cost, labels))
            first_of = order[np.searchsorted(labels[order], np.arange(k))] if k else np.zeros(0, np.int64)
            goal = rec[first_of, :3].astype(np.int32).reshape(-1, 3)
            reachable = np.flatnonzero(best != np.uint32(REACH_UNREACHABLE))
            headers = paths = None
            if cap_steps and len(reachable):
                headers, paths = avg.reach_paths(goal[reachable], cap_steps)
            return dict(table=table, cost=best, goal=goal, reachable=reachable, headers=headers, paths=paths)
