"""The view-gain queries of TSDFMapping (mapping.py mixes them in): what the sensor would see from candidate poses, over the window and
over everything the run has seen, and the next best view among the frontier clusters the robot can get to."""
from __future__ import annotations

import numpy as np

from ._lib import WsError
from .records import VIEW_GAIN_RECORD, rank_views, view_fan


class GainQueries:
    """TSDFMapping.view_gain, global_view_gain and next_best_view; uses the mapping's params_, mutex_, tsdf_, _window_in_store and
    reachable_frontier."""

    @staticmethod
    def _gain_origins(positions_m, poses):
        """the origins of a view-gain call in map-frame millimetres: `positions_m` ((m, 3) metres) or the translations of `poses`
        ((m, 4, 4), metres), rounded to nearest like the origin of raycast_rays"""
        if (positions_m is None) == (poses is None):
            raise WsError("view_gain: give positions_m or poses, not both and not neither")
        t = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)[:, :3, 3] if positions_m is None else np.asarray(positions_m, dtype=np.float64).reshape(-1, 3)
        return np.rint(t * 1000.0).astype(np.int32)

    @staticmethod
    def _gain_fan(fan):
        return view_fan(16, 64, 45.0) if fan is None else np.ascontiguousarray(fan, dtype=np.int32).reshape(-1, 3)

    def view_gain(self, positions_m=None, poses=None, fan=None, max_range_m=5.0, **kw):
        """The unknown space the sensor would see from candidate positions, in the averaged map (DeviceMapMemWrapper.view_gain on
        avg_map(), under the mapping's lock like a reader).  positions_m: (m, 3) metres in the map frame, or poses: (m, 4, 4) whose
        translations count (the fan is not rotated per view).  fan: (n, 3) int32 directions (None: view_fan(16, 64, 45)).
        Keywords: lo, hi, min_value, any_weight, rays, device.  Returns the records, or (records, rays)."""
        origins = self._gain_origins(positions_m, poses)
        with self.mutex_:
            avg = self.tsdf_.avg_map()
            out = avg.view_gain(origins, self._gain_fan(fan), int(np.rint(float(max_range_m) * 1000.0)), **kw)
            self.last_view_gain = avg.last_view_gain
            return out

    def global_view_gain(self, positions_m=None, poses=None, fan=None, max_range_m=5.0, **kw):
        """view_gain() through everything the run has seen: the window goes into the chunks of device_global_map exactly as in
        global_mesh, then DeviceGlobalMap.view_gain at the map's resolution (the box None: the bounding box of the chunks)."""
        if self.device_global_map_ is None:
            raise WsError("global_view_gain: this TSDFMapping has no device_global_map")
        origins = self._gain_origins(positions_m, poses)
        with self._window_in_store("global_view_gain") as store:
            out = store.view_gain(int(self.params_.map.resolution), origins, self._gain_fan(fan), int(np.rint(float(max_range_m) * 1000.0)), **kw)
            self.last_view_gain = store.last_view_gain
            return out

    def next_best_view(self, pose=None, clearance_m=0.0, fan=None, max_range_m=5.0, min_size=1, lam_per_m=0.0, min_value=0, unknown_free=False, seed_mm=None):
        """Where to go next: reachable_frontier from `pose` (or from seed_mm, as there: the voxel of the sensor itself is never observed, a
        robot seeds the free space it stands in), the voxel centres of the goals of the reachable clusters with at least
        min_size voxels as origins of one view_gain call, and rank_views of the records against the path costs.
        Returns a dict: `table`, `cost`, `goal` (of reachable_frontier, all clusters), `candidates` (the table indices that were
        evaluated), `records` (VIEW_GAIN_RECORD per candidate), `order` and `score` (rank_views over the candidates), `winner` (its
        table index, -1 without a candidate), and `header`, `path` (reach_paths of the winner's goal, goal first; None without)."""
        res = int(self.params_.map.resolution)
        with self.mutex_:
            rf = self.reachable_frontier(seed_mm=seed_mm, pose=pose, clearance_m=clearance_m, min_value=min_value, unknown_free=unknown_free)
            cand = np.asarray([i for i in rf["reachable"] if int(rf["table"]["count"][i]) >= int(min_size)], dtype=np.int64)
            out = dict(table=rf["table"], cost=rf["cost"], goal=rf["goal"], candidates=cand, records=np.zeros(0, dtype=VIEW_GAIN_RECORD),
                       order=np.zeros(0, np.int64), score=np.zeros(0), winner=-1, header=None, path=None)
            if len(cand) == 0:
                return out
            centres = rf["goal"][cand].astype(np.int64) * res + res // 2
            avg = self.tsdf_.avg_map()
            rec = avg.view_gain(centres.astype(np.int32), self._gain_fan(fan), int(np.rint(float(max_range_m) * 1000.0)), min_value=min_value)
            self.last_view_gain = avg.last_view_gain
            order, score = rank_views(rec, rf["cost"][cand], res, lam_per_m)
            win = int(cand[order[0]])
            hdr, _ = avg.reach_paths(rf["goal"][win:win + 1], 0)
            hdr, path = avg.reach_paths(rf["goal"][win:win + 1], int(hdr["steps"][0]) + 1)
            out.update(records=rec, order=order, score=score, winner=win, header=hdr[0], path=path[0, :int(hdr["written"][0])])
            return out
