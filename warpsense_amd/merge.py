"""merge_map, map_changes and align_map of TSDFMapping (mapping.py): another global map fused into the one of this run (fuse.py,
ws_store_fuse) or compared with it (changes.py, ws_store_changes), and its pose found by the existing registration."""
from __future__ import annotations

import numpy as np

from ._abi import unpack_entry
from ._lib import WsError
from .global_map import GlobalMap
from .pack import PackQueries
from .store import DeviceGlobalMap


class FuseQueries(PackQueries):
    """merge_map and align_map of TSDFMapping (mapping.py): the fuse behind the mapping's lock and its window; with PackQueries, what
    brings another map in or this one out: save_global_packed, load_global_packed"""

    def merge_map(self, other, T_src_to_dst, max_weight=None, count_only=False, pivot_src_mm=None):
        """Another map fused into everything this run has seen (DeviceGlobalMap.fuse, ws_store_fuse): the window goes into the chunks
        of device_global_map exactly as in global_mesh, `other` is resampled on this map's lattice under T_src_to_dst (4 x 4, mm,
        from the frame of `other` into this map's) and integrated with the weighted average of the TSDF update, and the window is
        loaded back from the chunks, so that it holds the merged voxels and a later save does not undo the merge.  other: a
        DeviceGlobalMap, or a host GlobalMap, which is loaded into a temporary one.  max_weight: None for the map's.  count_only:
        the statistics alone, nothing changes.  Returns FuseStats."""
        m = self.params_.map
        with self._window_in_store("merge_map") as store:
            tmp = None
            if isinstance(other, GlobalMap):
                value, weight = unpack_entry(other.default_raw)
                tmp = DeviceGlobalMap(int(value), int(weight), ctx=store.ctx)
            try:
                if tmp is not None:
                    tmp.load_from(other)
                stats = store.fuse(tmp if tmp is not None else other, T_src_to_dst, m.max_weight if max_weight is None else max_weight,
                                   count_only=count_only, pivot_src_mm=pivot_src_mm, resolution=int(m.resolution))
                if not count_only:
                    lo, hi = self.local_map_.window()
                    store.load_box(self.tsdf_, lo, hi)
                    self._pyramid_touch()  # (the fuse wrote chunks anywhere: global_pyramid rebuilds)
            finally:
                if tmp is not None:
                    tmp.close()
        return stats

    def map_changes(self, ref_store, T_ref_to_cur=None, band=None, free_value=None, min_weight=1, lo=None, hi=None, kinds="both", clusters=False,
                    pivot_ref_mm=None):
        """Where everything this run has seen differs from an earlier map (DeviceGlobalMap.changes, ws_store_changes): the window goes
        into the chunks of device_global_map exactly as in global_mesh, and the store is compared with ref_store, a DeviceGlobalMap
        or a host GlobalMap (loaded into a temporary one), under T_ref_to_cur (4 x 4, mm, from the frame of the earlier map into
        this one's; None: the identity).  band: None for the resolution; free_value: None for tau.  Returns a ChangeResult."""
        m = self.params_.map
        res = int(m.resolution)
        with self._window_in_store("map_changes") as store:
            tmp = None
            if isinstance(ref_store, GlobalMap):
                value, weight = unpack_entry(ref_store.default_raw)
                tmp = DeviceGlobalMap(int(value), int(weight), ctx=store.ctx)
            try:
                if tmp is not None:
                    tmp.load_from(ref_store)
                return store.changes(tmp if tmp is not None else ref_store, T_ref_to_cur, pivot_ref_mm, resolution=res, band=res if band is None else int(band),
                                     free_value=int(self.tsdf_.tau_) if free_value is None else int(free_value), min_weight=min_weight, lo=lo, hi=hi,
                                     kinds=kinds, clusters=clusters)
            finally:
                if tmp is not None:
                    tmp.close()

    def align_map(self, other, T_guess, max_points=65536, band=None):
        """The pose of another map against the window of this one: the surface cloud of `other` (DeviceGlobalMap.surface, records on
        the device, voxels with abs(value) < band, None: one voxel), every k-th record so that at most max_points remain, as voxel
        centres in mm; the points that T_guess (4 x 4, mm, from the frame of `other` into this map's) takes into the present window
        are registered against it by register_cloud from T_guess.  Returns the refined T_src_to_dst (4 x 4 float64), for merge_map
        or a count-only fuse.  Existing calls only: no kernel of its own.  Raises WsError if no point falls into the window."""
        import torch
        if not hasattr(self, "register_cloud"):
            raise WsError("align_map: this mapping has no registration (TSDFRegistration has)")
        m = self.params_.map
        res = int(m.resolution)
        rec = other.surface(self.tsdf_.tau_, res, band=res if band is None else int(band), device=True)
        k = max(1, -(-int(rec.shape[0]) // int(max_points)))
        pts = rec[::k, :3].to(torch.int64) * res + res // 2
        T = np.asarray(T_guess, dtype=np.float64).reshape(4, 4)
        moved = pts.to(torch.float64) @ torch.as_tensor(T[:3, :3].T.copy(), device=pts.device) + torch.as_tensor(T[:3, 3].copy(), device=pts.device)
        lo, hi = self.local_map_.window()
        lo_mm = torch.as_tensor((np.asarray(lo, dtype=np.float64) + 1) * res, device=pts.device)
        hi_mm = torch.as_tensor(np.asarray(hi, dtype=np.float64) * res, device=pts.device)
        keep = ((moved >= lo_mm) & (moved < hi_mm)).all(dim=1)
        cloud = pts[keep].to(torch.int32).contiguous()
        if int(cloud.shape[0]) == 0:
            raise WsError("align_map: no surface point of the other map falls into the window under T_guess")
        self.last_align_points = int(cloud.shape[0])
        torch.cuda.synchronize()  # the cloud was made on torch's stream; the registration copies it on the context's
        return np.asarray(self.register_cloud(cloud, T.astype(np.float32)), dtype=np.float64)
