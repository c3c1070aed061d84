"""ctypes binding of libwarpsense_hip.so — the C ABI declared in include/warpsense_hip.h.

There is NO CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# WS_HIP_LIB: another build of the same library (A/B measurements of kernel variants on one box; tools/ab_bench.sh)
LIB_PATH = os.environ.get("WS_HIP_LIB") or os.path.join(PKG_DIR, "libwarpsense_hip.so")

WS_MAP_AVG, WS_MAP_NEW = 0, 1
WS_INTEGRATE_SPARSE, WS_INTEGRATE_DENSE, WS_INTEGRATE_SPARSE_SEPARATE = 0, 1, 2
WS_REG_ALL_POINTS, WS_REG_COMPAT_REFERENCE_LAUNCH = 0, 1
WS_REG_LOOP_RESIDENT, WS_REG_LOOP_LAUNCHES = 0, 1
(WS_K_SETUP, WS_K_MARCH_TAILS, WS_K_MARCH_FREE, WS_K_TILE_BIN, WS_K_TILE_RESOLVE, WS_K_INTEGRATE, WS_K_REG, WS_K_UPDATE) = range(8)
KERNEL_CLASSES = ["ray_setup", "march_tails", "march_free", "tile_bin", "tile_resolve", "integrate", "reg_iteration", "tsdf_update"]

# every symbol include/warpsense_hip.h declares (tests check the library exports all of them)
EXPORTS = [
    "ws_last_error", "ws_version", "ws_ctx_create", "ws_ctx_destroy", "ws_ctx_set_stream", "ws_sync",
    "ws_device_reset", "ws_map_create", "ws_map_destroy", "ws_map_upload", "ws_map_set_params", "ws_map_download",
    "ws_map_extract_box", "ws_map_insert_box", "ws_shift_plan", "ws_shift_begin", "ws_shift_reserve", "ws_shift_count", "ws_shift_entering", "ws_shift_wait", "ws_shift_slab",
    "ws_shift_end", "ws_map_get_params", "ws_map_device_data", "ws_map_n_voxels", "ws_tsdf_update", "ws_tsdf_update_dev", "ws_tsdf_scatter_dev",
    "ws_tsdf_integrate", "ws_tsdf_set_integrate", "ws_tsdf_set_capacity", "ws_debug_tsdf_chunk_policy", "ws_tsdf_stats", "ws_reg_create", "ws_reg_destroy", "ws_reg_prepare",
    "ws_reg_prepare_dev", "ws_reg_points_dev", "ws_reg_iterate", "ws_register_cloud", "ws_reg_begin", "ws_reg_accumulate_dev",
    "ws_reg_solve_dev", "ws_reg_iterate_shard_dev", "ws_reg_poll", "ws_reg_peer_mailbox", "ws_reg_peer_connect", "ws_reg_peer_connect_local",
    "ws_reg_peer_disconnect", "ws_reg_peer_reset", "ws_register_cloud_peers", "ws_reg_set_loop", "ws_debug_solve6", "ws_debug_reg_stall", "ws_debug_reg_server", "ws_debug_reg_mail_selftest", "ws_debug_reg_sums", "ws_debug_block_stats", "ws_scan_create", "ws_scan_destroy", "ws_scan_preprocess",
    "ws_scan_preprocess_dev", "ws_scan_points_dev", "ws_scan_download", "ws_scan_preprocess_sweep", "ws_scan_preprocess_sweep_dev", "ws_sweep_poses", "ws_prof_enable", "ws_prof_read", "ws_prof_reset",
    "ws_map_surface", "ws_map_surface_records_dev", "ws_map_surface_marker_dev", "ws_map_surface_download", "ws_debug_surface_timing",
    "ws_map_mesh", "ws_map_mesh_vertices_dev", "ws_map_mesh_faces_dev", "ws_map_mesh_download", "ws_debug_mesh_timing",
    "ws_map_raycast", "ws_map_raycast_dev", "ws_map_raycast_records_dev", "ws_map_raycast_gradient_dev", "ws_map_raycast_download", "ws_debug_raycast_timing",
    "ws_map_distance", "ws_map_distance_dev", "ws_map_distance_download", "ws_debug_distance_timing",
    "ws_register_cloud_batch", "ws_reg_batch_best",
    "ws_store_create", "ws_store_destroy", "ws_store_reserve", "ws_store_count", "ws_store_keys", "ws_store_has", "ws_store_get_chunk", "ws_store_put_chunk",
    "ws_store_drop_chunk", "ws_store_chunk_dev", "ws_store_save_box", "ws_store_load_box", "ws_shift_device", "ws_store_chunks_of_box", "ws_debug_store_timing",
    "ws_store_distance", "ws_store_distance_dev", "ws_store_distance_download", "ws_debug_store_distance_timing",
    "ws_store_surface", "ws_store_surface_records_dev", "ws_store_surface_marker_dev", "ws_store_surface_download", "ws_debug_store_surface_timing",
    "ws_store_mesh", "ws_store_mesh_vertices_dev", "ws_store_mesh_faces_dev", "ws_store_mesh_download", "ws_debug_store_mesh_timing",
    "ws_map_sample", "ws_map_sample_dev", "ws_map_sample_records_dev", "ws_map_sample_gradient_dev", "ws_map_sample_selected_dev", "ws_map_sample_download",
    "ws_debug_sample_timing",
    "ws_store_sample", "ws_store_sample_dev", "ws_store_sample_records_dev", "ws_store_sample_gradient_dev", "ws_store_sample_selected_dev",
    "ws_store_sample_download", "ws_debug_store_sample_timing",
    "ws_store_raycast", "ws_store_raycast_dev", "ws_store_raycast_records_dev", "ws_store_raycast_gradient_dev", "ws_store_raycast_download",
    "ws_debug_store_raycast_timing", "ws_debug_store_raycast_table", "ws_debug_store_raycast_find",
    "ws_map_frontier", "ws_map_frontier_records_dev", "ws_map_frontier_labels_dev", "ws_map_frontier_clusters_dev", "ws_map_frontier_download",
    "ws_debug_frontier_timing",
    "ws_store_frontier", "ws_store_frontier_records_dev", "ws_store_frontier_labels_dev", "ws_store_frontier_clusters_dev", "ws_store_frontier_download",
    "ws_debug_store_frontier_timing",
    "ws_map_reach", "ws_map_reach_dev", "ws_map_reach_download", "ws_map_reach_box", "ws_store_reach_box", "ws_map_reach_lookup", "ws_map_reach_lookup_dev", "ws_map_reach_paths", "ws_debug_reach_timing",
    "ws_debug_reach_params", "ws_debug_reach_active",
    "ws_store_reach", "ws_store_reach_dev", "ws_store_reach_download", "ws_store_reach_lookup", "ws_store_reach_lookup_dev", "ws_store_reach_paths",
    "ws_debug_store_reach_timing",
    "ws_map_view_gain", "ws_map_view_gain_records_dev", "ws_map_view_gain_rays_dev", "ws_map_view_gain_download", "ws_debug_view_gain_timing",
    "ws_store_view_gain", "ws_store_view_gain_records_dev", "ws_store_view_gain_rays_dev", "ws_store_view_gain_download", "ws_debug_store_view_gain_timing",
    "ws_map_clearance", "ws_map_clearance_dev", "ws_map_clearance_records_dev", "ws_map_clearance_poses_dev", "ws_map_clearance_download", "ws_debug_clearance_timing",
    "ws_store_clearance", "ws_store_clearance_dev", "ws_store_clearance_records_dev", "ws_store_clearance_poses_dev", "ws_store_clearance_download",
    "ws_debug_store_clearance_timing", "ws_clearance_centres", "ws_clearance_margin",
    "ws_store_fuse", "ws_debug_store_fuse_timing",
    "ws_store_coarsen", "ws_store_parents_of", "ws_debug_store_coarsen_timing",
    "ws_store_changes", "ws_store_changes_records_dev", "ws_store_changes_labels_dev", "ws_store_changes_clusters_dev", "ws_store_changes_download",
    "ws_debug_store_changes_timing",
    "ws_map_ground", "ws_map_ground_dev", "ws_map_ground_download", "ws_map_ground_box", "ws_debug_ground_timing", "ws_map_ground_distance",
    "ws_store_ground", "ws_store_ground_dev", "ws_store_ground_download", "ws_store_ground_box", "ws_debug_store_ground_timing", "ws_store_ground_distance",
    "ws_store_pack", "ws_store_pack_headers_dev", "ws_store_pack_payload_dev", "ws_store_pack_download", "ws_store_unpack", "ws_store_unpack_dev",
    "ws_pack_check", "ws_pack_expand_chunk", "ws_pack_chunk", "ws_debug_store_pack_timing",
]
WS_SURFACE_RECORDS, WS_SURFACE_MARKER = 0, 1
WS_MESH_DEFAULT, WS_MESH_ANY_WEIGHT = 0, 1
WS_RAYCAST_DEFAULT, WS_RAYCAST_ANY_WEIGHT, WS_RAYCAST_GRADIENT, WS_RAYCAST_TARGETS = 0, 1, 2, 4
WS_SAMPLE_DEFAULT, WS_SAMPLE_ANY_WEIGHT, WS_SAMPLE_GRADIENT = 0, 1, 2
WS_SAMPLE_SELECT_UNKNOWN, WS_SAMPLE_SELECT_FREE, WS_SAMPLE_SELECT_SURFACE, WS_SAMPLE_SELECT_INSIDE = 4, 8, 16, 32
SAMPLE_CLASSES = ("unknown", "free", "surface", "inside")  # class c of a sample record; WS_SAMPLE_SELECT_* is 4 << c
WS_DISTANCE_DEFAULT, WS_DISTANCE_ANY_WEIGHT, WS_DISTANCE_UNKNOWN_OCCUPIED, WS_DISTANCE_COLUMNS = 0, 1, 2, 4
WS_GROUND_DEFAULT, WS_GROUND_ANY_WEIGHT, WS_GROUND_UNKNOWN_HEADROOM, WS_GROUND_TOP = 0, 1, 2, 4
GROUND_CLASSES = ("unknown", "ground", "blocked", "void")  # class c of a ground record
WS_FRONTIER_DEFAULT, WS_FRONTIER_ANY_WEIGHT, WS_FRONTIER_CLUSTERS = 0, 1, 2
WS_REACH_DEFAULT, WS_REACH_UNKNOWN_FREE, WS_REACH_UNREACHABLE = 0, 1, 0xFFFFFFFF
WS_GAIN_DEFAULT, WS_GAIN_ANY_WEIGHT, WS_GAIN_RAYS = 0, 1, 2
WS_CLEARANCE_DEFAULT, WS_CLEARANCE_POSES, WS_CLEARANCE_OUTSIDE_OK = 0, 1, 2
WS_FUSE_DEFAULT, WS_FUSE_COUNT_ONLY = 0, 1
WS_COARSEN_DEFAULT = 0
WS_CHANGES_APPEARED, WS_CHANGES_VANISHED, WS_CHANGES_CLUSTERS, WS_CHANGES_DEFAULT = 1, 2, 4, 3
WS_PACK_HEADER_WORDS, WS_PACK_DEFAULT, WS_PACK_EMIT_DIRECT = 40, 0, 1


class WsError(RuntimeError):
    pass


H5_LIB_PATH = os.path.join(PKG_DIR, "libwarpsense_h5.so")
H5_EXPORTS = ["ws_h5_last_error", "ws_h5_create", "ws_h5_open", "ws_h5_close", "ws_h5_flush", "ws_h5_write_meta", "ws_h5_read_meta",
              "ws_h5_write_chunk", "ws_h5_read_chunk", "ws_h5_num_chunks", "ws_h5_list_chunks", "ws_h5_write_pose", "ws_h5_num_poses",
              "ws_h5_read_pose"]
_h5 = None


def h5_available() -> bool:
    return os.path.exists(H5_LIB_PATH)


def load_h5() -> C.CDLL:
    """Load libwarpsense_h5.so (include/warpsense_h5.h); raises if it was not built (no HDF5 C library on the box)."""
    global _h5
    if _h5 is not None:
        return _h5
    if not os.path.exists(H5_LIB_PATH):
        raise WsError(f"{H5_LIB_PATH} is missing: `python -m warpsense_amd.build` builds it where the HDF5 C library is installed")
    L = C.CDLL(H5_LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    P = C.POINTER
    L.ws_h5_last_error.restype = C.c_char_p
    L.ws_h5_create.argtypes = [C.c_char_p, P(vp)]
    L.ws_h5_open.argtypes = [C.c_char_p, C.c_int, P(vp)]
    L.ws_h5_close.argtypes = [vp]
    L.ws_h5_flush.argtypes = [vp]
    L.ws_h5_write_meta.argtypes = [vp, i32, vp, C.c_float, i32, i32]
    L.ws_h5_read_meta.argtypes = [vp, P(i32), vp, P(C.c_float), P(i32), P(i32)]
    L.ws_h5_write_chunk.argtypes = [vp, i32, i32, i32, vp]
    L.ws_h5_read_chunk.argtypes = [vp, i32, i32, i32, vp, P(i32)]
    L.ws_h5_num_chunks.argtypes = [vp, P(i64)]
    L.ws_h5_list_chunks.argtypes = [vp, vp, i64, P(i64)]
    L.ws_h5_write_pose.argtypes = [vp, vp]
    L.ws_h5_num_poses.argtypes = [vp, P(i64)]
    L.ws_h5_read_pose.argtypes = [vp, i64, vp]
    _h5 = L
    return L


def check_h5(rc: int, what: str):
    if rc != 0:
        raise WsError(f"{what}: {load_h5().ws_h5_last_error().decode(errors='replace')}")


class TsdfStats(C.Structure):
    _fields_ = [("contested_voxels", C.c_int64), ("records", C.c_int64), ("tiles", C.c_int64),
                ("error_flags", C.c_int32), ("hash_entries", C.c_int32), ("runs", C.c_int64), ("free_space_hits", C.c_int64),
                ("record_slots", C.c_int64), ("record_capacity", C.c_int64)]


class ShiftPlan(C.Structure):
    """ws_shift_plan_t: the steps of a map shift and their boxes"""
    _fields_ = [("n", C.c_int32), ("axis", C.c_int32 * 3), ("d", C.c_int32 * 3),
                ("leave_lo", C.c_int32 * 3 * 3), ("leave_hi", C.c_int32 * 3 * 3), ("enter_lo", C.c_int32 * 3 * 3), ("enter_hi", C.c_int32 * 3 * 3),
                ("pos", C.c_int32 * 3), ("offset", C.c_int32 * 3)]


class Sweep(C.Structure):
    """ws_sweep_t: the rule that gives every point of a sweep its time bin"""
    _fields_ = [("columns", C.c_uint32), ("ring_major", C.c_int32), ("time_field", C.c_int32), ("t_begin", C.c_float), ("t_end", C.c_float)]


WS_SWEEP_MAX_BINS = 4096
_lib = None


def load() -> C.CDLL:
    """Load the HIP library; raises if it has not been built (python -m warpsense_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WsError(f"{LIB_PATH} is missing: build it with `python -m warpsense_amd.build` "
                      "(there is no CPU fallback for the hot path)")
    # PyTorch-ROCm ships its own libamdhip64; two HIP runtimes in one process do not share the device (whichever
    # initialises second reports "no ROCm-capable device").  Load torch's first, so that this library binds to it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, sz, i64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t, C.c_int64
    P = C.POINTER
    L.ws_last_error.restype = C.c_char_p
    L.ws_version.restype = C.c_int
    L.ws_ctx_create.argtypes = [C.c_int, P(vp)]
    L.ws_ctx_destroy.argtypes = [vp]
    L.ws_ctx_set_stream.argtypes = [vp, vp]
    L.ws_sync.argtypes = [vp]
    L.ws_map_create.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, P(vp)]
    L.ws_map_destroy.argtypes = [vp]
    L.ws_map_upload.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.ws_map_set_params.argtypes = [vp, C.c_int, vp, vp, vp]
    L.ws_map_download.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.ws_map_extract_box.argtypes = [vp, C.c_int, vp, vp, vp]
    L.ws_map_insert_box.argtypes = [vp, C.c_int, vp, vp, vp]
    L.ws_map_get_params.argtypes = [vp, C.c_int, vp, vp, vp]
    L.ws_map_surface.argtypes = [vp, C.c_int, vp, vp, i32, u32, P(sz)]
    L.ws_map_surface_records_dev.argtypes = [vp, P(sz)]
    L.ws_map_surface_records_dev.restype = vp
    L.ws_map_surface_marker_dev.argtypes = [vp, P(sz)]
    L.ws_map_surface_marker_dev.restype = vp
    L.ws_map_surface_download.argtypes = [vp, vp, vp, sz, P(sz)]
    L.ws_debug_surface_timing.argtypes = [vp, i32, vp]
    L.ws_map_mesh.argtypes = [vp, C.c_int, vp, vp, u32, P(sz), P(sz)]
    L.ws_map_mesh_vertices_dev.argtypes = [vp, P(sz)]
    L.ws_map_mesh_vertices_dev.restype = vp
    L.ws_map_mesh_faces_dev.argtypes = [vp, P(sz)]
    L.ws_map_mesh_faces_dev.restype = vp
    L.ws_map_mesh_download.argtypes = [vp, vp, vp, sz, sz, P(sz), P(sz)]
    L.ws_debug_mesh_timing.argtypes = [vp, i32, vp]
    L.ws_map_raycast.argtypes = [vp, C.c_int, vp, vp, sz, i32, u32, P(sz)]
    L.ws_map_raycast_dev.argtypes = [vp, C.c_int, vp, vp, sz, i32, u32, P(sz)]
    L.ws_map_raycast_records_dev.argtypes = [vp, P(sz)]
    L.ws_map_raycast_records_dev.restype = vp
    L.ws_map_raycast_gradient_dev.argtypes = [vp, P(sz)]
    L.ws_map_raycast_gradient_dev.restype = vp
    L.ws_map_raycast_download.argtypes = [vp, vp, vp, sz, P(sz)]
    L.ws_debug_raycast_timing.argtypes = [vp, i32, vp]
    L.ws_map_sample.argtypes = [vp, C.c_int, vp, sz, i32, u32, vp]
    L.ws_map_sample_dev.argtypes = [vp, C.c_int, vp, sz, i32, u32, vp]
    L.ws_store_sample.argtypes = [vp, vp, vp, vp, sz, i32, i32, u32, vp]
    L.ws_store_sample_dev.argtypes = [vp, vp, vp, vp, sz, i32, i32, u32, vp]
    for owner in ("map", "store"):
        for part in ("records", "gradient", "selected"):
            f = getattr(L, f"ws_{owner}_sample_{part}_dev")
            f.argtypes, f.restype = [vp, P(sz)], vp
        getattr(L, f"ws_{owner}_sample_download").argtypes = [vp, vp, vp, vp, sz, sz, P(sz), P(sz)]
    L.ws_debug_sample_timing.argtypes = [vp, i32, vp]
    L.ws_debug_store_sample_timing.argtypes = [vp, i32, vp]
    L.ws_map_distance.argtypes = [vp, C.c_int, vp, vp, i32, u32, P(sz)]
    L.ws_map_distance_dev.argtypes = [vp, P(sz)]
    L.ws_map_distance_dev.restype = vp
    L.ws_map_distance_download.argtypes = [vp, vp, sz, P(sz)]
    L.ws_debug_distance_timing.argtypes = [vp, i32, vp]
    L.ws_map_ground.argtypes = [vp, C.c_int, vp, vp, i32, u32, vp]
    L.ws_map_ground_dev.argtypes = [vp, P(sz)]
    L.ws_map_ground_dev.restype = vp
    L.ws_map_ground_download.argtypes = [vp, vp, sz, P(sz)]
    L.ws_map_ground_box.argtypes = [vp, vp, vp]
    L.ws_debug_ground_timing.argtypes = [vp, i32, vp]
    L.ws_map_ground_distance.argtypes = [vp, i32, i32, u32, P(sz)]
    L.ws_map_frontier.argtypes = [vp, C.c_int, vp, vp, i32, u32, P(sz), P(sz)]
    L.ws_store_frontier.argtypes = [vp, vp, vp, i32, u32, P(sz), P(sz)]
    for owner in ("map", "store"):
        for part in ("records", "labels", "clusters"):
            f = getattr(L, f"ws_{owner}_frontier_{part}_dev")
            f.argtypes, f.restype = [vp, P(sz)], vp
        getattr(L, f"ws_{owner}_frontier_download").argtypes = [vp, vp, vp, vp, sz, sz, P(sz), P(sz)]
    L.ws_debug_frontier_timing.argtypes = [vp, i32, vp]
    L.ws_debug_store_frontier_timing.argtypes = [vp, i32, vp]
    for owner in ("map", "store"):
        getattr(L, f"ws_{owner}_reach").argtypes = [vp, vp, sz, i32, u32, u32, P(sz), P(sz), vp]
        f = getattr(L, f"ws_{owner}_reach_dev")
        f.argtypes, f.restype = [vp, P(sz)], vp
        getattr(L, f"ws_{owner}_reach_download").argtypes = [vp, vp, sz, P(sz)]
        getattr(L, f"ws_{owner}_reach_box").argtypes = [vp, vp, vp, vp]
        getattr(L, f"ws_{owner}_reach_lookup").argtypes = [vp, vp, sz, i32, vp]
        getattr(L, f"ws_{owner}_reach_lookup_dev").argtypes = [vp, vp, sz, i32, vp]
        getattr(L, f"ws_{owner}_reach_paths").argtypes = [vp, vp, sz, u32, vp, vp]
    L.ws_debug_reach_timing.argtypes = [vp, i32, vp]
    L.ws_debug_store_reach_timing.argtypes = [vp, i32, vp]
    L.ws_debug_reach_params.argtypes = [vp]
    L.ws_map_view_gain.argtypes = [vp, C.c_int, vp, vp, vp, sz, vp, sz, i32, i32, u32, vp]
    L.ws_store_view_gain.argtypes = [vp, vp, vp, vp, sz, vp, sz, i32, i32, i32, u32, vp]
    for owner in ("map", "store"):
        for part in ("records", "rays"):
            f = getattr(L, f"ws_{owner}_view_gain_{part}_dev")
            f.argtypes, f.restype = [vp, P(sz)], vp
        getattr(L, f"ws_{owner}_view_gain_download").argtypes = [vp, vp, vp, sz, sz, P(sz), P(sz)]
    L.ws_debug_view_gain_timing.argtypes = [vp, i32, vp]
    L.ws_debug_store_view_gain_timing.argtypes = [vp, i32, vp]
    L.ws_map_clearance.argtypes = [vp, vp, sz, sz, vp, sz, i32, u32, P(i64)]
    L.ws_map_clearance_dev.argtypes = [vp, vp, sz, sz, vp, sz, i32, u32, P(i64)]
    L.ws_store_clearance.argtypes = [vp, vp, sz, sz, vp, sz, i32, i32, u32, P(i64)]
    L.ws_store_clearance_dev.argtypes = [vp, vp, sz, sz, vp, sz, i32, i32, u32, P(i64)]
    for owner in ("map", "store"):
        for part in ("records", "poses"):
            f = getattr(L, f"ws_{owner}_clearance_{part}_dev")
            f.argtypes, f.restype = [vp, P(sz)], vp
        getattr(L, f"ws_{owner}_clearance_download").argtypes = [vp, vp, vp, sz, sz, P(sz), P(sz)]
    L.ws_debug_clearance_timing.argtypes = [vp, i32, vp]
    L.ws_debug_store_clearance_timing.argtypes = [vp, i32, vp]
    L.ws_clearance_centres.argtypes = [vp, sz, vp, sz, i32, vp]
    L.ws_clearance_margin.argtypes, L.ws_clearance_margin.restype = [u32, i32, i32], i32
    L.ws_store_fuse.argtypes = [vp, vp, vp, i32, i32, u32, vp]
    L.ws_debug_store_fuse_timing.argtypes = [vp, i32, vp]
    L.ws_store_coarsen.argtypes = [vp, vp, vp, sz, i32, u32, vp]
    L.ws_store_parents_of.argtypes = [vp, sz, vp, sz, P(sz)]
    L.ws_debug_store_coarsen_timing.argtypes = [vp, i32, vp]
    L.ws_store_changes.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, u32, P(sz), P(sz), vp]
    for f in (L.ws_store_changes_records_dev, L.ws_store_changes_labels_dev, L.ws_store_changes_clusters_dev):
        f.argtypes, f.restype = [vp, P(sz)], vp
    L.ws_store_changes_download.argtypes = [vp, vp, vp, vp, sz, sz, P(sz), P(sz)]
    L.ws_debug_store_changes_timing.argtypes = [vp, i32, vp]
    L.ws_store_pack.argtypes = [vp, vp, sz, u32, P(sz), P(C.c_uint64), vp]
    L.ws_store_pack_headers_dev.argtypes, L.ws_store_pack_headers_dev.restype = [vp, P(sz)], vp
    L.ws_store_pack_payload_dev.argtypes, L.ws_store_pack_payload_dev.restype = [vp, P(C.c_uint64)], vp
    L.ws_store_pack_download.argtypes = [vp, vp, vp, sz, C.c_uint64, P(sz), P(C.c_uint64)]
    L.ws_store_unpack.argtypes = [vp, vp, vp, sz, C.c_uint64, u32, u32]
    L.ws_store_unpack_dev.argtypes = [vp, vp, vp, sz, C.c_uint64, u32, u32]
    L.ws_pack_check.argtypes = [vp, sz, C.c_uint64]
    L.ws_pack_expand_chunk.argtypes = [vp, vp, u32, vp]
    L.ws_pack_chunk.argtypes = [vp, vp, u32, vp, vp, C.c_uint64, P(C.c_uint64)]
    L.ws_debug_store_pack_timing.argtypes = [vp, i32, vp]
    L.ws_debug_reach_active.argtypes = [vp, vp, sz, P(sz)]
    L.ws_shift_plan.argtypes = [vp, vp, vp, vp, P(ShiftPlan)]
    L.ws_shift_begin.argtypes = [vp, vp, u32, P(vp)]
    L.ws_shift_count.argtypes = [vp]
    L.ws_shift_reserve.argtypes = [vp, C.c_uint64]
    L.ws_shift_entering.argtypes = [vp, C.c_int, vp, vp]
    L.ws_shift_wait.argtypes = [vp]
    L.ws_shift_slab.argtypes = [vp, C.c_int, vp, vp, P(vp)]
    L.ws_shift_end.argtypes = [vp]
    L.ws_map_device_data.argtypes = [vp, C.c_int]
    L.ws_map_device_data.restype = vp
    L.ws_map_n_voxels.argtypes = [vp]
    L.ws_map_n_voxels.restype = i64
    L.ws_tsdf_update.argtypes = [vp, vp, sz, vp, vp]
    L.ws_tsdf_update_dev.argtypes = [vp, vp, sz, vp, vp]
    L.ws_tsdf_scatter_dev.argtypes = [vp, vp, sz, vp, vp]
    L.ws_tsdf_integrate.argtypes = [vp]
    L.ws_tsdf_set_integrate.argtypes = [vp, C.c_int]
    L.ws_tsdf_set_capacity.argtypes = [vp, C.c_uint64]
    L.ws_tsdf_stats.argtypes = [vp, P(TsdfStats)]
    L.ws_reg_create.argtypes = [vp, sz, P(vp)]
    L.ws_reg_destroy.argtypes = [vp]
    L.ws_reg_prepare.argtypes = [vp, vp, sz]
    L.ws_reg_prepare_dev.argtypes = [vp, vp, sz]
    L.ws_reg_points_dev.argtypes = [vp, P(sz)]
    L.ws_reg_points_dev.restype = vp
    L.ws_reg_iterate.argtypes = [vp, vp, vp, i32, u32, vp, vp, P(i32), P(i32)]
    L.ws_register_cloud.argtypes = [vp, vp, vp, i32, C.c_float, C.c_float, i32, u32, vp, P(i32)]
    L.ws_reg_begin.argtypes = [vp, vp, i32, C.c_float, C.c_float]
    L.ws_reg_set_loop.argtypes = [vp, C.c_int]
    L.ws_reg_iterate_shard_dev.argtypes = [vp, vp, i32, u32, sz, sz, vp, i32]
    L.ws_debug_solve6.argtypes = [vp, vp, vp, sz, vp, vp]
    L.ws_debug_reg_stall.argtypes = [vp, C.c_int32, vp]
    L.ws_debug_reg_server.argtypes = [vp, C.c_int32, C.c_int32, vp]
    L.ws_debug_reg_mail_selftest.argtypes = []
    L.ws_debug_reg_sums.argtypes = [vp, vp]
    L.ws_debug_block_stats.argtypes = [vp, vp, sz]
    L.ws_debug_tsdf_chunk_policy.argtypes = [vp, C.c_uint64, u32]
    L.ws_scan_create.argtypes = [vp, sz, P(vp)]
    L.ws_scan_destroy.argtypes = [vp]
    L.ws_scan_preprocess.argtypes = [vp, vp, sz, sz, vp, i32, P(sz)]
    L.ws_scan_preprocess_dev.argtypes = [vp, vp, sz, sz, vp, i32, P(sz)]
    L.ws_scan_points_dev.argtypes = [vp]
    L.ws_scan_points_dev.restype = vp
    L.ws_scan_download.argtypes = [vp, vp, sz, P(sz)]
    L.ws_scan_preprocess_sweep.argtypes = [vp, vp, sz, sz, vp, u32, P(Sweep), i32, P(sz)]
    L.ws_scan_preprocess_sweep_dev.argtypes = [vp, vp, sz, sz, vp, u32, P(Sweep), i32, P(sz)]
    L.ws_sweep_poses.argtypes = [vp, vp, u32, vp]
    L.ws_reg_accumulate_dev.argtypes = [vp, vp, i32, u32, sz, sz, vp]
    L.ws_reg_solve_dev.argtypes = [vp, vp]
    L.ws_reg_poll.argtypes = [vp, P(i32), P(i32), vp]
    L.ws_reg_peer_mailbox.argtypes = [vp, vp]
    L.ws_reg_peer_connect.argtypes = [vp, i32, i32, vp, i32]
    L.ws_reg_peer_connect_local.argtypes = [vp, i32, i32, vp, i32]
    L.ws_reg_peer_disconnect.argtypes = [vp]
    L.ws_reg_peer_reset.argtypes = [vp]
    L.ws_register_cloud_peers.argtypes = [vp, vp, sz, sz, vp, i32, C.c_float, C.c_float, i32, u32, vp, P(i32)]
    L.ws_register_cloud_batch.argtypes = [vp, vp, vp, sz, i32, C.c_float, C.c_float, i32, u32, vp, vp, vp, vp]
    L.ws_reg_batch_best.argtypes = [vp, vp, sz, i32, P(i64)]
    L.ws_store_create.argtypes = [vp, u32, C.c_uint64, u32, P(vp)]
    L.ws_store_destroy.argtypes = [vp]
    L.ws_store_reserve.argtypes = [vp, C.c_uint64]
    L.ws_store_count.argtypes = [vp, P(C.c_uint64), P(C.c_uint64)]
    L.ws_store_keys.argtypes = [vp, vp, sz, P(sz)]
    L.ws_store_has.argtypes = [vp, vp]
    L.ws_store_get_chunk.argtypes = [vp, vp, vp, P(i32)]
    L.ws_store_put_chunk.argtypes = [vp, vp, vp]
    L.ws_store_drop_chunk.argtypes = [vp, vp]
    L.ws_store_chunk_dev.argtypes = [vp, vp]
    L.ws_store_chunk_dev.restype = vp
    L.ws_store_save_box.argtypes = [vp, vp, C.c_int, vp, vp]
    L.ws_store_load_box.argtypes = [vp, vp, C.c_int, vp, vp]
    L.ws_shift_device.argtypes = [vp, vp, vp]
    L.ws_store_chunks_of_box.argtypes = [vp, vp, vp, sz, P(sz)]
    L.ws_debug_store_timing.argtypes = [vp, i32, vp]
    L.ws_store_surface.argtypes = [vp, vp, vp, i32, i32, i32, u32, P(sz)]
    L.ws_store_surface_records_dev.argtypes = [vp, P(sz)]
    L.ws_store_surface_records_dev.restype = vp
    L.ws_store_surface_marker_dev.argtypes = [vp, P(sz)]
    L.ws_store_surface_marker_dev.restype = vp
    L.ws_store_surface_download.argtypes = [vp, vp, vp, sz, P(sz)]
    L.ws_debug_store_surface_timing.argtypes = [vp, i32, vp]
    L.ws_store_mesh.argtypes = [vp, vp, vp, i32, u32, P(sz), P(sz)]
    L.ws_store_mesh_vertices_dev.argtypes = [vp, P(sz)]
    L.ws_store_mesh_vertices_dev.restype = vp
    L.ws_store_mesh_faces_dev.argtypes = [vp, P(sz)]
    L.ws_store_mesh_faces_dev.restype = vp
    L.ws_store_mesh_download.argtypes = [vp, vp, vp, sz, sz, P(sz), P(sz)]
    L.ws_debug_store_mesh_timing.argtypes = [vp, i32, vp]
    L.ws_store_distance.argtypes = [vp, vp, vp, i32, u32, P(sz)]
    L.ws_store_distance_dev.argtypes = [vp, P(sz)]
    L.ws_store_distance_dev.restype = vp
    L.ws_store_distance_download.argtypes = [vp, vp, sz, P(sz)]
    L.ws_debug_store_distance_timing.argtypes = [vp, i32, vp]
    L.ws_store_ground.argtypes = [vp, vp, vp, i32, u32, vp]
    L.ws_store_ground_dev.argtypes = [vp, P(sz)]
    L.ws_store_ground_dev.restype = vp
    L.ws_store_ground_download.argtypes = [vp, vp, sz, P(sz)]
    L.ws_store_ground_box.argtypes = [vp, vp, vp]
    L.ws_debug_store_ground_timing.argtypes = [vp, i32, vp]
    L.ws_store_ground_distance.argtypes = [vp, i32, i32, u32, P(sz)]
    L.ws_store_raycast.argtypes = [vp, vp, vp, vp, vp, sz, i32, i32, u32, P(sz)]
    L.ws_store_raycast_dev.argtypes = [vp, vp, vp, vp, vp, sz, i32, i32, u32, P(sz)]
    L.ws_store_raycast_records_dev.argtypes = [vp, P(sz)]
    L.ws_store_raycast_records_dev.restype = vp
    L.ws_store_raycast_gradient_dev.argtypes = [vp, P(sz)]
    L.ws_store_raycast_gradient_dev.restype = vp
    L.ws_store_raycast_download.argtypes = [vp, vp, vp, sz, P(sz)]
    L.ws_debug_store_raycast_timing.argtypes = [vp, i32, vp]
    L.ws_debug_store_raycast_table.argtypes = [vp, sz, vp, sz, P(sz)]
    L.ws_debug_store_raycast_find.argtypes = [vp, sz, vp]
    L.ws_debug_store_raycast_find.restype = u32
    L.ws_prof_enable.argtypes = [vp, u32]
    L.ws_prof_read.argtypes = [vp, C.c_int, P(C.c_double), P(i64)]
    L.ws_prof_reset.argtypes = [vp]
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().ws_last_error()
        raise WsError(f"{what} failed with status {rc}: {msg.decode(errors='replace') if msg else ''}")
