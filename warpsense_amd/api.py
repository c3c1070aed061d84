"""Host-side mirror of the reference's device API over the C ABI (include/warpsense_hip.h).

Same names, argument meaning and error behaviour as the reference classes, so tests read like the
reference's own (test/cuda.cpp, test/pcd_registration.cpp):

    DeviceMap            include/warpsense/cuda/device_map.h:32-164     (non-owning host view)
    DeviceMapMemWrapper  include/warpsense/cuda/device_map_wrapper.h:10-36
    TSDFCuda             include/warpsense/cuda/update_tsdf.h:9-34
    RegistrationCuda     include/warpsense/cuda/registration.h:10-45
    TSDFMapping          src/warpsense/tsdf_mapping.cpp:30-95            (ROS-free constructor path)
    TSDFRegistration     src/warpsense/tsdf_registration.cpp:22-96
    pause / cleanup      src/warpsense/cuda/cleanup.cu

Matrices handed to these classes are ordinary numpy 4x4 arrays (math layout, M[i, j]); the column-major
flattening the C ABI wants (rmagine::Matrix4x4f / Eigen) happens here.  All compute runs in the HIP
library; nothing here falls back to the CPU.

This module only gathers the names; the code lives in one module per subsystem, cut like the C side (csrc/api_*.hip):

    _abi.py          pointers, three-int and column-major forms, the packed entry, device buffers as tensors
    records.py       the record dtypes of the queries, the distance record's parts, the PLY writers
    context.py       Context, pause, cleanup                                        (api_core)
    scan.py          DevicePoints, ScanPreprocessor, the sweep rules and host model (api_scan)
    queries.py       what window and store queries share: box, call, result, timing (api_query)
    global_map.py    GlobalMap on the host and its .h5 file, pose_to_values
    store.py         DeviceGlobalMap, chunks_of_box                                 (api_store, api_store_query)
    fuse.py          fuse_pose, FuseStats: one global map fused into another        (api_store_pair)
    merge.py         merge_map and align_map of TSDFMapping
    pyramid.py       CoarsenStats, parents_of, MapPyramid, global_pyramid           (api_store_pair)
    changes.py       ChangeStats, ChangeResult, write_changes_ply: where two maps differ (api_store_pair)
    ground.py        GROUND_RECORD, GroundResult: levels, heights and steps of the ground  (api_query, api_store_query)
    pack.py          PackedMap: packed snapshots of the global map and their .wspk file (api_pack)
    device_map.py    DeviceMap, LocalMap, DeviceMapMemWrapper, TSDFCuda             (api_map, api_tsdf)
    registration.py  RegistrationCuda, batch_best, candidate_poses                  (api_reg)
    mapping.py       the parameters, TSDFMapping, TSDFRegistration
"""
from __future__ import annotations

from ._abi import MATRIX_RESOLUTION, WEIGHT_RESOLUTION, pack_entry, unpack_entry  # noqa: F401
from ._lib import (WS_INTEGRATE_DENSE, WS_INTEGRATE_SPARSE, WS_MAP_AVG, WS_MAP_NEW, WS_REG_ALL_POINTS,  # noqa: F401
                   WS_REG_COMPAT_REFERENCE_LAUNCH, WsError, check)
from .context import Context, cleanup, pause  # noqa: F401
from .device_map import DeviceMap, DeviceMapMemWrapper, LocalMap, TSDFCuda  # noqa: F401
from .global_map import GlobalMap, pose_to_values  # noqa: F401
from .mapping import MapParams, Params, RegistrationParams, TSDFMapping, TSDFRegistration  # noqa: F401
from .records import (FRONTIER_CLUSTER, FRONTIER_RECORD, REACH_PATH_HEADER, REACH_PATH_RECORD, REACH_UNREACHABLE, frontier_goals, reach_mm, write_frontier_ply, write_path_ply, RAY, SAMPLE, SAMPLE_CLASSES, SURFACE_RECORD, VERT, distance_class, distance_d2, distance_mm,  # noqa: F401
                      write_mesh_ply, write_raycast_ply, write_surface_ply)
from .clearance import CLEARANCE_POSE, CLEARANCE_RECORD, ClearanceResult, arc_rollouts, body_spheres, clearance_centres, clearance_margin, trajectory_poses  # noqa: F401
from .records import VIEW_GAIN_RAY, VIEW_GAIN_RECORD, gain_volume_m3, rank_views, view_fan  # noqa: F401
from .registration import RegistrationCuda, batch_best, candidate_poses  # noqa: F401
from .scan import DevicePoints, ScanPreprocessor, preprocess_sweep_host, sweep_bins, sweep_poses, to_int_mat, to_map  # noqa: F401
from .store import DeviceGlobalMap, chunks_of_box  # noqa: F401
from .fuse import FuseStats, fuse_pose, pose_transform  # noqa: F401
from .pyramid import CoarsenStats, MapPyramid, parents_of  # noqa: F401
from .changes import CHANGE_RECORD, ChangeResult, ChangeStats, write_changes_ply  # noqa: F401
from .pack import PackedMap  # noqa: F401
from .ground import GROUND_RECORD, GroundResult, max_step_q8  # noqa: F401
