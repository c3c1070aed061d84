"""warpsense_amd — MI355X-native TSDF update and Point-to-TSDF registration (the hot path of warpsense).

The compute lives in libwarpsense_hip.so (warpsense_amd/csrc, C ABI in include/warpsense_hip.h);
this package is the thin host-side mirror of the reference's device API plus the synthetic workload.
"""
from .api import (Context, DeviceGlobalMap, chunks_of_box, DeviceMap, DeviceMapMemWrapper, DevicePoints, GlobalMap, LocalMap, MapParams, Params, RegistrationCuda,  # noqa: F401
                  RegistrationParams, ScanPreprocessor, TSDFCuda, TSDFMapping, TSDFRegistration, cleanup, pack_entry, pause, pose_to_values, to_int_mat,
                  to_map, unpack_entry, SURFACE_RECORD, write_surface_ply, VERT, write_mesh_ply, RAY, write_raycast_ply, SAMPLE, SAMPLE_CLASSES, distance_class, distance_d2, distance_mm, batch_best, candidate_poses, sweep_poses, sweep_bins, preprocess_sweep_host)
from ._lib import (WS_INTEGRATE_DENSE, WS_INTEGRATE_SPARSE, WS_INTEGRATE_SPARSE_SEPARATE, WS_MAP_AVG, WS_MAP_NEW, WS_REG_ALL_POINTS,  # noqa: F401
                   WS_REG_COMPAT_REFERENCE_LAUNCH, WS_REG_LOOP_LAUNCHES, WS_REG_LOOP_RESIDENT, WS_DISTANCE_ANY_WEIGHT, WS_DISTANCE_COLUMNS, WS_DISTANCE_DEFAULT, WS_DISTANCE_UNKNOWN_OCCUPIED, WS_FRONTIER_ANY_WEIGHT, WS_FRONTIER_CLUSTERS, WS_FRONTIER_DEFAULT, WS_MESH_ANY_WEIGHT, WS_MESH_DEFAULT, WS_RAYCAST_ANY_WEIGHT, WS_RAYCAST_DEFAULT, WS_RAYCAST_GRADIENT, WS_RAYCAST_TARGETS, WS_SURFACE_MARKER, WS_SURFACE_RECORDS, WsError)
from .records import FRONTIER_CLUSTER, FRONTIER_RECORD, frontier_goals, write_frontier_ply  # noqa: F401
from .records import REACH_PATH_HEADER, REACH_PATH_RECORD, REACH_UNREACHABLE, reach_mm, write_path_ply  # noqa: F401
from ._lib import WS_REACH_DEFAULT, WS_REACH_UNKNOWN_FREE, WS_REACH_UNREACHABLE  # noqa: F401
from .records import VIEW_GAIN_RAY, VIEW_GAIN_RECORD, gain_volume_m3, rank_views, view_fan  # noqa: F401
from ._lib import WS_GAIN_ANY_WEIGHT, WS_GAIN_DEFAULT, WS_GAIN_RAYS  # noqa: F401
from .clearance import CLEARANCE_POSE, CLEARANCE_RECORD, ClearanceResult, arc_rollouts, body_spheres, clearance_centres, clearance_margin, trajectory_poses  # noqa: F401
from ._lib import WS_CLEARANCE_DEFAULT, WS_CLEARANCE_OUTSIDE_OK, WS_CLEARANCE_POSES  # noqa: F401
from .fuse import FuseStats, fuse_pose, pose_transform  # noqa: F401
from ._lib import WS_FUSE_COUNT_ONLY, WS_FUSE_DEFAULT  # noqa: F401
from .pyramid import CoarsenStats, MapPyramid, parents_of  # noqa: F401
from ._lib import WS_COARSEN_DEFAULT  # noqa: F401
from .changes import CHANGE_RECORD, ChangeResult, ChangeStats, write_changes_ply  # noqa: F401
from .pack import PackedMap  # noqa: F401
from .ground import GROUND_RECORD, GroundResult, max_step_q8  # noqa: F401
from ._lib import WS_GROUND_ANY_WEIGHT, WS_GROUND_DEFAULT, WS_GROUND_TOP, WS_GROUND_UNKNOWN_HEADROOM  # noqa: F401
from ._lib import WS_CHANGES_APPEARED, WS_CHANGES_CLUSTERS, WS_CHANGES_DEFAULT, WS_CHANGES_VANISHED  # noqa: F401

__all__ = [n for n in dir() if not n.startswith("_")]
from .app import App  # noqa: F401,E402
