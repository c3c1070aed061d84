// visualization.hpp — the data behind the reference's two map markers (include/warpsense/visualization/map.h), without ROS:
//
//   local_map_cloud      publish_local_map           map.h:14-121    the surface cloud of a DEVICE map, over ws_map_surface
//   global_map_cloud     pcl_writer's exported map, without the export                        the surface cloud of the device global map, over ws_store_surface
//   local_map_mesh       (no counterpart: the reference sends the user to an offline mesher)   a triangle mesh, over ws_map_mesh
//   global_map_mesh      (no counterpart)                                                     the mesh of the device global map, over ws_store_mesh
//   local_map_raycast    (no counterpart: the reference leaves all viewing to RViz)            a predicted scan, over ws_map_raycast
//   global_map_raycast   (no counterpart)                                                     a predicted scan from anywhere the run has been, over ws_store_raycast
//   local_map_sample / global_map_sample   (no counterpart)                                   what the map says at given points, over ws_map_sample / ws_store_sample
//   local_map_distance   (no counterpart: the reference has no distance field)                   a cost map, over ws_map_distance
//   global_map_distance  (no counterpart)                                                     the cost map of the whole run, over ws_store_distance
//   local_map_ground / global_map_ground (no counterpart)                                    the elevation layer a ground robot plans on, over ws_map_ground / ws_store_ground
//   local_map_frontier / global_map_frontier   (no counterpart)                               where the known world ends, over ws_map_frontier / ws_store_frontier
//   local_map_reach / global_map_reach, local_map_reach_paths / global_map_reach_paths   (no counterpart)   path costs and paths, over ws_map_reach / ws_store_reach
//   local_map_view_gain / global_map_view_gain   (no counterpart)                             what the sensor would see from candidate poses, over ws_map_view_gain / ws_store_view_gain
//   local_map_clearance / global_map_clearance   (no counterpart)                             candidate trajectories of a body of spheres against the last distance result, over ws_map_clearance / ws_store_clearance
//   local_map_skeleton   publish_local_map_skeleton  map.h:175-227   the 24 end points of the window's line list (host only)
//
// The reference walks every voxel of a host map (after a whole-map download for the CUDA map, test/pcd2tsdf.cpp:134-137); here
// the selection runs on the device and only the qualifying voxels travel.  What a caller with ROS does with the result is the
// rest of map.h: marker.points / marker.colors from the 7 floats per point (x y z r g b a, a float widened to the double of
// geometry_msgs::Point is the same number), header, scale = map_resolution * 0.6 / 1000.
// There is deliberately no forwarding header under the reference's visualization/map.h name: its functions take a ros::Publisher.
#pragma once

#include <algorithm>
#include <array>
#include <vector>

#include "warpsense_hip/compat.hpp"

namespace warpsense
{
struct SurfaceRecord // one record of ws_map_surface
{
  int32_t x, y, z; // world voxels
  uint32_t raw;    // the packed TSDFEntry
};
static_assert(sizeof(SurfaceRecord) == 16, "ws_map_surface writes 16-byte records");

struct SurfaceCloud
{
  std::vector<SurfaceRecord> records; // ascending world (x, y, z), z fastest
  std::vector<float> marker;          // 7 floats per record (x y z in metres, r g b a), empty unless asked for
};

// The voxels of `which` (WS_MAP_AVG / WS_MAP_NEW) with weight > 0 && abs(value) < band (map.h:45; band <= 0: tau) inside the
// inclusive world-voxel box [lo, hi] (both nullptr: the whole window, map.h:19-26).
inline SurfaceCloud local_map_cloud(cuda::TSDFCuda &tsdf, int which = WS_MAP_AVG, bool marker = true, const rmagine::Pointi *lo = nullptr,
                                    const rmagine::Pointi *hi = nullptr, int band = 0)
{
  SurfaceCloud out;
  size_t n = 0;
  WS_CHECK(ws_map_surface(tsdf.handle(), which, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, band, marker ? WS_SURFACE_MARKER : WS_SURFACE_RECORDS, &n));
  out.records.resize(n);
  if (marker) out.marker.resize(n * 7);
  size_t got = 0;
  WS_CHECK(ws_map_surface_download(tsdf.handle(), n ? out.records.data() : nullptr, n && marker ? out.marker.data() : nullptr, n, &got));
  return out;
}

// The surface cloud of the global map in device memory (the rules: warpsense_hip.h at ws_store_surface): the qualifying voxels of the
// store's chunks inside the inclusive world-voxel box [lo, hi] (both nullptr: every present chunk), in the order of local_map_cloud
// across chunk borders.  tau, resolution: the map's (the store knows neither).  (app.hpp adds the overload that takes a DeviceGlobalMap.)
inline SurfaceCloud global_map_cloud(ws_store *store, int tau, int resolution, bool marker = true, const rmagine::Pointi *lo = nullptr,
                                     const rmagine::Pointi *hi = nullptr, int band = 0)
{
  SurfaceCloud out;
  size_t n = 0;
  WS_CHECK(ws_store_surface(store, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, band, tau, resolution, marker ? WS_SURFACE_MARKER : WS_SURFACE_RECORDS, &n));
  out.records.resize(n);
  if (marker) out.marker.resize(n * 7);
  size_t got = 0;
  WS_CHECK(ws_store_surface_download(store, n ? out.records.data() : nullptr, n && marker ? out.marker.data() : nullptr, n, &got));
  return out;
}

struct FrontierRecord // one record of ws_map_frontier
{
  int32_t x, y, z; // world voxels
  uint32_t mask;   // bits 0..5: an UNKNOWN neighbour at -x +x -y +y -z +z
};
struct FrontierCluster // one row of its cluster table
{
  uint32_t first, count; // record index of the first member, members
  int32_t lo[3], hi[3];  // the bounding box in world voxels
  int64_t sum[3];        // the sum of the members' coordinates
  uint64_t pad;
};
static_assert(sizeof(FrontierRecord) == 16 && sizeof(FrontierCluster) == 64, "ws_map_frontier writes 16-byte records and 64-byte rows");

struct Frontier
{
  std::vector<FrontierRecord> records;   // ascending world (x, y, z), z fastest
  std::vector<uint32_t> labels;          // the cluster number of every record; empty unless asked for
  std::vector<FrontierCluster> clusters; // numbered by their first record; empty unless asked for
};

// The frontier of `which` (the rules: warpsense_hip.h at ws_map_frontier) inside the inclusive world-voxel box [lo, hi] (both nullptr:
// the whole window): the voxels that are observed free (value >= min_value; 0: any non-negative value) and touch a never-observed
// voxel of the box; with `clusters` their 26-connected patches as labels and a table.
inline Frontier local_map_frontier(cuda::TSDFCuda &tsdf, int which = WS_MAP_AVG, bool clusters = true, int32_t min_value = 0, bool any_weight = false,
                                   const rmagine::Pointi *lo = nullptr, const rmagine::Pointi *hi = nullptr)
{
  Frontier out;
  size_t n = 0, k = 0;
  const uint32_t flags = (any_weight ? WS_FRONTIER_ANY_WEIGHT : 0u) | (clusters ? WS_FRONTIER_CLUSTERS : 0u);
  WS_CHECK(ws_map_frontier(tsdf.handle(), which, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, min_value, flags, &n, &k));
  out.records.resize(n);
  if (clusters) out.labels.resize(n), out.clusters.resize(k);
  size_t got = 0, got_k = 0;
  WS_CHECK(ws_map_frontier_download(tsdf.handle(), n ? out.records.data() : nullptr, n && clusters ? out.labels.data() : nullptr,
                                    k && clusters ? out.clusters.data() : nullptr, n, k, &got, &got_k));
  return out;
}

// The frontier of the global map in device memory (the rules: warpsense_hip.h at ws_store_frontier) inside the inclusive world-voxel
// box [lo, hi] (both nullptr: the bounding box of the present chunks, whose faces are no frontier: pass a box one voxel larger to get the
// outer faces of the mapped volume).  Voxels of absent chunks are unknown.  (app.hpp adds the overload that takes a DeviceGlobalMap.)
inline Frontier global_map_frontier(ws_store *store, bool clusters = true, int32_t min_value = 0, bool any_weight = false, const rmagine::Pointi *lo = nullptr,
                                    const rmagine::Pointi *hi = nullptr)
{
  Frontier out;
  size_t n = 0, k = 0;
  const uint32_t flags = (any_weight ? WS_FRONTIER_ANY_WEIGHT : 0u) | (clusters ? WS_FRONTIER_CLUSTERS : 0u);
  WS_CHECK(ws_store_frontier(store, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, min_value, flags, &n, &k));
  out.records.resize(n);
  if (clusters) out.labels.resize(n), out.clusters.resize(k);
  size_t got = 0, got_k = 0;
  WS_CHECK(ws_store_frontier_download(store, n ? out.records.data() : nullptr, n && clusters ? out.labels.data() : nullptr,
                                      k && clusters ? out.clusters.data() : nullptr, n, k, &got, &got_k));
  return out;
}

struct ViewGainRecord // one record of ws_map_view_gain per view
{
  uint64_t unknown_k2, free_k2; // the sums of k^2 over the UNKNOWN / FREE samples
  uint32_t unknown, free_n;     // UNKNOWN / FREE samples
  uint32_t blocked, live;       // rays that ended at an OCCUPIED voxel; rays that are not dead
};
struct ViewGainRay // with rays: one record per (view, ray), view-major
{
  uint32_t unknown; // the UNKNOWN samples of the ray
  int32_t stop;     // the k of the blocking sample, -1 for none, -2 for a dead ray
};
static_assert(sizeof(ViewGainRecord) == 32 && sizeof(ViewGainRay) == 8, "ws_map_view_gain writes 32-byte view records and 8-byte ray records");

struct ViewGain
{
  std::vector<ViewGainRecord> records; // one per origin, in their order
  std::vector<ViewGainRay> rays;       // [view][ray]; empty unless asked for
  uint64_t best_unknown_k2 = 0;        // the largest unknown_k2 of the views
};

// What the sensor would see from `origins` (map frame, mm) along the one fan `dirs` (any length, the rules of local_map_raycast) in
// `which` (the rules: warpsense_hip.h at ws_map_view_gain) inside the inclusive world-voxel box [lo, hi] (both nullptr: the whole
// window): per view the UNKNOWN and FREE samples before a voxel with value < min_value blocks the ray, as counts and weighted by k^2.
// No origin or no direction: an empty result, nothing is called.
inline ViewGain local_map_view_gain(cuda::TSDFCuda &tsdf, const std::vector<rmagine::Pointi> &origins, const std::vector<rmagine::Pointi> &dirs, int32_t max_range_mm,
                                    int which = WS_MAP_AVG, int32_t min_value = 0, bool any_weight = false, bool with_rays = false, const rmagine::Pointi *lo = nullptr,
                                    const rmagine::Pointi *hi = nullptr)
{
  ViewGain out;
  if (origins.empty() || dirs.empty()) return out;
  const uint32_t flags = (any_weight ? WS_GAIN_ANY_WEIGHT : 0u) | (with_rays ? WS_GAIN_RAYS : 0u);
  WS_CHECK(ws_map_view_gain(tsdf.handle(), which, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, &origins[0].x, origins.size(), &dirs[0].x, dirs.size(), max_range_mm,
                            min_value, flags, &out.best_unknown_k2));
  out.records.resize(origins.size());
  if (with_rays) out.rays.resize(origins.size() * dirs.size());
  size_t got = 0, got_rays = 0;
  WS_CHECK(ws_map_view_gain_download(tsdf.handle(), out.records.data(), with_rays ? out.rays.data() : nullptr, out.records.size(), out.rays.size(), &got, &got_rays));
  return out;
}

// The same through the global map in device memory (the rules: warpsense_hip.h at ws_store_view_gain) inside the inclusive world-voxel
// box [lo, hi] (both nullptr: the bounding box of the present chunks).  Voxels of absent chunks are unknown: they count and block
// nothing.  resolution: the map's (the store does not know it).  (app.hpp adds the overload that takes a DeviceGlobalMap.)
inline ViewGain global_map_view_gain(ws_store *store, int resolution, const std::vector<rmagine::Pointi> &origins, const std::vector<rmagine::Pointi> &dirs,
                                     int32_t max_range_mm, int32_t min_value = 0, bool any_weight = false, bool with_rays = false, const rmagine::Pointi *lo = nullptr,
                                     const rmagine::Pointi *hi = nullptr)
{
  ViewGain out;
  if (origins.empty() || dirs.empty()) return out;
  const uint32_t flags = (any_weight ? WS_GAIN_ANY_WEIGHT : 0u) | (with_rays ? WS_GAIN_RAYS : 0u);
  WS_CHECK(ws_store_view_gain(store, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, &origins[0].x, origins.size(), &dirs[0].x, dirs.size(), max_range_mm, resolution,
                              min_value, flags, &out.best_unknown_k2));
  out.records.resize(origins.size());
  if (with_rays) out.rays.resize(origins.size() * dirs.size());
  size_t got = 0, got_rays = 0;
  WS_CHECK(ws_store_view_gain_download(store, out.records.data(), with_rays ? out.rays.data() : nullptr, out.records.size(), out.rays.size(), &got, &got_rays));
  return out;
}

struct ClearanceRecord // one record of ws_map_clearance per trajectory
{
  int32_t min_margin, first_hit;           // the smallest margin (INT32_MAX without a sample inside the box); the first pose with a hit, -1 for none
  uint32_t argmin, hits, outside, unknown; // p * 64 + k of the first sample at min_margin (0xFFFFFFFF for none); the counts
  uint64_t cost;                           // the sum of max(0, soft_mm - margin)^2
};
struct ClearancePose // with per_pose: one record per (trajectory, pose), trajectory-major
{
  int32_t min_margin;
  uint16_t hits, outside;
};
static_assert(sizeof(ClearanceRecord) == 32 && sizeof(ClearancePose) == 8, "ws_map_clearance writes 32-byte trajectory records and 8-byte pose records");
struct ClearanceSphere // one sphere of the body: the centre in the body frame and the radius, mm
{
  int32_t off_mm[3], radius_mm;
};
struct ClearanceInput // one pose of a trajectory: rot_q30 row-major (the convention of ws_fuse_pose), then the position in the map frame, mm
{
  int32_t rot_q30[9], pos_mm[3];
};
static_assert(sizeof(ClearanceSphere) == 16 && sizeof(ClearanceInput) == 48, "ws_map_clearance reads 4 int32 per sphere and 12 per pose");

struct Clearance
{
  std::vector<ClearanceRecord> records; // one per trajectory, in their order
  std::vector<ClearancePose> poses;     // [trajectory][pose]; empty unless asked for
  int64_t best = -1;                    // the trajectory without a hit (and without an outside sample unless outside_ok) of the smallest (cost, index)
};

// `poses` (trajectory-major, n_poses per trajectory) and a body of spheres against the LAST distance result of the map (ws_map_distance
// or ws_map_ground_distance; the rules: warpsense_hip.h at ws_map_clearance).  No pose: an empty result, nothing is called.
inline Clearance local_map_clearance(cuda::TSDFCuda &tsdf, const std::vector<ClearanceInput> &poses, size_t n_poses, const std::vector<ClearanceSphere> &body,
                                     int32_t soft_mm = 0, bool per_pose = false, bool outside_ok = false)
{
  Clearance out;
  if (poses.empty() || n_poses == 0) return out;
  if (poses.size() % n_poses) throw std::invalid_argument("local_map_clearance: the poses are no whole number of trajectories");
  const size_t t = poses.size() / n_poses;
  const uint32_t flags = (per_pose ? WS_CLEARANCE_POSES : 0u) | (outside_ok ? WS_CLEARANCE_OUTSIDE_OK : 0u);
  WS_CHECK(ws_map_clearance(tsdf.handle(), poses[0].rot_q30, t, n_poses, body.empty() ? nullptr : body[0].off_mm, body.size(), soft_mm, flags, &out.best));
  out.records.resize(t);
  if (per_pose) out.poses.resize(poses.size());
  size_t got = 0, got_poses = 0;
  WS_CHECK(ws_map_clearance_download(tsdf.handle(), out.records.data(), per_pose ? out.poses.data() : nullptr, out.records.size(), out.poses.size(), &got, &got_poses));
  return out;
}

// The same against the last distance result of the global map in device memory (ws_store_distance or ws_store_ground_distance).
// resolution: the map's (the store does not know it).  (app.hpp adds the overload that takes a DeviceGlobalMap.)
inline Clearance global_map_clearance(ws_store *store, int resolution, const std::vector<ClearanceInput> &poses, size_t n_poses, const std::vector<ClearanceSphere> &body,
                                      int32_t soft_mm = 0, bool per_pose = false, bool outside_ok = false)
{
  Clearance out;
  if (poses.empty() || n_poses == 0) return out;
  if (poses.size() % n_poses) throw std::invalid_argument("global_map_clearance: the poses are no whole number of trajectories");
  const size_t t = poses.size() / n_poses;
  const uint32_t flags = (per_pose ? WS_CLEARANCE_POSES : 0u) | (outside_ok ? WS_CLEARANCE_OUTSIDE_OK : 0u);
  WS_CHECK(ws_store_clearance(store, poses[0].rot_q30, t, n_poses, body.empty() ? nullptr : body[0].off_mm, body.size(), soft_mm, resolution, flags, &out.best));
  out.records.resize(t);
  if (per_pose) out.poses.resize(poses.size());
  size_t got = 0, got_poses = 0;
  WS_CHECK(ws_store_clearance_download(store, out.records.data(), per_pose ? out.poses.data() : nullptr, out.records.size(), out.poses.size(), &got, &got_poses));
  return out;
}

struct ReachField // the result of ws_map_reach / ws_store_reach
{
  std::vector<uint32_t> cost; // one per record of the distance result it ran on, in its order; WS_REACH_UNREACHABLE without a path
  size_t seeded = 0, reached = 0;
  uint32_t rounds = 0;
  rmagine::Pointi lo;         // the box of the result: first voxel, and the extent (nx, ny, nz; a column map: nx, ny, 1)
  uint32_t ext[3] = {0, 0, 0};
  bool columns = false;
};
struct ReachPathHeader // one goal of ws_map_reach_paths
{
  uint32_t cost, steps, written, status; // status: 0 reached, 1 not reachable, 2 outside the box
};
struct ReachPathRecord
{
  int32_t x, y, z; // world voxels
  uint32_t cost;
};
static_assert(sizeof(ReachPathHeader) == 16 && sizeof(ReachPathRecord) == 16, "ws_map_reach_paths writes 16-byte headers and records");
struct ReachPaths
{
  std::vector<ReachPathHeader> headers; // one per goal
  std::vector<ReachPathRecord> records; // cap_steps per goal, goal first; zero beyond `written`
  uint32_t cap_steps = 0;
};

// The geodesic field over the LAST distance result of the map (the rules: warpsense_hip.h at ws_map_reach): call local_map_distance
// first.  seeds: world voxels.  clear_d2: the squared clearance in voxels a path keeps.
inline ReachField local_map_reach(cuda::TSDFCuda &tsdf, const std::vector<rmagine::Pointi> &seeds, int32_t clear_d2 = 0, bool unknown_free = false,
                                  uint32_t max_rounds = 0)
{
  ReachField out;
  WS_CHECK(ws_map_reach(tsdf.handle(), seeds.empty() ? nullptr : &seeds[0].x, seeds.size(), clear_d2, unknown_free ? WS_REACH_UNKNOWN_FREE : WS_REACH_DEFAULT,
                        max_rounds, &out.seeded, &out.reached, &out.rounds));
  size_t n = 0, got = 0;
  int32_t columns = 0;
  ws_map_reach_dev(tsdf.handle(), &n);
  out.cost.resize(n);
  WS_CHECK(ws_map_reach_download(tsdf.handle(), n ? out.cost.data() : nullptr, n, &got));
  WS_CHECK(ws_map_reach_box(tsdf.handle(), &out.lo.x, out.ext, &columns));
  out.columns = columns != 0;
  return out;
}

// the same over the last distance result of the global map in device memory (ws_store_reach; app.hpp adds the DeviceGlobalMap overload)
inline ReachField global_map_reach(ws_store *store, const std::vector<rmagine::Pointi> &seeds, int32_t clear_d2 = 0, bool unknown_free = false,
                                   uint32_t max_rounds = 0)
{
  ReachField out;
  WS_CHECK(ws_store_reach(store, seeds.empty() ? nullptr : &seeds[0].x, seeds.size(), clear_d2, unknown_free ? WS_REACH_UNKNOWN_FREE : WS_REACH_DEFAULT, max_rounds,
                          &out.seeded, &out.reached, &out.rounds));
  size_t n = 0, got = 0;
  int32_t columns = 0;
  ws_store_reach_dev(store, &n);
  out.cost.resize(n);
  WS_CHECK(ws_store_reach_download(store, n ? out.cost.data() : nullptr, n, &got));
  WS_CHECK(ws_store_reach_box(store, &out.lo.x, out.ext, &columns));
  out.columns = columns != 0;
  return out;
}

// The paths of the last reach result from `goals` (world voxels) back to a seed (ws_map_reach_paths); cap_steps = 0: the headers alone
inline ReachPaths local_map_reach_paths(cuda::TSDFCuda &tsdf, const std::vector<rmagine::Pointi> &goals, uint32_t cap_steps)
{
  ReachPaths out;
  out.cap_steps = cap_steps;
  out.headers.resize(goals.size());
  out.records.resize(goals.size() * (size_t)cap_steps);
  if (!goals.empty())
    WS_CHECK(ws_map_reach_paths(tsdf.handle(), &goals[0].x, goals.size(), cap_steps, out.headers.data(), cap_steps ? out.records.data() : nullptr));
  return out;
}

inline ReachPaths global_map_reach_paths(ws_store *store, const std::vector<rmagine::Pointi> &goals, uint32_t cap_steps)
{
  ReachPaths out;
  out.cap_steps = cap_steps;
  out.headers.resize(goals.size());
  out.records.resize(goals.size() * (size_t)cap_steps);
  if (!goals.empty()) WS_CHECK(ws_store_reach_paths(store, &goals[0].x, goals.size(), cap_steps, out.headers.data(), cap_steps ? out.records.data() : nullptr));
  return out;
}

struct MeshVertex // one vertex of ws_map_mesh
{
  int32_t x_mm, y_mm, z_mm; // world position in millimetres
  uint32_t weight;          // the smallest corner weight of the vertex's cell
};
struct MeshFace
{
  uint32_t v[3]; // vertex indices, normal towards the outside
};
static_assert(sizeof(MeshVertex) == 16 && sizeof(MeshFace) == 12, "ws_map_mesh writes 16-byte vertices and 12-byte faces");

struct SurfaceMesh
{
  std::vector<MeshVertex> vertices; // ascending cell (x, y, z), z fastest
  std::vector<MeshFace> faces;      // ascending owner voxel, then axis; the two triangles of a quad adjacent
};

// A triangle mesh of `which` by naive surface nets (the rules: warpsense_hip.h at ws_map_mesh) inside the inclusive world-voxel box
// [lo, hi] (both nullptr: the whole window).  any_weight: voxels with a negative weight count as observed (WS_MESH_ANY_WEIGHT).
inline SurfaceMesh local_map_mesh(cuda::TSDFCuda &tsdf, int which = WS_MAP_AVG, bool any_weight = false, const rmagine::Pointi *lo = nullptr,
                                  const rmagine::Pointi *hi = nullptr)
{
  SurfaceMesh out;
  size_t nv = 0, nf = 0;
  WS_CHECK(ws_map_mesh(tsdf.handle(), which, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, any_weight ? WS_MESH_ANY_WEIGHT : WS_MESH_DEFAULT, &nv, &nf));
  out.vertices.resize(nv);
  out.faces.resize(nf);
  size_t gv = 0, gf = 0;
  WS_CHECK(ws_map_mesh_download(tsdf.handle(), nv ? out.vertices.data() : nullptr, nf ? &out.faces.data()->v[0] : nullptr, nv, nf, &gv, &gf));
  return out;
}

// The mesh of the global map in device memory (the rules: warpsense_hip.h at ws_store_mesh): everything the store's chunks hold inside
// the inclusive world-voxel box [lo, hi] (both nullptr: the bounding box of the present chunks), in the order of local_map_mesh across
// chunk borders.  resolution: the map's, mm per voxel.  (app.hpp adds the overload that takes a DeviceGlobalMap.)
inline SurfaceMesh global_map_mesh(ws_store *store, int resolution, bool any_weight = false, const rmagine::Pointi *lo = nullptr,
                                   const rmagine::Pointi *hi = nullptr)
{
  SurfaceMesh out;
  size_t nv = 0, nf = 0;
  WS_CHECK(ws_store_mesh(store, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, resolution, any_weight ? WS_MESH_ANY_WEIGHT : WS_MESH_DEFAULT, &nv, &nf));
  out.vertices.resize(nv);
  out.faces.resize(nf);
  size_t gv = 0, gf = 0;
  WS_CHECK(ws_store_mesh_download(store, nv ? out.vertices.data() : nullptr, nf ? &out.faces.data()->v[0] : nullptr, nv, nf, &gv, &gf));
  return out;
}

struct RayHit // one record of ws_map_raycast
{
  int32_t x_mm, y_mm, z_mm; // the hit point in the map frame; 0, 0, 0 without a hit
  int32_t range_mm;         // along the ray; -1 without a hit
};
static_assert(sizeof(RayHit) == 16, "ws_map_raycast writes 16-byte records");

struct RayCast
{
  std::vector<RayHit> records;          // in ray order
  std::vector<rmagine::Pointi> gradient; // with_gradient: value(g + e_k) - value(g - e_k) at the hit, towards the outside; else empty
  size_t hits = 0;                      // records with range_mm >= 0
};

// The ray cast of `which` from origin_mm (the rules: warpsense_hip.h at ws_map_raycast): one ray per element of `dirs`, integer
// directions of any length, or -- targets -- map-frame points in millimetres the rays run towards.  any_weight: voxels with a
// negative weight count as observed (WS_RAYCAST_ANY_WEIGHT).
inline RayCast local_map_raycast(cuda::TSDFCuda &tsdf, const rmagine::Pointi &origin_mm, const std::vector<rmagine::Pointi> &dirs, int32_t max_range_mm,
                                 bool with_gradient = false, bool any_weight = false, bool targets = false, int which = WS_MAP_AVG)
{
  RayCast out;
  const uint32_t flags = (any_weight ? WS_RAYCAST_ANY_WEIGHT : 0u) | (with_gradient ? WS_RAYCAST_GRADIENT : 0u) | (targets ? WS_RAYCAST_TARGETS : 0u);
  WS_CHECK(ws_map_raycast(tsdf.handle(), which, &origin_mm.x, dirs.empty() ? nullptr : &dirs.data()->x, dirs.size(), max_range_mm, flags, &out.hits));
  out.records.resize(dirs.size());
  if (with_gradient) out.gradient.resize(dirs.size());
  size_t got = 0;
  WS_CHECK(ws_map_raycast_download(tsdf.handle(), dirs.empty() ? nullptr : out.records.data(), with_gradient && !dirs.empty() ? &out.gradient.data()->x : nullptr,
                                   dirs.size(), &got));
  return out;
}

// The ray cast of the global map in device memory (the rules: warpsense_hip.h at ws_store_raycast): ws_map_raycast's records through
// everything the store's chunks hold inside the inclusive world-voxel box [lo, hi] (both nullptr: everything), from an origin that
// need not lie in any window.  resolution: the map's, in mm per voxel.
inline RayCast global_map_raycast(ws_store *store, int resolution, const rmagine::Pointi &origin_mm, const std::vector<rmagine::Pointi> &dirs, int32_t max_range_mm,
                                  bool any_weight = false, bool with_gradient = false, const rmagine::Pointi *lo = nullptr, const rmagine::Pointi *hi = nullptr,
                                  bool targets = false)
{
  RayCast out;
  const uint32_t flags = (any_weight ? WS_RAYCAST_ANY_WEIGHT : 0u) | (with_gradient ? WS_RAYCAST_GRADIENT : 0u) | (targets ? WS_RAYCAST_TARGETS : 0u);
  WS_CHECK(ws_store_raycast(store, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, &origin_mm.x, dirs.empty() ? nullptr : &dirs.data()->x, dirs.size(), max_range_mm,
                            resolution, flags, &out.hits));
  out.records.resize(dirs.size());
  if (with_gradient) out.gradient.resize(dirs.size());
  size_t got = 0;
  WS_CHECK(ws_store_raycast_download(store, dirs.empty() ? nullptr : out.records.data(), with_gradient && !dirs.empty() ? &out.gradient.data()->x : nullptr,
                                     dirs.size(), &got));
  return out;
}

struct SampleRecord // one record of ws_map_sample
{
  int32_t d_mm;   // floor(T(p) / res^3); 0 where the cell is not valid
  int32_t weight; // the smallest corner weight of the cell; 0 where it is not valid
  uint32_t cls;   // WS_SAMPLE_UNKNOWN, _FREE, _SURFACE, _INSIDE
  uint32_t raw;   // the packed entry of the nearest voxel; 0 where the field has none
};
static_assert(sizeof(SampleRecord) == 16, "ws_map_sample writes 16-byte records");

struct PointSample
{
  std::vector<SampleRecord> records;      // in input order
  std::vector<rmagine::Pointi> gradient;  // with_gradient: value(g + e_k) - value(g - e_k) at the nearest voxel; else empty
  std::vector<rmagine::Pointi> selected;  // the input points of the selected classes, in input order
  uint64_t counts[4] = {0, 0, 0, 0};      // points per class
};

namespace detail
{
// select: bit c set selects class c (WS_SAMPLE_UNKNOWN .. WS_SAMPLE_INSIDE)
inline uint32_t sample_flags(bool any_weight, bool with_gradient, uint32_t select)
{
  return (any_weight ? WS_SAMPLE_ANY_WEIGHT : 0u) | (with_gradient ? WS_SAMPLE_GRADIENT : 0u) | ((select & 15u) * WS_SAMPLE_SELECT_UNKNOWN);
}
inline void sample_room(PointSample &out, size_t n, bool with_gradient, uint32_t select)
{
  out.records.resize(n);
  if (with_gradient) out.gradient.resize(n);
  size_t n_sel = 0;
  for (int c = 0; c < 4; ++c)
    if ((select >> c) & 1u) n_sel += (size_t)out.counts[c];
  out.selected.resize(n_sel);
}
} // namespace detail

// What map `which` says at map-frame points in millimetres (the rules: warpsense_hip.h at ws_map_sample).  band_mm <= 0: the map's
// tau.  select: bit c set selects class c; the input points of the selected classes come back in input order.
inline PointSample local_map_sample(cuda::TSDFCuda &tsdf, const std::vector<rmagine::Pointi> &points, int32_t band_mm = 0, bool any_weight = false,
                                    bool with_gradient = false, uint32_t select = 0, int which = WS_MAP_AVG)
{
  PointSample out;
  WS_CHECK(ws_map_sample(tsdf.handle(), which, points.empty() ? nullptr : &points.data()->x, points.size(), band_mm,
                         detail::sample_flags(any_weight, with_gradient, select), out.counts));
  detail::sample_room(out, points.size(), with_gradient, select);
  size_t got = 0, got_sel = 0;
  WS_CHECK(ws_map_sample_download(tsdf.handle(), out.records.data(), out.gradient.empty() ? nullptr : &out.gradient.data()->x,
                                  out.selected.empty() ? nullptr : &out.selected.data()->x, points.size(), out.selected.size(), &got, &got_sel));
  return out;
}

// The same of the global map in device memory (the rules: warpsense_hip.h at ws_store_sample), through everything the store's chunks
// hold inside the inclusive world-voxel box [lo, hi] (both nullptr: everything).  resolution: the map's, in mm per voxel; band_mm > 0.
inline PointSample global_map_sample(ws_store *store, int resolution, const std::vector<rmagine::Pointi> &points, int32_t band_mm, bool any_weight = false,
                                     bool with_gradient = false, uint32_t select = 0, const rmagine::Pointi *lo = nullptr, const rmagine::Pointi *hi = nullptr)
{
  PointSample out;
  WS_CHECK(ws_store_sample(store, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, points.empty() ? nullptr : &points.data()->x, points.size(), band_mm, resolution,
                           detail::sample_flags(any_weight, with_gradient, select), out.counts));
  detail::sample_room(out, points.size(), with_gradient, select);
  size_t got = 0, got_sel = 0;
  WS_CHECK(ws_store_sample_download(store, out.records.data(), out.gradient.empty() ? nullptr : &out.gradient.data()->x,
                                    out.selected.empty() ? nullptr : &out.selected.data()->x, points.size(), out.selected.size(), &got, &got_sel));
  return out;
}

struct DistanceField
{
  int32_t extent[3] = {0, 0, 0};  // nx, ny, nz of the box (nz = 1 for a column field)
  std::vector<uint32_t> records;  // x major, z fastest (columns: y fastest): bits 0..23 d2 in voxels, bits 30..31 the class
  size_t sites = 0;               // site voxels / site columns
  static uint32_t d2(uint32_t rec) { return rec & 0xffffffu; }
  static uint32_t cls(uint32_t rec) { return rec >> 30; } // 2 occupied, 1 free, 0 unknown
};

// The distance field of `which` (the rules: warpsense_hip.h at ws_map_distance) inside the inclusive world-voxel box [lo, hi] (both
// nullptr: the whole window): per voxel the squared distance in voxels to the nearest occupied voxel of the box, clamped at
// max_dist_vox squared.  unknown_occupied: never observed voxels are obstacles too; columns: the 2-D field over the (x, y) columns;
// any_weight: voxels with a negative weight count as observed (WS_DISTANCE_ANY_WEIGHT).
inline DistanceField local_map_distance(cuda::TSDFCuda &tsdf, int32_t max_dist_vox, bool unknown_occupied = false, bool columns = false,
                                        bool any_weight = false, const rmagine::Pointi *lo = nullptr, const rmagine::Pointi *hi = nullptr,
                                        int which = WS_MAP_AVG)
{
  DistanceField out;
  const uint32_t flags = (any_weight ? WS_DISTANCE_ANY_WEIGHT : 0u) | (unknown_occupied ? WS_DISTANCE_UNKNOWN_OCCUPIED : 0u) | (columns ? WS_DISTANCE_COLUMNS : 0u);
  WS_CHECK(ws_map_distance(tsdf.handle(), which, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, max_dist_vox, flags, &out.sites));
  if (lo)
  {
    const int32_t *a = &lo->x, *b = &hi->x;
    for (int k = 0; k < 3; ++k) out.extent[k] = b[k] - a[k] + 1;
  }
  else
    WS_CHECK(ws_map_get_params(tsdf.handle(), which, out.extent, nullptr, nullptr));
  if (columns) out.extent[2] = 1;
  size_t n = 0;
  WS_CHECK(ws_map_distance_download(tsdf.handle(), nullptr, 0, &n));
  out.records.resize(n);
  WS_CHECK(ws_map_distance_download(tsdf.handle(), n ? out.records.data() : nullptr, n, &n));
  return out;
}

// The distance field of the global map in device memory (the rules: warpsense_hip.h at ws_store_distance): ws_map_distance's records
// over everything the store's chunks hold inside the inclusive world-voxel box [lo, hi] (both nullptr: the bounding box of the present
// chunks), which need not lie in any window.  Voxels of absent chunks are unknown.  The result is dense: 8 bytes of device memory per
// record of the box.  (app.hpp adds DeviceGlobalMap::distance.)
inline DistanceField global_map_distance(ws_store *store, int32_t max_dist_vox, bool unknown_occupied = false, bool columns = false, bool any_weight = false,
                                         const rmagine::Pointi *lo = nullptr, const rmagine::Pointi *hi = nullptr)
{
  DistanceField out;
  const uint32_t flags = (any_weight ? WS_DISTANCE_ANY_WEIGHT : 0u) | (unknown_occupied ? WS_DISTANCE_UNKNOWN_OCCUPIED : 0u) | (columns ? WS_DISTANCE_COLUMNS : 0u);
  if (lo && hi)
  {
    const int32_t *a = &lo->x, *b = &hi->x;
    for (int k = 0; k < 3; ++k) out.extent[k] = (int32_t)((int64_t)b[k] - (int64_t)a[k] + 1); // (a 3-D extent fits: the records are counted in 32 bits)
  }
  else if (!lo && !hi)
  {
    size_t nk = 0;
    WS_CHECK(ws_store_keys(store, nullptr, 0, &nk));
    std::vector<int32_t> keys(3 * nk);
    WS_CHECK(ws_store_keys(store, keys.data(), nk, &nk));
    for (int k = 0; k < 3 && nk; ++k)
    {
      int32_t kmin = keys[k], kmax = keys[k];
      for (size_t i = 1; i < nk; ++i) kmin = std::min(kmin, keys[3 * i + k]), kmax = std::max(kmax, keys[3 * i + k]);
      out.extent[k] = (int32_t)(((int64_t)kmax - (int64_t)kmin + 1) * 64);
    }
  }
  WS_CHECK(ws_store_distance(store, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, max_dist_vox, flags, &out.sites));
  if (columns) out.extent[2] = 1;
  size_t n = 0;
  WS_CHECK(ws_store_distance_download(store, nullptr, 0, &n));
  out.records.resize(n);
  WS_CHECK(ws_store_distance_download(store, n ? out.records.data() : nullptr, n, &n));
  return out;
}

struct GroundLayer
{
  struct Record
  {
    int32_t z;  // the level's voxel (0 without a level)
    uint32_t w; // bits 0..7 frac, bits 8..23 step, bits 30..31 the column's class
  };
  int32_t lo[3] = {0, 0, 0};     // the box's first world voxel
  uint32_t extent[3] = {0, 0, 0}; // nx, ny, nz of the box
  std::vector<Record> records;    // nx ny columns, x major, y fastest
  uint64_t counts[4] = {0, 0, 0, 0}; // columns per class: unknown, ground, blocked, void
  static uint32_t cls(const Record &r) { return r.w >> 30; }
  static uint32_t frac(const Record &r) { return r.w & 0xffu; }
  static uint32_t step_q8(const Record &r) { return (r.w >> 8) & 0xffffu; }
  static int64_t height_q8(const Record &r) { return (int64_t)r.z * 256 + (int64_t)(r.w & 0xffu); }
  static double height_mm(const Record &r, int resolution) { return (double)height_q8(r) * ((double)resolution / 256.0); }
};

namespace detail
{
inline uint32_t ground_flags(bool any_weight, bool unknown_headroom, bool top)
{
  return (any_weight ? WS_GROUND_ANY_WEIGHT : 0u) | (unknown_headroom ? WS_GROUND_UNKNOWN_HEADROOM : 0u) | (top ? WS_GROUND_TOP : 0u);
}
} // namespace detail

// The ground layer of `which` (the rules: warpsense_hip.h at ws_map_ground) inside the inclusive world-voxel box [lo, hi] (both nullptr:
// the whole window): per column the lowest (top: the highest) occupied voxel under a free one with clear_vox (1 .. 64) voxels of
// headroom, its sub-voxel height and the largest height step to the neighbouring ground columns.
inline GroundLayer local_map_ground(cuda::TSDFCuda &tsdf, int32_t clear_vox, bool any_weight = false, bool unknown_headroom = false, bool top = false,
                                    const rmagine::Pointi *lo = nullptr, const rmagine::Pointi *hi = nullptr, int which = WS_MAP_AVG)
{
  GroundLayer out;
  WS_CHECK(ws_map_ground(tsdf.handle(), which, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, clear_vox, detail::ground_flags(any_weight, unknown_headroom, top), out.counts));
  WS_CHECK(ws_map_ground_box(tsdf.handle(), out.lo, out.extent));
  size_t n = 0;
  WS_CHECK(ws_map_ground_download(tsdf.handle(), nullptr, 0, &n));
  out.records.resize(n);
  WS_CHECK(ws_map_ground_download(tsdf.handle(), n ? out.records.data() : nullptr, n, &n));
  return out;
}

// The column distance field over the last local_map_ground of the map (ws_map_ground_distance): it replaces the map's distance
// result, and local_map_reach then plans over it.  max_step_q8: the largest step of a free column in 1/256 voxel.
inline DistanceField local_map_ground_distance(cuda::TSDFCuda &tsdf, int32_t max_step_q8, int32_t max_dist_vox, bool unknown_occupied = false)
{
  DistanceField out;
  uint32_t ext[3] = {0, 0, 0};
  WS_CHECK(ws_map_ground_distance(tsdf.handle(), max_step_q8, max_dist_vox, unknown_occupied ? WS_DISTANCE_UNKNOWN_OCCUPIED : 0u, &out.sites));
  WS_CHECK(ws_map_ground_box(tsdf.handle(), nullptr, ext));
  out.extent[0] = (int32_t)ext[0], out.extent[1] = (int32_t)ext[1], out.extent[2] = 1;
  size_t n = 0;
  WS_CHECK(ws_map_distance_download(tsdf.handle(), nullptr, 0, &n));
  out.records.resize(n);
  WS_CHECK(ws_map_distance_download(tsdf.handle(), n ? out.records.data() : nullptr, n, &n));
  return out;
}

// The same two over the global map in device memory (ws_store_ground, ws_store_ground_distance): the box need not lie in any window
// (both nullptr: the bounding box of the present chunks); voxels of absent chunks are unknown.  (app.hpp adds DeviceGlobalMap::ground.)
inline GroundLayer global_map_ground(ws_store *store, int32_t clear_vox, bool any_weight = false, bool unknown_headroom = false, bool top = false,
                                     const rmagine::Pointi *lo = nullptr, const rmagine::Pointi *hi = nullptr)
{
  GroundLayer out;
  WS_CHECK(ws_store_ground(store, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, clear_vox, detail::ground_flags(any_weight, unknown_headroom, top), out.counts));
  WS_CHECK(ws_store_ground_box(store, out.lo, out.extent));
  size_t n = 0;
  WS_CHECK(ws_store_ground_download(store, nullptr, 0, &n));
  out.records.resize(n);
  WS_CHECK(ws_store_ground_download(store, n ? out.records.data() : nullptr, n, &n));
  return out;
}

inline DistanceField global_map_ground_distance(ws_store *store, int32_t max_step_q8, int32_t max_dist_vox, bool unknown_occupied = false)
{
  DistanceField out;
  uint32_t ext[3] = {0, 0, 0};
  WS_CHECK(ws_store_ground_distance(store, max_step_q8, max_dist_vox, unknown_occupied ? WS_DISTANCE_UNKNOWN_OCCUPIED : 0u, &out.sites));
  WS_CHECK(ws_store_ground_box(store, nullptr, ext));
  out.extent[0] = (int32_t)ext[0], out.extent[1] = (int32_t)ext[1], out.extent[2] = 1;
  size_t n = 0;
  WS_CHECK(ws_store_distance_download(store, nullptr, 0, &n));
  out.records.resize(n);
  WS_CHECK(ws_store_distance_download(store, n ? out.records.data() : nullptr, n, &n));
  return out;
}

// publish_local_map_skeleton (map.h:175-227): the line list of the window's edges, 12 lines = 24 end points in the reference's
// order, in metres truncated to integers exactly as written there (`int *= float`: the corner in voxels goes to float, is
// multiplied by (float)map_resolution / 1000.f and truncated toward zero; map.h:182-185).
inline std::vector<std::array<double, 3>> local_map_skeleton(const int size[3], const int pos[3], int map_resolution)
{
  const float metres_per_voxel = (float)map_resolution / 1000.f;
  int top_left[3], bottom_right[3], dims[3];
  for (int k = 0; k < 3; ++k)
  {
    // the compound assignment of the reference spelled out: int -> float, one float product, truncation toward zero
    bottom_right[k] = (int)((float)(pos[k] - size[k] / 2) * metres_per_voxel);
    top_left[k] = (int)((float)(pos[k] + size[k] / 2) * metres_per_voxel);
    dims[k] = top_left[k] - bottom_right[k];
  }
  std::vector<std::array<double, 3>> pts;
  pts.reserve(24);
  auto line = [&pts](const std::array<double, 3> &from, const std::array<double, 3> &to) {
    pts.push_back(from);
    pts.push_back(to);
  };
  auto rectangle = [&](int z_offset) { // draw_rectangle, map.h:150-173
    std::array<double, 3> bbr = {(double)bottom_right[0], (double)bottom_right[1], (double)(bottom_right[2] + z_offset)};
    std::array<double, 3> btr = bbr;
    btr[0] += dims[0];
    line(bbr, btr);
    std::array<double, 3> btl = btr;
    btl[1] += dims[1];
    line(btr, btl);
    std::array<double, 3> bbl = btl;
    bbl[0] -= dims[0];
    line(btl, bbl);
    line(bbl, bbr);
  };
  auto ipt = [](int x, int y, int z) { return std::array<double, 3>{(double)x, (double)y, (double)z}; };
  rectangle(0);       // map.h:192
  rectangle(dims[2]); // map.h:193
  line(ipt(top_left[0], top_left[1], top_left[2]), ipt(top_left[0], top_left[1], top_left[2] - dims[2]));                             // :195-199
  line(ipt(bottom_right[0], bottom_right[1], bottom_right[2]), ipt(bottom_right[0], bottom_right[1], bottom_right[2] + dims[2]));       // :201-205
  line(ipt(top_left[0] - dims[0], top_left[1], top_left[2]), ipt(top_left[0] - dims[0], top_left[1], top_left[2] - dims[2]));           // :207-216
  line(ipt(bottom_right[0] + dims[0], bottom_right[1], bottom_right[2]), ipt(bottom_right[0] + dims[0], bottom_right[1], bottom_right[2] + dims[2])); // :218-227
  return pts;
}

} // namespace warpsense
