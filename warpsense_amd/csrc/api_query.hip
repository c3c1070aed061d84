// api_query.hip — the queries of a map's window: surface cloud, mesh, ray cast, point sample and distance field (ws_map_surface, ws_map_mesh,
// ws_map_raycast, ws_map_sample, ws_map_distance and what goes with each), ground, frontier, reach, view gain and clearance, and the parts
// of the query cores of ws_api.h that are no templates.
#include <algorithm>

#include "ws_api.h"
#include "ws_clearance.h"

using namespace ws;

// ---- surface cloud: publish_local_map's extraction (visualization/map.h:14-121) on the device, map_surface.hip
int ws_map_surface(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], int32_t band, uint32_t flags, size_t *n_out)
{
  if (!m || (which != WS_MAP_AVG && which != WS_MAP_NEW) || (flags & ~WS_SURFACE_MARKER) || ((lo == nullptr) != (hi == nullptr)))
    return invalid("ws_map_surface: bad argument");
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->surf.mu);
  ws_map::Surface &q = m->surf;
  WS_TRY(q.timer.arm());
  int32_t l[3], ext[3];
  WS_TRY(resolve_box(m, which, lo, hi, true, "ws_map_surface", l, ext));
  if (band <= 0) band = m->tau;
  const size_t n_cols = (size_t)ext[0] * (size_t)ext[1]; // n_cols < 2^31 (ws_map_create)
  WS_TRY(surface_run(
      q, m->ctx->stream, surface_blocks_for((int64_t)n_cols), (flags & WS_SURFACE_MARKER) != 0, n_out, n_cols > q.col_cnt.cap,
      [&] { return q.col_cnt.grow(n_cols, sizeof(uint32_t)); }, [&] { return launch_surface_count(m, which, l, ext, band); },
      [&](size_t cap) { return launch_surface_emit(m, which, l, ext, band, (flags & WS_SURFACE_MARKER) != 0, cap); }));
  return map_take_error(m);
}

// ---- surface cloud: what the host core of ws_api.h (surface_run) needs beside it, for the window of a map here and for the chunks of
// the store in api_store_query.hip
const void *ws::surface_records_dev(const SurfResult *q, size_t *n)
{
  if (n) *n = q ? q->n : 0;
  return q && q->n ? q->rec.p : nullptr;
}

const float *ws::surface_marker_dev(const SurfResult *q, size_t *n)
{
  const bool have = q && q->has_marker && q->n;
  if (n) *n = have ? q->n : 0;
  return have ? static_cast<const float *>(q->marker.p) : nullptr;
}

// `name`, `call`: the download entry point, and the entry point whose flag it misses
int ws::surface_download(const SurfResult &q, hipStream_t s, const char *name, const char *call, void *records_host, float *marker_host, size_t capacity_points,
                         size_t *n_out)
{
  *n_out = q.n;
  const size_t k = std::min(capacity_points, q.n);
  if (k == 0) return WS_OK;
  if (marker_host && !q.has_marker) return invalid(std::string(name) + ": the last " + call + " did not ask for WS_SURFACE_MARKER");
  if (records_host) WS_HIP(hipMemcpyAsync(records_host, q.rec.p, k * 16, hipMemcpyDeviceToHost, s));
  if (marker_host) WS_HIP(hipMemcpyAsync(marker_host, q.marker.p, k * 7 * sizeof(float), hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

const void *ws_map_surface_records_dev(const ws_map *m, size_t *n) { return surface_records_dev(m ? &m->surf : nullptr, n); }

const float *ws_map_surface_marker_dev(const ws_map *m, size_t *n) { return surface_marker_dev(m ? &m->surf : nullptr, n); }

int ws_map_surface_download(ws_map *m, void *records_host, float *marker_host, size_t capacity_points, size_t *n_out)
{
  if (!m || !n_out) return invalid("ws_map_surface_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->surf.mu);
  return surface_download(m->surf, m->ctx->stream, "ws_map_surface_download", "ws_map_surface", records_host, marker_host, capacity_points, n_out);
}

// ws_debug_*_timing: the times of the last call between the event pairs of `pairs`, then the switch
int ws::query_timing(hipStream_t s, QueryTimer &t, int32_t enable, float *ms_out, const int (*pairs)[2], int n)
{
  const int rc = t.read(ms_out, pairs, n, s);
  if (rc == WS_OK) t.set(enable);
  return rc;
}

int ws_debug_surface_timing(ws_map *m, int32_t enable, float ms_out[3])
{
  if (!m) return invalid("ws_debug_surface_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->surf.mu);
  return query_timing(m->ctx->stream, m->surf.timer, enable, ms_out, SURF_PAIRS, 3);
}

// ---- mesh and ray cast: what the host cores of ws_api.h (mesh_run, raycast_check, raycast_run) need beside them, for the window of
// a map here and for the chunks of the store in api_store_query.hip
int ws::mesh_corners_fit(const int32_t lo[3], const int32_t hi[3], int32_t res, const char *name)
{
  for (int k = 0; k < 3; ++k)
    for (int64_t c : {(int64_t)lo[k], (int64_t)hi[k]})
      if (((c < 0 ? -c : c) + 1) * (int64_t)res > (int64_t)INT32_MAX) return range_error(name, ": a box corner in millimetres does not fit int32");
  return WS_OK;
}

int ws::mesh_publish(MeshResult &q, size_t nv, size_t nf, size_t *n_vertices, size_t *n_faces)
{
  q.nv = nv, q.nf = nf;
  if (n_vertices) *n_vertices = nv;
  if (n_faces) *n_faces = nf;
  return WS_OK;
}

const void *ws::mesh_vertices_dev(const MeshResult *q, size_t *n)
{
  if (n) *n = q ? q->nv : 0;
  return q && q->nv ? q->vert.p : nullptr;
}

const uint32_t *ws::mesh_faces_dev(const MeshResult *q, size_t *n)
{
  if (n) *n = q ? q->nf : 0;
  return q && q->nf ? static_cast<const uint32_t *>(q->face.p) : nullptr;
}

int ws::mesh_download(const MeshResult &q, hipStream_t s, void *vertices_host, uint32_t *faces_host, size_t cap_vertices, size_t cap_faces, size_t *n_vertices,
                      size_t *n_faces)
{
  *n_vertices = q.nv;
  *n_faces = q.nf;
  const size_t kv = vertices_host ? std::min(cap_vertices, q.nv) : 0, kf = faces_host ? std::min(cap_faces, q.nf) : 0;
  if (kv) WS_HIP(hipMemcpyAsync(vertices_host, q.vert.p, kv * 16, hipMemcpyDeviceToHost, s));
  if (kf) WS_HIP(hipMemcpyAsync(faces_host, q.face.p, kf * 12, hipMemcpyDeviceToHost, s));
  if (kv || kf) WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

const void *ws::raycast_records_dev(const RayResult *q, size_t *n)
{
  if (n) *n = q ? q->n : 0;
  return q && q->n ? q->rec.p : nullptr;
}

const int32_t *ws::raycast_gradient_dev(const RayResult *q, size_t *n)
{
  const bool have = q && q->has_grad && q->n;
  if (n) *n = have ? q->n : 0;
  return have ? static_cast<const int32_t *>(q->grad.p) : nullptr;
}

// `name`, `call`: the download entry point, and the entry point whose flag it misses
int ws::raycast_download(const RayResult &q, hipStream_t s, const char *name, const char *call, void *records_host, int32_t *gradient_host, size_t capacity_rays,
                         size_t *n_out)
{
  *n_out = q.n;
  const size_t k = std::min(capacity_rays, q.n);
  if (k == 0) return WS_OK;
  if (gradient_host && !q.has_grad) return invalid(std::string(name) + ": the last " + call + " did not ask for WS_RAYCAST_GRADIENT");
  if (records_host) WS_HIP(hipMemcpyAsync(records_host, q.rec.p, k * 16, hipMemcpyDeviceToHost, s));
  if (gradient_host) WS_HIP(hipMemcpyAsync(gradient_host, q.grad.p, k * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

// ---- mesh: naive surface nets over a device map, map_mesh.hip (the rules are stated in warpsense_hip.h)
int ws_map_mesh(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], uint32_t flags, size_t *n_vertices, size_t *n_faces)
{
  if (!m || (which != WS_MAP_AVG && which != WS_MAP_NEW) || (flags & ~WS_MESH_ANY_WEIGHT) || ((lo == nullptr) != (hi == nullptr)))
    return invalid("ws_map_mesh: bad argument");
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->mesh.mu);
  MeshResult &q = m->mesh;
  WS_TRY(q.timer.arm());
  int32_t l[3], ext[3];
  WS_TRY(resolve_box(m, which, lo, hi, true, "ws_map_mesh", l, ext));
  const int32_t h[3] = {l[0] + (ext[0] - 1), l[1] + (ext[1] - 1), l[2] + (ext[2] - 1)}; // (a voxel of the window)
  WS_TRY(mesh_corners_fit(l, h, m->res, "ws_map_mesh"));
  mesh_publish(q, 0, 0, n_vertices, n_faces);
  const uint64_t n_words = (uint64_t)ext[0] * (uint64_t)ext[1] * (uint64_t)((ext[2] + 63) / 64);
  if (n_words >= (1ull << 31)) return range_error("ws_map_mesh", ": box too large (columns x 64-voxel words must stay below 2^31)");
  if (ext[0] < 2 || ext[1] < 2 || ext[2] < 2) return map_take_error(m); // one voxel thick along an axis: no cells
  WS_TRY(mesh_run(
      q, m->ctx->stream, "ws_map_mesh", n_words, n_vertices, n_faces, [&] { return launch_mesh_count(m, q, which, l, ext, flags); },
      [&] { return launch_mesh_emit(m, q, which, l, ext, flags); }));
  return map_take_error(m);
}

const void *ws_map_mesh_vertices_dev(const ws_map *m, size_t *n) { return mesh_vertices_dev(m ? &m->mesh : nullptr, n); }

const uint32_t *ws_map_mesh_faces_dev(const ws_map *m, size_t *n) { return mesh_faces_dev(m ? &m->mesh : nullptr, n); }

int ws_map_mesh_download(ws_map *m, void *vertices_host, uint32_t *faces_host, size_t cap_vertices, size_t cap_faces, size_t *n_vertices, size_t *n_faces)
{
  if (!m || !n_vertices || !n_faces) return invalid("ws_map_mesh_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->mesh.mu);
  return mesh_download(m->mesh, m->ctx->stream, vertices_host, faces_host, cap_vertices, cap_faces, n_vertices, n_faces);
}

int ws_debug_mesh_timing(ws_map *m, int32_t enable, float ms_out[3])
{
  if (!m) return invalid("ws_debug_mesh_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->mesh.mu);
  return query_timing(m->ctx->stream, m->mesh.timer, enable, ms_out, MESH_PAIRS, 3);
}

// ---- ray cast: the range image of a device map, map_raycast.hip (the rules are stated in warpsense_hip.h)
static int map_raycast(ws_map *m, int which, const int32_t origin[3], const int32_t *dirs, bool dirs_on_host, size_t n, int32_t max_range, uint32_t flags,
                       size_t *n_hits)
{
  WS_TRY(raycast_check("ws_map_raycast", !m || (which != WS_MAP_AVG && which != WS_MAP_NEW), origin, dirs, n, max_range, m ? m->res : 0, flags,
                       [] { return WS_OK; }));
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->ray.mu);
  RayResult &q = m->ray;
  WS_TRY(raycast_run(
      q, m->ctx->stream, dirs, dirs_on_host, n, flags, n_hits, false, [] { return WS_OK; },
      [&](const int32_t *dirs_dev) { return launch_raycast(m, q, which, origin, dirs_dev, n, max_range, flags); }));
  return map_take_error(m);
}

int ws_map_raycast(ws_map *m, int which, const int32_t origin_mm[3], const int32_t *dirs_host, size_t n, int32_t max_range_mm, uint32_t flags, size_t *n_hits)
{
  return map_raycast(m, which, origin_mm, dirs_host, true, n, max_range_mm, flags, n_hits);
}

int ws_map_raycast_dev(ws_map *m, int which, const int32_t origin_mm[3], const int32_t *dirs_dev, size_t n, int32_t max_range_mm, uint32_t flags, size_t *n_hits)
{
  return map_raycast(m, which, origin_mm, dirs_dev, false, n, max_range_mm, flags, n_hits);
}

const void *ws_map_raycast_records_dev(const ws_map *m, size_t *n) { return raycast_records_dev(m ? &m->ray : nullptr, n); }

const int32_t *ws_map_raycast_gradient_dev(const ws_map *m, size_t *n) { return raycast_gradient_dev(m ? &m->ray : nullptr, n); }

int ws_map_raycast_download(ws_map *m, void *records_host, int32_t *gradient_host, size_t capacity_rays, size_t *n_out)
{
  if (!m || !n_out) return invalid("ws_map_raycast_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->ray.mu);
  return raycast_download(m->ray, m->ctx->stream, "ws_map_raycast_download", "ws_map_raycast", records_host, gradient_host, capacity_rays, n_out);
}

int ws_debug_raycast_timing(ws_map *m, int32_t enable, float ms_out[3])
{
  if (!m) return invalid("ws_debug_raycast_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->ray.mu);
  return query_timing(m->ctx->stream, m->ray.timer, enable, ms_out, RAY_PAIRS, 3);
}

// ---- point sample: what the host cores of ws_api.h (sample_check, sample_run) need beside them, for the window of a map here and
// for the chunks of the store in api_store_query.hip
const void *ws::sample_records_dev(const SampleResult *q, size_t *n)
{
  if (n) *n = q ? q->n : 0;
  return q && q->n ? q->rec.p : nullptr;
}

const int32_t *ws::sample_gradient_dev(const SampleResult *q, size_t *n)
{
  const bool have = q && q->has_grad && q->n;
  if (n) *n = have ? q->n : 0;
  return have ? static_cast<const int32_t *>(q->grad.p) : nullptr;
}

const int32_t *ws::sample_selected_dev(const SampleResult *q, size_t *n)
{
  const bool have = q && q->has_sel && q->n_sel;
  if (n) *n = have ? q->n_sel : 0;
  return have ? static_cast<const int32_t *>(q->sel.p) : nullptr;
}

// `name`, `call`: the download entry point, and the entry point whose flag it misses
int ws::sample_download(const SampleResult &q, hipStream_t s, const char *name, const char *call, void *records_host, int32_t *gradient_host,
                        int32_t *selected_host, size_t capacity_points, size_t capacity_selected, size_t *n_out, size_t *n_selected)
{
  *n_out = q.n;
  if (n_selected) *n_selected = q.n_sel;
  const size_t k = std::min(capacity_points, q.n), ks = selected_host ? std::min(capacity_selected, q.n_sel) : 0;
  if (k && gradient_host && !q.has_grad) return invalid(std::string(name) + ": the last " + call + " did not ask for WS_SAMPLE_GRADIENT");
  if (selected_host && capacity_selected && q.n && !q.has_sel) return invalid(std::string(name) + ": the last " + call + " did not ask for a selection");
  if (k && records_host) WS_HIP(hipMemcpyAsync(records_host, q.rec.p, k * 16, hipMemcpyDeviceToHost, s));
  if (k && gradient_host) WS_HIP(hipMemcpyAsync(gradient_host, q.grad.p, k * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (ks) WS_HIP(hipMemcpyAsync(selected_host, q.sel.p, ks * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (k || ks) WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

// ---- point sample: the map's value at given points, map_sample.hip (the rules are stated in warpsense_hip.h)
static int map_sample(ws_map *m, int which, const int32_t *points, bool points_on_host, size_t n, int32_t band, uint32_t flags, uint64_t counts[4])
{
  // (the kernel forms the window's ends in int32: a window that does not lie in int32 is refused like a box query's, before anything moves)
  WS_TRY(sample_check("ws_map_sample", !m || (which != WS_MAP_AVG && which != WS_MAP_NEW), points, n, m ? m->res : 0, flags, [&] {
    int32_t l[3], ext[3];
    return resolve_box(m, which, nullptr, nullptr, true, "ws_map_sample", l, ext);
  }));
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->sample.mu);
  SampleResult &q = m->sample;
  if (band <= 0) band = m->tau;
  WS_TRY(sample_run(
      q, m->ctx->stream, points, points_on_host, n, flags, counts, false, [] { return WS_OK; },
      [&](const int32_t *pts_dev) { return launch_sample(m, q, which, pts_dev, n, band, flags); }));
  return map_take_error(m);
}

int ws_map_sample(ws_map *m, int which, const int32_t *points_host, size_t n, int32_t band_mm, uint32_t flags, uint64_t counts[4])
{
  return map_sample(m, which, points_host, true, n, band_mm, flags, counts);
}

int ws_map_sample_dev(ws_map *m, int which, const int32_t *points_dev, size_t n, int32_t band_mm, uint32_t flags, uint64_t counts[4])
{
  return map_sample(m, which, points_dev, false, n, band_mm, flags, counts);
}

const void *ws_map_sample_records_dev(const ws_map *m, size_t *n) { return sample_records_dev(m ? &m->sample : nullptr, n); }

const int32_t *ws_map_sample_gradient_dev(const ws_map *m, size_t *n) { return sample_gradient_dev(m ? &m->sample : nullptr, n); }

const int32_t *ws_map_sample_selected_dev(const ws_map *m, size_t *n) { return sample_selected_dev(m ? &m->sample : nullptr, n); }

int ws_map_sample_download(ws_map *m, void *records_host, int32_t *gradient_host, int32_t *selected_host, size_t capacity_points, size_t capacity_selected,
                           size_t *n_out, size_t *n_selected)
{
  if (!m || !n_out) return invalid("ws_map_sample_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->sample.mu);
  return sample_download(m->sample, m->ctx->stream, "ws_map_sample_download", "ws_map_sample", records_host, gradient_host, selected_host, capacity_points,
                         capacity_selected, n_out, n_selected);
}

int ws_debug_sample_timing(ws_map *m, int32_t enable, float ms_out[3])
{
  if (!m) return invalid("ws_debug_sample_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->sample.mu);
  return query_timing(m->ctx->stream, m->sample.timer, enable, ms_out, SAMPLE_PAIRS, 3);
}

// ---- distance field: the same beside distance_check and distance_run.  The window and the store differ in pass 0 only.
const uint32_t *ws::distance_dev(const DistResult *q, size_t *n)
{
  if (n) *n = q ? q->n : 0;
  return q && q->n ? static_cast<const uint32_t *>(q->rec.p) : nullptr;
}

int ws::distance_download(const DistResult &q, hipStream_t s, uint32_t *host, size_t capacity, size_t *n_out)
{
  *n_out = q.n;
  const size_t k = host ? std::min(capacity, q.n) : 0;
  if (k == 0) return WS_OK;
  WS_HIP(hipMemcpyAsync(host, q.rec.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

// ---- distance field: the exact Euclidean transform of a device map, map_distance.hip (the rules are stated in warpsense_hip.h)
int ws_map_distance(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], int32_t max_dist_vox, uint32_t flags, size_t *n_sites)
{
  std::unique_lock<std::mutex> lock;
  int32_t l[3], ext[3];
  uint32_t e32[3];
  size_t n = 0;
  WS_TRY(distance_check(
      "ws_map_distance", !m || (which != WS_MAP_AVG && which != WS_MAP_NEW), lo, hi, max_dist_vox, flags,
      [&](uint64_t e[3]) {
        WS_SETTLE(m);
        lock = std::unique_lock<std::mutex>(m->dist.mu);
        WS_TRY(m->dist.timer.arm());
        WS_TRY(resolve_box(m, which, lo, hi, true, "ws_map_distance", l, ext)); // ext[0] ext[1] < 2^31, ext[2] <= 2^20
        for (int k = 0; k < 3; ++k) e[k] = (uint64_t)ext[k];
        return (int)WS_OK;
      },
      e32, &n));
  DistResult &q = m->dist;
  WS_TRY(distance_run(q, m->ctx->stream, l, e32, max_dist_vox, flags, n, n_sites, [&] { return launch_dist_classify(m, q, which, l, ext, max_dist_vox, flags); }));
  return map_take_error(m);
}

const uint32_t *ws_map_distance_dev(const ws_map *m, size_t *n) { return distance_dev(m ? &m->dist : nullptr, n); }

int ws_map_distance_download(ws_map *m, uint32_t *host, size_t capacity, size_t *n_out)
{
  if (!m || !n_out) return invalid("ws_map_distance_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->dist.mu);
  return distance_download(m->dist, m->ctx->stream, host, capacity, n_out);
}

int ws_debug_distance_timing(ws_map *m, int32_t enable, float ms_out[4])
{
  if (!m) return invalid("ws_debug_distance_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->dist.mu);
  return query_timing(m->ctx->stream, m->dist.timer, enable, ms_out, DIST_PAIRS, 4);
}

// ---- ground: the same beside ground_check and ground_run.  The window and the store differ in pass 1 only.
const void *ws::ground_dev(const GroundResult *q, size_t *n)
{
  if (n) *n = q ? q->n : 0;
  return q && q->n ? q->rec.p : nullptr;
}

int ws::ground_download(const GroundResult &q, hipStream_t s, void *host, size_t capacity, size_t *n_out)
{
  *n_out = q.n;
  const size_t k = host ? std::min(capacity, q.n) : 0;
  if (k == 0) return WS_OK;
  WS_HIP(hipMemcpyAsync(host, q.rec.p, k * 8, hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

int ws::ground_box(const GroundResult &q, const char *name, int32_t lo[3], uint32_t ext[3])
{
  if (!q.have) return invalid(std::string(name) + ": no ground result yet");
  for (int k = 0; k < 3; ++k)
  {
    if (lo) lo[k] = q.lo[k];
    if (ext) ext[k] = q.ext[k];
  }
  return WS_OK;
}

// ---- ground: the elevation layer of a device map, map_ground.hip (the rules are stated in warpsense_hip.h)
int ws_map_ground(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], int32_t clear_vox, uint32_t flags, uint64_t counts[4])
{
  std::unique_lock<std::mutex> lock;
  int32_t l[3], ext[3];
  uint32_t e32[3];
  size_t n = 0;
  WS_TRY(ground_check(
      "ws_map_ground", !m || (which != WS_MAP_AVG && which != WS_MAP_NEW), lo, hi, clear_vox, flags,
      [&](uint64_t e[3]) {
        WS_SETTLE(m);
        lock = std::unique_lock<std::mutex>(m->ground.mu);
        WS_TRY(m->ground.timer.arm());
        WS_TRY(resolve_box(m, which, lo, hi, true, "ws_map_ground", l, ext)); // ext[0] ext[1] < 2^31, ext[2] <= 2^20
        for (int k = 0; k < 3; ++k) e[k] = (uint64_t)ext[k];
        return (int)WS_OK;
      },
      e32, &n));
  GroundResult &q = m->ground;
  WS_TRY(ground_run(q, m->ctx->stream, l, e32, n, counts, [&] { return launch_ground_levels(m, q, which, l, ext, clear_vox, flags); }));
  return map_take_error(m);
}

const void *ws_map_ground_dev(const ws_map *m, size_t *n) { return ground_dev(m ? &m->ground : nullptr, n); }

int ws_map_ground_download(ws_map *m, void *host, size_t capacity, size_t *n_out)
{
  if (!m || !n_out) return invalid("ws_map_ground_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->ground.mu);
  return ground_download(m->ground, m->ctx->stream, host, capacity, n_out);
}

int ws_map_ground_box(ws_map *m, int32_t lo[3], uint32_t ext[3])
{
  if (!m) return invalid("ws_map_ground_box: map is NULL");
  std::lock_guard<std::mutex> lock(m->ground.mu);
  return ground_box(m->ground, "ws_map_ground_box", lo, ext);
}

int ws_debug_ground_timing(ws_map *m, int32_t enable, float ms_out[2])
{
  if (!m) return invalid("ws_debug_ground_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->ground.mu);
  return query_timing(m->ctx->stream, m->ground.timer, enable, ms_out, GROUND_PAIRS, 2);
}

// the bridge to the planner: a column distance call whose pass 0 reads the last ground result (ground.mu, then dist.mu)
int ws_map_ground_distance(ws_map *m, int32_t max_step_q8, int32_t max_dist_vox, uint32_t flags, size_t *n_sites)
{
  std::unique_lock<std::mutex> ground_lock, lock;
  int32_t l[3] = {0, 0, 0};
  uint32_t e32[3];
  size_t n = 0;
  WS_TRY(ground_distance_check(
      "ws_map_ground_distance", !m, max_step_q8, max_dist_vox, flags,
      [&](uint64_t e[3]) {
        WS_SETTLE(m);
        ground_lock = std::unique_lock<std::mutex>(m->ground.mu);
        lock = std::unique_lock<std::mutex>(m->dist.mu);
        if (!m->ground.have) return invalid("ws_map_ground_distance: no ground result yet (the call runs on the records of the last ws_map_ground)");
        WS_TRY(m->dist.timer.arm());
        for (int k = 0; k < 3; ++k) e[k] = m->ground.n ? (uint64_t)m->ground.ext[k] : 0u, l[k] = m->ground.lo[k];
        return (int)WS_OK;
      },
      e32, &n));
  DistResult &q = m->dist;
  const uint32_t dflags = flags | WS_DISTANCE_COLUMNS;
  WS_TRY(distance_run(q, m->ctx->stream, l, e32, max_dist_vox, dflags, n, n_sites,
                      [&] { return launch_ground_sites(m->ctx->stream, m->ground, q, (uint32_t)max_step_q8, max_dist_vox, dflags); }));
  return map_take_error(m);
}

// ---- frontier: what the host core of ws_api.h (frontier_run) needs beside it, for the window of a map here and for the chunks of the
// store in api_store_query.hip
int ws::frontier_check(const char *name, bool bad, const int32_t *lo, const int32_t *hi, int32_t min_value, uint32_t flags)
{
  const uint32_t known = WS_FRONTIER_ANY_WEIGHT | WS_FRONTIER_CLUSTERS;
  if (bad || (flags & ~known) || ((lo == nullptr) != (hi == nullptr))) return invalid(std::string(name) + ": bad argument");
  if (min_value < 0 || min_value > 32767) return range_error(name, ": min_value must be 0 .. 32767 (a raw int16 value; 0: any non-negative value)");
  return WS_OK;
}

int ws::frontier_publish(FrontierResult &q, size_t n, size_t k, bool clusters, size_t *n_out, size_t *n_clusters)
{
  q.n = n, q.n_clusters = k, q.has_clusters = clusters;
  if (n_out) *n_out = n;
  if (n_clusters) *n_clusters = k;
  return WS_OK;
}

const uint32_t *ws::frontier_labels_dev(const FrontierResult *q, size_t *n)
{
  const bool have = q && q->has_clusters && q->n;
  if (n) *n = have ? q->n : 0;
  return have ? static_cast<const uint32_t *>(q->labels.p) : nullptr;
}

const void *ws::frontier_clusters_dev(const FrontierResult *q, size_t *n)
{
  const bool have = q && q->has_clusters && q->n_clusters;
  if (n) *n = have ? q->n_clusters : 0;
  return have ? q->clusters.p : nullptr;
}

// `name`, `call`: the download entry point, and the entry point whose flag it misses
int ws::frontier_download(const FrontierResult &q, hipStream_t s, const char *name, const char *call, void *records_host, uint32_t *labels_host, void *clusters_host,
                          size_t cap_records, size_t cap_clusters, size_t *n_out, size_t *n_clusters)
{
  *n_out = q.n;
  if (n_clusters) *n_clusters = q.n_clusters;
  if (q.n && !q.has_clusters && ((labels_host && cap_records) || (clusters_host && cap_clusters)))
    return invalid(std::string(name) + ": the last " + call + " did not ask for WS_FRONTIER_CLUSTERS");
  const size_t k = std::min(cap_records, q.n), kc = clusters_host ? std::min(cap_clusters, q.n_clusters) : 0;
  if (k && records_host) WS_HIP(hipMemcpyAsync(records_host, q.rec.p, k * 16, hipMemcpyDeviceToHost, s));
  if (k && labels_host) WS_HIP(hipMemcpyAsync(labels_host, q.labels.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (kc) WS_HIP(hipMemcpyAsync(clusters_host, q.clusters.p, kc * 64, hipMemcpyDeviceToHost, s));
  if (k || kc) WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

// ---- frontier: the observed-free voxels of a box that touch a never-observed one, and their clusters, map_frontier.hip (the rules are
// stated in warpsense_hip.h)
int ws_map_frontier(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], int32_t min_value, uint32_t flags, size_t *n_out, size_t *n_clusters)
{
  WS_TRY(frontier_check("ws_map_frontier", !m || (which != WS_MAP_AVG && which != WS_MAP_NEW), lo, hi, min_value, flags));
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->frontier.mu);
  ws_map::Frontier &q = m->frontier;
  int32_t l[3], ext[3];
  WS_TRY(resolve_box(m, which, lo, hi, true, "ws_map_frontier", l, ext));
  WS_TRY(q.timer.arm());
  const size_t n_cols = (size_t)ext[0] * (size_t)ext[1]; // n_cols < 2^31 (ws_map_create)
  WS_TRY(frontier_run(
      q, m->ctx->stream, "ws_map_frontier", surface_blocks_for((int64_t)n_cols), flags, n_out, n_clusters, n_cols > q.col_cnt.cap,
      [&] { return q.col_cnt.grow(n_cols, sizeof(uint32_t)); }, [&] { return launch_frontier_count(m, which, l, ext, min_value, flags); },
      [&](size_t cap) { return launch_frontier_emit(m, which, l, ext, min_value, flags, cap); }));
  return map_take_error(m);
}

const void *ws_map_frontier_records_dev(const ws_map *m, size_t *n) { return surface_records_dev(m ? &m->frontier : nullptr, n); }

const uint32_t *ws_map_frontier_labels_dev(const ws_map *m, size_t *n) { return frontier_labels_dev(m ? &m->frontier : nullptr, n); }

const void *ws_map_frontier_clusters_dev(const ws_map *m, size_t *n) { return frontier_clusters_dev(m ? &m->frontier : nullptr, n); }

int ws_map_frontier_download(ws_map *m, void *records_host, uint32_t *labels_host, void *clusters_host, size_t cap_records, size_t cap_clusters, size_t *n_out,
                             size_t *n_clusters)
{
  if (!m || !n_out) return invalid("ws_map_frontier_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->frontier.mu);
  return frontier_download(m->frontier, m->ctx->stream, "ws_map_frontier_download", "ws_map_frontier", records_host, labels_host, clusters_host, cap_records,
                           cap_clusters, n_out, n_clusters);
}

int ws_debug_frontier_timing(ws_map *m, int32_t enable, float ms_out[4])
{
  if (!m) return invalid("ws_debug_frontier_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->frontier.mu);
  return query_timing(m->ctx->stream, m->frontier.timer, enable, ms_out, FRONTIER_PAIRS, 4);
}

// ---- reach: what the host core of ws_api.h (reach_run) needs beside it, for the window of a map here and for the store in
// api_store_query.hip.  reach_rounds is the flow behind the refusals, from "the old result is dropped" to the publish: seeding, then one launch
// and one read per round until the list of the next round is empty.
int ws::reach_rounds(ReachResult &q, const DistResult &d, hipStream_t s, const char *name, const int32_t *seeds, size_t n_seeds, int32_t clear_d2, uint32_t flags,
                     uint32_t max_rounds, size_t *n_seeded, size_t *n_reached, uint32_t *rounds)
{
  const bool columns = (d.flags & WS_DISTANCE_COLUMNS) != 0;
  if (d.n > (size_t)(0xfffffffeull / 17ull)) return range_error(name, ": more than (2^32 - 2) / 17 records (a cost could overflow 32 bits)");
  WS_TRY(q.timer.arm());
  if (n_seeded) *n_seeded = 0;
  if (n_reached) *n_reached = 0;
  if (rounds) *rounds = 0;
  q.n = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  q.have = false;
  ReachBox &b = q.box;
  copy3(b.lo, d.lo);
  b.columns = columns ? 1u : 0u;
  b.e[0] = columns ? 1u : d.ext[0], b.e[1] = columns ? d.ext[0] : d.ext[1], b.e[2] = columns ? d.ext[1] : d.ext[2];
  if (d.n == 0)
  {
    b.e[0] = b.e[1] = b.e[2] = 0u;
    q.have = true;
    return WS_OK;
  }
  const size_t n = d.n, n_tiles = (size_t)reach_tiles(b);
  WS_TRY(q.words.alloc(4));
  if (n > q.cost.cap || n_tiles > q.mark.cap || 2 * n_tiles > q.list.cap || n_seeds > q.seeds.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.cost.grow(n, sizeof(uint32_t)));
    WS_TRY(q.mark.grow(n_tiles, sizeof(uint32_t)));
    WS_TRY(q.list.grow(2 * n_tiles, sizeof(uint32_t)));
    WS_TRY(q.seeds.grow(n_seeds, 3 * sizeof(int32_t)));
  }
  const uint32_t *dist = d.rec.as<uint32_t>();
  const uint64_t cap = max_rounds ? (uint64_t)max_rounds : std::min<uint64_t>((uint64_t)REACH_ROUNDS_PER_TILE * n_tiles + 64u, 0xfffffffeull);
  WS_HIP(hipMemcpyAsync(q.seeds.p, seeds, n_seeds * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  WS_TRY(launch_reach_seed(q, s, dist, n_seeds, (uint32_t)clear_d2, flags));
  WS_HIP(hipStreamSynchronize(s));
  const size_t kept = (size_t)q.words.host[0];
  uint64_t active = q.words.host[3]; // round r reads list r & 1
  uint32_t r = 0;
  q.active.clear();
  while (active)
  {
    if ((uint64_t)r >= cap)
    {
      q.timer.marked = 0; // (a call without a result leaves no times either: ws_debug_reach_timing reads zeros)
      set_error(std::string(name) + ": not converged after " + std::to_string(r) + " rounds (max_rounds); no result is left");
      return WS_ERR_RANGE;
    }
    ++r;
    q.active.push_back((uint32_t)std::min<uint64_t>(active, 0xffffffffull));
    WS_TRY(launch_reach_round(q, s, dist, r, (uint32_t)std::min<uint64_t>(active, 0xffffffffull), (uint32_t)clear_d2, flags));
    WS_HIP(hipStreamSynchronize(s)); // the one host read of a round: the length of the next list sizes the next launch
    active = q.words.host[2 + ((r + 1u) & 1u)];
  }
  WS_TRY(launch_reach_count(q, s));
  WS_HIP(hipStreamSynchronize(s));
  q.n = n;
  q.have = true;
  if (n_seeded) *n_seeded = kept;
  if (n_reached) *n_reached = (size_t)q.words.host[1];
  if (rounds) *rounds = r;
  return WS_OK;
}

const uint32_t *ws::reach_dev(const ReachResult *q, size_t *n)
{
  if (n) *n = q ? q->n : 0;
  return q && q->n ? static_cast<const uint32_t *>(q->cost.p) : nullptr;
}

int ws::reach_box(const ReachResult &q, int32_t lo[3], uint32_t ext[3], int32_t *columns)
{
  const bool have = q.have && q.n;
  for (int k = 0; k < 3; ++k)
  {
    if (lo) lo[k] = have ? q.box.lo[k] : 0;
    if (ext) ext[k] = !have ? 0u : q.box.columns ? (k < 2 ? q.box.e[k + 1] : 1u) : q.box.e[k];
  }
  if (columns) *columns = have && q.box.columns ? 1 : 0;
  return WS_OK;
}

int ws::reach_download(const ReachResult &q, hipStream_t s, uint32_t *host, size_t capacity, size_t *n_out)
{
  *n_out = q.n;
  const size_t k = host ? std::min(capacity, q.n) : 0;
  if (k == 0) return WS_OK;
  WS_HIP(hipMemcpyAsync(host, q.cost.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

int ws::reach_lookup(ReachResult &q, hipStream_t s, const char *name, const int32_t *points, bool on_host, size_t n, int32_t stride, uint32_t *cost)
{
  if ((stride != 3 && stride != 4) || (n && (!points || !cost))) return invalid(std::string(name) + ": bad argument");
  if (!q.have) return invalid(std::string(name) + ": no reach result");
  if (n > ((size_t)1 << 27)) return range_error(name, ": more than 2^27 points");
  if (n == 0) return WS_OK;
  uint32_t *out = cost;
  if (on_host)
  {
    if (n * (size_t)stride > q.pts.cap || n > q.out.cap)
    {
      WS_HIP(hipStreamSynchronize(s));
      WS_TRY(q.pts.grow(n * (size_t)stride, sizeof(int32_t)));
      WS_TRY(q.out.grow(n, sizeof(uint32_t)));
    }
    WS_HIP(hipMemcpyAsync(q.pts.p, points, n * (size_t)stride * sizeof(int32_t), hipMemcpyHostToDevice, s));
    points = q.pts.as<int32_t>();
    out = q.out.as<uint32_t>();
  }
  WS_TRY(launch_reach_lookup(q, s, points, n, stride, out));
  if (on_host) WS_HIP(hipMemcpyAsync(cost, out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

int ws::reach_paths(ReachResult &q, hipStream_t s, const char *name, const int32_t *goals_host, size_t g, uint32_t cap_steps, void *headers_host, void *records_host)
{
  if (!goals_host || !headers_host || g == 0 || g > ((size_t)1 << 20) || (cap_steps && !records_host)) return invalid(std::string(name) + ": bad argument");
  if (!q.have) return invalid(std::string(name) + ": no reach result");
  const size_t n_rec = g * (size_t)cap_steps;
  if (n_rec > ((size_t)1 << 26)) return range_error(name, ": more than 2^26 path records (goals x cap_steps)");
  if (g > q.goals.cap || g > q.hdr.cap || n_rec > q.steps.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.goals.grow(g, 3 * sizeof(int32_t)));
    WS_TRY(q.hdr.grow(g, 16));
    WS_TRY(q.steps.grow(n_rec, 16));
  }
  WS_HIP(hipMemcpyAsync(q.goals.p, goals_host, g * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  WS_TRY(launch_reach_paths(q, s, g, cap_steps));
  WS_HIP(hipMemcpyAsync(headers_host, q.hdr.p, g * 16, hipMemcpyDeviceToHost, s));
  if (n_rec) WS_HIP(hipMemcpyAsync(records_host, q.steps.p, n_rec * 16, hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

// ---- reach: the geodesic field over the last distance result of the map, map_reach.hip (the rules are stated in warpsense_hip.h)
int ws_map_reach(ws_map *m, const int32_t *seeds_host, size_t n_seeds, int32_t clear_d2, uint32_t flags, uint32_t max_rounds, size_t *n_seeded, size_t *n_reached,
                 uint32_t *rounds)
{
  if (!m) return invalid("ws_map_reach: bad argument");
  std::unique_lock<std::mutex> lock_dist, lock;
  return reach_run(m->reach, m->dist, m->ctx->stream, "ws_map_reach", seeds_host, n_seeds, clear_d2, flags, max_rounds, n_seeded, n_reached, rounds, [&] {
    WS_SETTLE(m);
    lock_dist = std::unique_lock<std::mutex>(m->dist.mu); // (the order of every call that holds both)
    lock = std::unique_lock<std::mutex>(m->reach.mu);
    return (int)WS_OK;
  });
}

const uint32_t *ws_map_reach_dev(const ws_map *m, size_t *n) { return reach_dev(m ? &m->reach : nullptr, n); }

int ws_map_reach_download(ws_map *m, uint32_t *host, size_t capacity, size_t *n_out)
{
  if (!m || !n_out) return invalid("ws_map_reach_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->reach.mu);
  return reach_download(m->reach, m->ctx->stream, host, capacity, n_out);
}

int ws_map_reach_box(ws_map *m, int32_t lo[3], uint32_t ext[3], int32_t *columns)
{
  if (!m) return invalid("ws_map_reach_box: map is NULL");
  std::lock_guard<std::mutex> lock(m->reach.mu);
  return reach_box(m->reach, lo, ext, columns);
}

int ws_map_reach_lookup(ws_map *m, const int32_t *points_host, size_t n, int32_t stride, uint32_t *cost_host)
{
  if (!m) return invalid("ws_map_reach_lookup: bad argument");
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->reach.mu);
  return reach_lookup(m->reach, m->ctx->stream, "ws_map_reach_lookup", points_host, true, n, stride, cost_host);
}

int ws_map_reach_lookup_dev(ws_map *m, const int32_t *points_dev, size_t n, int32_t stride, uint32_t *cost_dev)
{
  if (!m) return invalid("ws_map_reach_lookup_dev: bad argument");
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->reach.mu);
  return reach_lookup(m->reach, m->ctx->stream, "ws_map_reach_lookup_dev", points_dev, false, n, stride, cost_dev);
}

int ws_map_reach_paths(ws_map *m, const int32_t *goals_host, size_t g, uint32_t cap_steps, void *headers_host, void *records_host)
{
  if (!m) return invalid("ws_map_reach_paths: bad argument");
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->reach.mu);
  return reach_paths(m->reach, m->ctx->stream, "ws_map_reach_paths", goals_host, g, cap_steps, headers_host, records_host);
}

int ws_debug_reach_timing(ws_map *m, int32_t enable, float ms_out[3])
{
  if (!m) return invalid("ws_debug_reach_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->reach.mu);
  return query_timing(m->ctx->stream, m->reach.timer, enable, ms_out, REACH_PAIRS, 3);
}

int ws_debug_reach_active(ws_map *m, uint32_t *host, size_t capacity, size_t *n_out)
{
  if (!m || !n_out) return invalid("ws_debug_reach_active: NULL argument");
  std::lock_guard<std::mutex> lock(m->reach.mu);
  *n_out = m->reach.active.size();
  if (host) std::copy_n(m->reach.active.begin(), std::min(capacity, m->reach.active.size()), host);
  return WS_OK;
}

int ws_debug_reach_params(int32_t out[8])
{
  if (!out) return invalid("ws_debug_reach_params: NULL argument");
  const int32_t v[8] = {REACH_SWEEPS, REACH_VA, REACH_VB, REACH_VC, REACH_CB, REACH_CC, (int32_t)REACH_ROUNDS_PER_TILE, 0};
  std::copy(v, v + 8, out);
  return WS_OK;
}

// ---- view gain: what the host core of ws_api.h (gain_check, gain_run) needs beside it, for the window of a map here and for the chunks
// of the store in api_store_query.hip
const void *ws::gain_records_dev(const GainResult *q, size_t *n)
{
  if (n) *n = q ? q->m : 0;
  return q && q->m ? q->rec.p : nullptr;
}

const void *ws::gain_rays_dev(const GainResult *q, size_t *n)
{
  const bool have = q && q->has_rays && q->m;
  if (n) *n = have ? q->m * q->n : 0;
  return have ? q->rays.p : nullptr;
}

// `name`, `call`: the download entry point, and the entry point whose flag it misses
int ws::gain_download(const GainResult &q, hipStream_t s, const char *name, const char *call, void *records_host, void *rays_host, size_t cap_views, size_t cap_rays,
                      size_t *n_views, size_t *n_rays)
{
  const size_t total = q.has_rays ? q.m * q.n : 0;
  *n_views = q.m;
  if (n_rays) *n_rays = total;
  if (q.m && !q.has_rays && rays_host && cap_rays) return invalid(std::string(name) + ": the last " + call + " did not ask for WS_GAIN_RAYS");
  const size_t k = records_host ? std::min(cap_views, q.m) : 0, kr = rays_host ? std::min(cap_rays, total) : 0;
  if (k) WS_HIP(hipMemcpyAsync(records_host, q.rec.p, k * 32, hipMemcpyDeviceToHost, s));
  if (kr) WS_HIP(hipMemcpyAsync(rays_host, q.rays.p, kr * 8, hipMemcpyDeviceToHost, s));
  if (k || kr) WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

// ---- view gain: the unknown volume m candidate poses would see along one fan, map_gain.hip (the rules are stated in warpsense_hip.h)
int ws_map_view_gain(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], const int32_t *origins_host, size_t n_views, const int32_t *dirs_host, size_t n,
                     int32_t max_range_mm, int32_t min_value, uint32_t flags, uint64_t *best_unknown_k2)
{
  WS_TRY(gain_check("ws_map_view_gain", !m || (which != WS_MAP_AVG && which != WS_MAP_NEW), lo, hi, origins_host, n_views, dirs_host, n, max_range_mm, min_value,
                    m ? m->res : 0, flags, best_unknown_k2, [] { return (int)WS_OK; }));
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->gain.mu);
  GainResult &q = m->gain;
  int32_t l[3], ext[3];
  WS_TRY(resolve_box(m, which, lo, hi, true, "ws_map_view_gain", l, ext));
  if (n_views == 0 || n == 0) return WS_OK; // nothing written, the last result stays
  GainCall c;
  c.m = n_views, c.n = n;
  for (int k = 0; k < 3; ++k) c.lo[k] = l[k], c.hi[k] = l[k] + ext[k] - 1;
  c.res = m->res, c.max_range = max_range_mm, c.min_value = min_value, c.flags = flags;
  WS_TRY(gain_run(q, m->ctx->stream, c, origins_host, dirs_host, best_unknown_k2, false, [] { return (int)WS_OK; }, [&] { return launch_map_gain(m, q, which, c); }));
  return map_take_error(m);
}

const void *ws_map_view_gain_records_dev(const ws_map *m, size_t *n) { return gain_records_dev(m ? &m->gain : nullptr, n); }

const void *ws_map_view_gain_rays_dev(const ws_map *m, size_t *n) { return gain_rays_dev(m ? &m->gain : nullptr, n); }

int ws_map_view_gain_download(ws_map *m, void *records_host, void *rays_host, size_t cap_views, size_t cap_rays, size_t *n_views, size_t *n_rays)
{
  if (!m || !n_views) return invalid("ws_map_view_gain_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->gain.mu);
  return gain_download(m->gain, m->ctx->stream, "ws_map_view_gain_download", "ws_map_view_gain", records_host, rays_host, cap_views, cap_rays, n_views, n_rays);
}

int ws_debug_view_gain_timing(ws_map *m, int32_t enable, float ms_out[3])
{
  if (!m) return invalid("ws_debug_view_gain_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->gain.mu);
  return query_timing(m->ctx->stream, m->gain.timer, enable, ms_out, GAIN_PAIRS, 3);
}

// ---- clearance: what the host core of ws_api.h (clearance_run) needs beside it, for the window of a map here and for the store in
// api_store_query.hip.  clearance_check: every refusal that needs neither a lock nor the distance result; among these the INVALID ones
// come first.  clearance_flow: the refusals that look at the distance result, then the flow from "the old result is dropped" to the
// publish.
int ws::clearance_check(const char *name, bool bad, const int32_t *poses, size_t t, size_t p, const int32_t *body, size_t k, int32_t soft, int32_t res, uint32_t flags,
                        int32_t *reach_mm)
{
  const uint32_t known = WS_CLEARANCE_POSES | WS_CLEARANCE_OUTSIDE_OK;
  if (bad || (flags & ~known) || (t && p && !poses) || (k && !body)) return invalid(std::string(name) + ": bad argument");
  if (res <= 0) return invalid(std::string(name) + ": map_resolution <= 0");
  if (res > 1024) return range_error(name, ": the resolution must not exceed 1024 mm");
  if (k < 1 || k > CLEAR_MAX_SPHERES) return range_error(name, ": the body must have 1 .. 64 spheres");
  if (p < 1 || p > (size_t)CLEAR_MAX_LENGTH) return range_error(name, ": a trajectory must have 1 .. 65535 poses");
  if (t > ((size_t)1 << 20)) return range_error(name, ": more than 2^20 trajectories");
  if (t * p > ((size_t)1 << 21)) return range_error(name, ": more than 2^21 poses in all");
  if (soft < 0 || soft > CLEAR_MAX_LENGTH) return range_error(name, ": soft_mm must be 0 .. 65535");
  int32_t widest = 0;
  for (size_t i = 0; i < k; ++i)
  {
    const int32_t *b = body + 4 * i;
    for (int a = 0; a < 3; ++a)
      if (b[a] < -CLEAR_MAX_OFFSET || b[a] > CLEAR_MAX_OFFSET) return range_error(name, ": a sphere's offset exceeds 2^20 mm on an axis");
    if (b[3] < 0 || b[3] > CLEAR_MAX_LENGTH) return range_error(name, ": a sphere's radius must be 0 .. 65535 mm");
    widest = std::max(widest, b[3]);
  }
  *reach_mm = widest + soft;
  return WS_OK;
}

int ws::clearance_flow(ClearanceResult &q, const DistResult &d, hipStream_t s, const char *name, const int32_t *poses, bool poses_on_host, size_t t, size_t p,
                       const int32_t *body, size_t k, int32_t soft, int32_t res, uint32_t flags, int32_t reach_mm, int64_t *best)
{
  if (t == 0) return WS_OK; // nothing written, the last result stays; the distance result is not looked at
  if (!d.have) return invalid(std::string(name) + ": no distance result yet (the call runs on the records of the last distance call)");
  if ((int64_t)d.R * res < (int64_t)reach_mm)
    return range_error(name, ": max_dist_vox x resolution of the distance result is below the largest radius + soft_mm (the clamp of d2 could hide a penalty)");
  WS_TRY(q.timer.arm());
  q.t = q.p = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  q.has_poses = false;
  const bool pose_rec = (flags & WS_CLEARANCE_POSES) != 0;
  const size_t n = t * p;
  WS_TRY(q.best.alloc(1));
  if ((poses_on_host && n > q.poses.cap) || CLEAR_MAX_SPHERES > q.body.cap || t > q.rec.cap || (pose_rec && n > q.pose_rec.cap))
  {
    WS_HIP(hipStreamSynchronize(s));
    if (poses_on_host) WS_TRY(q.poses.grow(n, 12 * sizeof(int32_t)));
    WS_TRY(q.body.grow(CLEAR_MAX_SPHERES, 4 * sizeof(int32_t), DevBuf::EXACT));
    WS_TRY(q.rec.grow(t, sizeof(ClearRecord)));
    if (pose_rec) WS_TRY(q.pose_rec.grow(n, sizeof(ClearPose)));
  }
  q.timer.mark(0, s);
  WS_HIP(hipMemcpyAsync(q.body.p, body, k * 4 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (poses_on_host)
  {
    WS_HIP(hipMemcpyAsync(q.poses.p, poses, n * 12 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    poses = q.poses.as<int32_t>();
  }
  ClearCall c;
  c.t = t, c.p = p, c.k = (uint32_t)k, c.res = res, c.soft = soft, c.flags = flags;
  WS_TRY(launch_clearance(q, d, s, c, poses));
  WS_HIP(hipStreamSynchronize(s));
  q.t = t, q.p = p;
  q.has_poses = pose_rec;
  if (best) *best = (int64_t)*q.best.host;
  return WS_OK;
}

const void *ws::clearance_records_dev(const ClearanceResult *q, size_t *n)
{
  if (n) *n = q ? q->t : 0;
  return q && q->t ? q->rec.p : nullptr;
}

const void *ws::clearance_poses_dev(const ClearanceResult *q, size_t *n)
{
  const bool have = q && q->has_poses && q->t;
  if (n) *n = have ? q->t * q->p : 0;
  return have ? q->pose_rec.p : nullptr;
}

// `name`, `call`: the download entry point, and the entry point whose flag it misses
int ws::clearance_download(const ClearanceResult &q, hipStream_t s, const char *name, const char *call, void *records_host, void *poses_host, size_t cap_traj,
                           size_t cap_poses, size_t *n_traj, size_t *n_poses)
{
  const size_t total = q.has_poses ? q.t * q.p : 0;
  *n_traj = q.t;
  if (n_poses) *n_poses = total;
  if (q.t && !q.has_poses && poses_host && cap_poses) return invalid(std::string(name) + ": the last " + call + " did not ask for WS_CLEARANCE_POSES");
  const size_t k = records_host ? std::min(cap_traj, q.t) : 0, kp = poses_host ? std::min(cap_poses, total) : 0;
  if (k) WS_HIP(hipMemcpyAsync(records_host, q.rec.p, k * sizeof(ClearRecord), hipMemcpyDeviceToHost, s));
  if (kp) WS_HIP(hipMemcpyAsync(poses_host, q.pose_rec.p, kp * sizeof(ClearPose), hipMemcpyDeviceToHost, s));
  if (k || kp) WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

// ---- clearance: trajectories of a body of spheres against the last distance result of the map, map_clearance.hip (the rules are
// stated in warpsense_hip.h)
static int map_clearance(ws_map *m, const char *name, const int32_t *poses, bool poses_on_host, size_t t, size_t p, const int32_t *body, size_t k, int32_t soft,
                         uint32_t flags, int64_t *best)
{
  if (!m) return invalid(std::string(name) + ": bad argument");
  std::unique_lock<std::mutex> lock_dist, lock;
  return clearance_run(m->clear, m->dist, m->ctx->stream, name, false, poses, poses_on_host, t, p, body, k, soft, m->res, flags, best, [&] {
    WS_SETTLE(m);
    lock_dist = std::unique_lock<std::mutex>(m->dist.mu); // (the order of every call that holds both)
    lock = std::unique_lock<std::mutex>(m->clear.mu);
    return (int)WS_OK;
  });
}

int ws_map_clearance(ws_map *m, const int32_t *poses_host, size_t n_traj, size_t n_poses, const int32_t *body_host, size_t k, int32_t soft_mm, uint32_t flags,
                     int64_t *best)
{
  return map_clearance(m, "ws_map_clearance", poses_host, true, n_traj, n_poses, body_host, k, soft_mm, flags, best);
}

int ws_map_clearance_dev(ws_map *m, const int32_t *poses_dev, size_t n_traj, size_t n_poses, const int32_t *body_host, size_t k, int32_t soft_mm, uint32_t flags,
                         int64_t *best)
{
  return map_clearance(m, "ws_map_clearance_dev", poses_dev, false, n_traj, n_poses, body_host, k, soft_mm, flags, best);
}

const void *ws_map_clearance_records_dev(const ws_map *m, size_t *n) { return clearance_records_dev(m ? &m->clear : nullptr, n); }

const void *ws_map_clearance_poses_dev(const ws_map *m, size_t *n) { return clearance_poses_dev(m ? &m->clear : nullptr, n); }

int ws_map_clearance_download(ws_map *m, void *records_host, void *poses_host, size_t cap_traj, size_t cap_poses, size_t *n_traj, size_t *n_poses)
{
  if (!m || !n_traj) return invalid("ws_map_clearance_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->clear.mu);
  return clearance_download(m->clear, m->ctx->stream, "ws_map_clearance_download", "ws_map_clearance", records_host, poses_host, cap_traj, cap_poses, n_traj, n_poses);
}

int ws_debug_clearance_timing(ws_map *m, int32_t enable, float ms_out[3])
{
  if (!m) return invalid("ws_debug_clearance_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->clear.mu);
  return query_timing(m->ctx->stream, m->clear.timer, enable, ms_out, CLEAR_PAIRS, 3);
}

// ---- clearance: the two host-only statements of the rules (ws_clearance.h), no GPU and no context
int ws_clearance_centres(const int32_t *poses, size_t n_poses, const int32_t *body, size_t k, int32_t res, int32_t *voxels_out)
{
  if ((n_poses && (!poses || !voxels_out)) || (k && !body)) return invalid("ws_clearance_centres: NULL argument");
  int32_t reach_mm = 0;
  WS_TRY(clearance_check("ws_clearance_centres", false, poses, 0, 1, body, k, 0, res, 0u, &reach_mm));
  for (size_t i = 0; i < n_poses * 12; ++i)
  {
    const int64_t v = poses[i];
    if (i % 12 < 9 ? (v < -((int64_t)1 << 30) || v > ((int64_t)1 << 30)) : (v <= -((int64_t)1 << 30) || v >= ((int64_t)1 << 30)))
      return range_error("ws_clearance_centres", ": a pose leaves its domain (rot_q30 in [-2^30, 2^30], |pos_mm| < 2^30)");
  }
  for (size_t i = 0; i < n_poses; ++i)
    for (size_t j = 0; j < k; ++j)
      for (int a = 0; a < 3; ++a) voxels_out[(i * k + j) * 3 + a] = (int32_t)clear_voxel(clear_centre(poses + 12 * i, body + 4 * j, a), res);
  return WS_OK;
}

int32_t ws_clearance_margin(uint32_t d2, int32_t res, int32_t radius_mm)
{
  const uint32_t d = std::min(d2, 65025u);
  const int32_t r = std::min(std::max(res, 1), 1024), rad = std::min(std::max(radius_mm, 0), (int32_t)CLEAR_MAX_LENGTH);
  return clear_margin(d, r, rad);
}
