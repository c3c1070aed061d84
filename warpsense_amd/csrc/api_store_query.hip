// api_store_query.hip — the calls that read one chunk store (api_store.hip): its surface cloud, mesh, ray cast, point sample, distance
// field, ground with ws_store_ground_distance, frontier, reach, view gain and clearance, with their _dev, _download, _box and _timing entry
// points, and ws_debug_store_raycast_table / _find.  Each runs the host core of its window-side twin (ws_api.h, api_query.hip) over the
// chunks the call lists (ws_store_list.h), with the kernels of store_surface.hip, store_mesh.hip, store_raycast.hip, store_sample.hip,
// store_distance.hip, store_ground.hip, store_frontier.hip, map_reach.hip and store_gain.hip (the semantics are stated in
// warpsense_hip.h).  The box, the list and the chunk tables of such a call are shared with api_store_pair.hip through ws_api.h.
#include <algorithm>
#include <cstring>

#include "ws_api.h"

using namespace ws;

namespace
{
// The box of a query, into l and h.  First the refusal of a box whose hi < lo, in the name of the entry point; then the store's lock,
// into `lock` for the rest of the call; then the box (store_box_of).
// (ws_store_raycast calls this among its argument checks: its later refusals return with the lock held until then.)
int store_query_box(ws_store *st, const char *name, const int32_t lo[3], const int32_t hi[3], bool everything, std::unique_lock<std::mutex> &lock, int32_t l[3],
                    int32_t h[3])
{
  WS_TRY(store_box_refuse(name, lo, hi));
  lock = std::unique_lock<std::mutex>(st->mu);
  store_box_of(st, lo, hi, everything, l, h);
  return WS_OK;
}

// The lookup of the listed chunks (store_ray_table_fill) in the pinned table of a ray cast or a distance call: its places, and the
// fill.  A table that is too small is replaced with its device twin: the caller has synchronised the stream then.
size_t store_lookup_places(size_t n) { return n ? store_ray_table_slots(n) : 0; }
int store_lookup_fill(HostBlock &host, DevBuf &dev, const std::vector<StoreRaySlot> &listed)
{
  const size_t places = store_lookup_places(listed.size());
  if (places > host.cap)
  {
    WS_TRY(host.alloc(places, sizeof(StoreRaySlot), HostBlock::PINNED));
    WS_TRY(dev.alloc(places, sizeof(StoreRaySlot)));
  }
  if (!listed.empty()) store_ray_table_fill(listed.data(), listed.size(), host.as<StoreRaySlot>());
  return WS_OK;
}

// Room for `need` bytes of chunk tables of a surface or mesh call, pinned and on the device (`want` where they have to grow, which
// waits for the stream: the kernels in flight read the old table)
int store_tables_reserve(ws_store *st, HostBlock &host, DevBuf &dev, size_t need, size_t want)
{
  if (need <= host.cap && need <= dev.cap) return WS_OK; // (both: a failed allocation of the second leaves the first one grown)
  WS_HIP(hipStreamSynchronize(st->ctx->stream));
  WS_TRY(host.alloc(want, 1, HostBlock::PINNED));
  return dev.alloc(want, 1);
}

// The tables of a mesh call over the n listed chunks (0 < n < 2^19), into st->mesh.table_host: the word-space tables, and the list
// positions of every chunk's 26 neighbours (and its own).  Everything is O(n log n).
int store_mesh_tables(ws_store *st, const std::vector<StoreRaySlot> &listed)
{
  int32_t off[27][3];
  for (int c = 0; c < 27; ++c) off[c][0] = c / 9 - 1, off[c][1] = c / 3 % 3 - 1, off[c][2] = c % 3 - 1;
  return store_chunk_tables(st, st->mesh.table_host, st->mesh.table_dev, listed, store_mesh_table_bytes, off, 27);
}

// The tables of a frontier call over the n listed chunks (0 < n < 2^19), into st->frontier.table_host: the word-space tables, and the
// list positions of every chunk's six face neighbours, -x +x -y +y -z +z
int store_frontier_tables(ws_store *st, const std::vector<StoreRaySlot> &listed)
{
  static const int32_t off[6][3] = {{-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
  return store_chunk_tables(st, st->frontier.table_host, st->frontier.table_dev, listed, store_frontier_table_bytes, off, 6);
}

// What ws_store_distance and ws_store_ground do alike in front of their passes.  check(box) is the entry point's *_check with its own
// arguments and p.ext, &p.n; its box(e) is here: the refusal of hi < lo, the lock, the box, the timer armed, the extents.  Then the
// present chunks the box overlaps, with the refusal of too many, and the call's fields: the columns and the z range the chunks cover
// inside the box.
struct StoreColumns
{
  std::unique_lock<std::mutex> lock;
  StoreDistCall c;
  uint32_t ext[3];
  size_t n = 0;
  std::vector<StoreRaySlot> listed;
};
template <typename Check>
int store_columns(ws_store *st, const char *name, const int32_t *lo, const int32_t *hi, QueryTimer *timer, StoreColumns &p, Check check)
{
  StoreDistCall &c = p.c;
  WS_TRY(check([&](uint64_t e[3]) {
    WS_TRY(store_query_box(st, name, lo, hi, false, p.lock, c.lo, c.hi));
    WS_TRY(timer->arm());
    if (c.lo[0] > c.hi[0]) return (int)WS_OK; // no box and no chunk: zero records
    for (int k = 0; k < 3; ++k) e[k] = (uint64_t)((int64_t)c.hi[k] - (int64_t)c.lo[k]) + 1u;
    return (int)WS_OK;
  }));
  if (p.n) store_list(st, c.lo, c.hi, p.listed);
  if (p.listed.size() >= STORE_LIST_LIMIT) return range_error(name, ": the box overlaps 2^19 present chunks or more");
  c.n_chunks = (uint32_t)p.listed.size();
  c.nx = p.ext[0], c.ny = p.ext[1];
  store_z_range(p.listed, c.lo[2], c.hi[2], &c.zlo, &c.zhi);
  return WS_OK;
}

// ... and at the head of their first pass: the lookup of the listed chunks, behind a synchronise where its table must grow
int store_columns_lookup(ws_store *st, HostBlock &host, DevBuf &dev, const std::vector<StoreRaySlot> &listed)
{
  if (store_lookup_places(listed.size()) > host.cap) WS_HIP(hipStreamSynchronize(st->ctx->stream));
  return store_lookup_fill(host, dev, listed);
}
} // namespace

// (declared in ws_api.h: the calls over two stores, api_store_pair.hip, take their box, list and tables by the same rules)
namespace ws
{
int store_box_refuse(const char *name, const int32_t lo[3], const int32_t hi[3])
{
  for (int k = 0; k < 3 && lo; ++k)
    if (hi[k] < lo[k]) return invalid(std::string(name) + ": hi < lo");
  return WS_OK;
}

// The box of a call, into l and h: the call's, or without one all of int32 where `everything` (a ray cast), else the bounding box of
// the present chunks (keys are floor(int32 / 64): 64 k + 63 fits), which leaves l > h in an empty store.
void store_box_of(const ws_store *st, const int32_t lo[3], const int32_t hi[3], bool everything, int32_t l[3], int32_t h[3])
{
  for (int k = 0; k < 3; ++k) l[k] = lo ? lo[k] : everything ? INT32_MIN : INT32_MAX, h[k] = lo ? hi[k] : everything ? INT32_MAX : INT32_MIN;
  if (!lo && !everything)
    for (const auto &kv : st->dir)
      for (int k = 0; k < 3; ++k) l[k] = std::min(l[k], kv.first[k] * STORE_CS), h[k] = std::max(h[k], kv.first[k] * STORE_CS + (STORE_CS - 1));
}

// The written chunks a query lists, {cx, cy, cz, slot} ascending like the directory: those the box overlaps, or without a box
// (lo == NULL) all of them.  The directory is ordered by cx first and only the keys of the box's cx range are visited: nothing here
// follows the volume of the box.
void store_list(const ws_store *st, const int32_t *lo, const int32_t *hi, std::vector<StoreRaySlot> &listed)
{
  const auto put = [&](const StoreKey &key, const ws_store::Entry &e) { listed.push_back(StoreRaySlot{key[0], key[1], key[2], e.slot}); };
  listed.clear();
  if (!lo)
  {
    for (const auto &kv : st->dir)
      if (kv.second.written) put(kv.first, kv.second);
    return;
  }
  const ChunkRange cr(lo, hi);
  for (auto it = st->dir.lower_bound(StoreKey{cr.c0[0], INT32_MIN, INT32_MIN}); it != st->dir.end() && it->first[0] - cr.c0[0] < cr.nc[0]; ++it)
  {
    bool in = it->second.written;
    for (int k = 1; k < 3; ++k) in = in && it->first[k] >= cr.c0[k] && it->first[k] - cr.c0[k] < cr.nc[k];
    if (in) put(it->first, it->second);
  }
}

// A store call waits for the stream even after a failed enqueue (whose error it reports): the pinned table of the call must be free
// again when the call returns.
int store_enqueued(const ws_store *st, int rc)
{
  if (rc != WS_OK) (void)hipStreamSynchronize(st->ctx->stream);
  return rc;
}

// The chunk tables of a call over the n listed chunks (0 < n < 2^19): room for bytes(n), grown to bytes(n + n / 8); the word-space
// tables; behind them the neighbour positions at the n_off offsets (none for a call that reads no neighbour chunk).
int store_chunk_tables(ws_store *st, HostBlock &host, DevBuf &dev, const std::vector<StoreRaySlot> &listed, size_t (*bytes)(size_t), const int32_t (*off)[3], int n_off)
{
  const size_t n = listed.size();
  WS_TRY(store_tables_reserve(st, host, dev, bytes(n), bytes(n + n / 8)));
  uint32_t *grp = host.as<uint32_t>();
  store_word_tables(listed, grp);
  store_neighbour_positions(listed, off, n_off, grp + 8 * n);
  return WS_OK;
}
} // namespace ws

// ---- the surface cloud, the mesh and the ray cast of the store: the rules and the host flow of ws_map_surface, ws_map_mesh and
// ws_map_raycast over the chunks, store_surface.hip, store_mesh.hip and store_raycast.hip
int ws_store_surface(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t band, int32_t tau, int32_t map_resolution, uint32_t flags, size_t *n_out)
{
  if (!st || (flags & ~WS_SURFACE_MARKER) || ((lo == nullptr) != (hi == nullptr)) || tau <= 0 || map_resolution <= 0) return invalid("ws_store_surface: bad argument");
  std::unique_lock<std::mutex> lock;
  StoreSurfCall c;
  WS_TRY(store_query_box(st, "ws_store_surface", lo, hi, false, lock, c.lo, c.hi));
  ws_store::Surface &q = st->surf;
  std::vector<StoreRaySlot> listed;
  if (c.lo[0] <= c.hi[0]) store_list(st, c.lo, c.hi, listed); // (else: no box and no chunk)
  if (listed.size() >= STORE_LIST_LIMIT) return range_error("ws_store_surface", ": the box overlaps 2^19 present chunks or more (4096 words each must stay below 2^31)");
  WS_TRY(q.timer.arm());
  if (listed.empty()) // an empty store, or the box meets no present chunk
  {
    q.n = 0, q.has_marker = false;
    if (n_out) *n_out = 0;
    return WS_OK;
  }
  c.n_chunks = (uint32_t)listed.size();
  c.band = band <= 0 ? tau : band, c.tau = tau, c.res = map_resolution;
  const bool marker = (flags & WS_SURFACE_MARKER) != 0;
  const size_t n_words = (size_t)c.n_chunks * 4096u;
  WS_TRY(store_chunk_tables(st, q.table_host, q.table_dev, listed, store_word_table_bytes, nullptr, 0));
  return surface_run(
      q, st->ctx->stream, store_surface_blocks(c.n_chunks), marker, n_out, n_words > q.mask.cap, [&] { return q.mask.grow(n_words, sizeof(uint64_t)); },
      [&] { return store_enqueued(st, launch_store_surface_count(st, q, c)); },
      [&](size_t cap) { return store_enqueued(st, launch_store_surface_emit(st, q, c, marker, cap)); });
}

const void *ws_store_surface_records_dev(const ws_store *st, size_t *n) { return surface_records_dev(st ? &st->surf : nullptr, n); }

const float *ws_store_surface_marker_dev(const ws_store *st, size_t *n) { return surface_marker_dev(st ? &st->surf : nullptr, n); }

int ws_store_surface_download(ws_store *st, void *records_host, float *marker_host, size_t capacity_points, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_surface_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return surface_download(st->surf, st->ctx->stream, "ws_store_surface_download", "ws_store_surface", records_host, marker_host, capacity_points, n_out);
}

int ws_debug_store_surface_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  return store_timing(st, "ws_debug_store_surface_timing", &ws_store::surf, enable, ms_out, SURF_PAIRS);
}

int ws_store_mesh(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t map_resolution, uint32_t flags, size_t *n_vertices, size_t *n_faces)
{
  if (!st || (flags & ~WS_MESH_ANY_WEIGHT) || ((lo == nullptr) != (hi == nullptr)) || map_resolution <= 0) return invalid("ws_store_mesh: bad argument");
  std::unique_lock<std::mutex> lock;
  StoreMeshCall c;
  WS_TRY(store_query_box(st, "ws_store_mesh", lo, hi, false, lock, c.lo, c.hi));
  ws_store::Mesh &q = st->mesh;
  WS_TRY(q.timer.arm());
  if (c.lo[0] > c.hi[0]) return mesh_publish(q, 0, 0, n_vertices, n_faces); // no box and no chunk
  WS_TRY(mesh_corners_fit(c.lo, c.hi, map_resolution, "ws_store_mesh"));
  if (c.hi[0] == c.lo[0] || c.hi[1] == c.lo[1] || c.hi[2] == c.lo[2]) return mesh_publish(q, 0, 0, n_vertices, n_faces); // one voxel thick along an axis: no cells
  std::vector<StoreRaySlot> listed;
  store_list(st, c.lo, c.hi, listed);
  if (listed.empty()) return mesh_publish(q, 0, 0, n_vertices, n_faces); // the box meets no present chunk
  if (listed.size() >= STORE_LIST_LIMIT) return range_error("ws_store_mesh", ": the box overlaps 2^19 present chunks or more (4096 words each must stay below 2^31)");
  WS_TRY(store_mesh_tables(st, listed));
  c.n_chunks = (uint32_t)listed.size();
  c.res = map_resolution;
  c.flags = flags;
  return mesh_run(
      q, st->ctx->stream, "ws_store_mesh", (uint64_t)c.n_chunks * 4096u, n_vertices, n_faces, [&] { return store_enqueued(st, launch_store_mesh_count(st, q, c)); },
      [&] { return store_enqueued(st, launch_store_mesh_emit(st, q, c)); });
}

const void *ws_store_mesh_vertices_dev(const ws_store *st, size_t *n) { return mesh_vertices_dev(st ? &st->mesh : nullptr, n); }

const uint32_t *ws_store_mesh_faces_dev(const ws_store *st, size_t *n) { return mesh_faces_dev(st ? &st->mesh : nullptr, n); }

int ws_store_mesh_download(ws_store *st, void *vertices_host, uint32_t *faces_host, size_t cap_vertices, size_t cap_faces, size_t *n_vertices, size_t *n_faces)
{
  if (!st || !n_vertices || !n_faces) return invalid("ws_store_mesh_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return mesh_download(st->mesh, st->ctx->stream, vertices_host, faces_host, cap_vertices, cap_faces, n_vertices, n_faces);
}

int ws_debug_store_mesh_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  return store_timing(st, "ws_debug_store_mesh_timing", &ws_store::mesh, enable, ms_out, MESH_PAIRS);
}

static int store_raycast(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin[3], const int32_t *dirs, bool dirs_on_host, size_t n,
                         int32_t max_range, int32_t res, uint32_t flags, size_t *n_hits)
{
  std::unique_lock<std::mutex> lock;
  StoreRayCall c;
  c.res = res;
  WS_TRY(raycast_check("ws_store_raycast", !st || ((lo == nullptr) != (hi == nullptr)), origin, dirs, n, max_range, res, flags, [&] {
    WS_TRY(store_query_box(st, "ws_store_raycast", lo, hi, true, lock, c.lo, c.hi));
    return res <= 0 ? invalid("ws_store_raycast: map_resolution <= 0") : (int)WS_OK;
  }));
  ws_store::Ray &q = st->ray;
  std::vector<StoreRaySlot> listed;
  store_list(st, lo, hi, listed); // (without a box: every written chunk)
  if (listed.size() >= STORE_LIST_LIMIT) return range_error("ws_store_raycast", ": the call lists 2^19 present chunks or more");
  c.n_chunks = (uint32_t)listed.size();
  store_live_box(listed, c.lo, c.hi, c.blo, c.bhi);
  // (no listed chunk: the call still launches and answers no-hit for every ray)
  return raycast_run(
      q, st->ctx->stream, dirs, dirs_on_host, n, flags, n_hits, store_lookup_places(listed.size()) > q.table_host.cap,
      [&] { return store_lookup_fill(q.table_host, q.table_dev, listed); },
      [&](const int32_t *dirs_dev) { return store_enqueued(st, launch_store_raycast(st, q, c, origin, dirs_dev, n, max_range, flags)); });
}

int ws_store_raycast(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin_mm[3], const int32_t *dirs_host, size_t n, int32_t max_range_mm,
                     int32_t map_resolution, uint32_t flags, size_t *n_hits)
{
  return store_raycast(st, lo, hi, origin_mm, dirs_host, true, n, max_range_mm, map_resolution, flags, n_hits);
}

int ws_store_raycast_dev(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin_mm[3], const int32_t *dirs_dev, size_t n, int32_t max_range_mm,
                         int32_t map_resolution, uint32_t flags, size_t *n_hits)
{
  return store_raycast(st, lo, hi, origin_mm, dirs_dev, false, n, max_range_mm, map_resolution, flags, n_hits);
}

const void *ws_store_raycast_records_dev(const ws_store *st, size_t *n) { return raycast_records_dev(st ? &st->ray : nullptr, n); }

const int32_t *ws_store_raycast_gradient_dev(const ws_store *st, size_t *n) { return raycast_gradient_dev(st ? &st->ray : nullptr, n); }

int ws_store_raycast_download(ws_store *st, void *records_host, int32_t *gradient_host, size_t capacity_rays, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_raycast_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return raycast_download(st->ray, st->ctx->stream, "ws_store_raycast_download", "ws_store_raycast", records_host, gradient_host, capacity_rays, n_out);
}

int ws_debug_store_raycast_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  return store_timing(st, "ws_debug_store_raycast_timing", &ws_store::ray, enable, ms_out, RAY_PAIRS);
}

// ---- the point sample of the store: the rules and the host flow of ws_map_sample over the chunks, store_sample.hip
static int store_sample(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *points, bool points_on_host, size_t n, int32_t band, int32_t res,
                        uint32_t flags, uint64_t counts[4])
{
  std::unique_lock<std::mutex> lock;
  StoreRayCall c;
  c.res = res;
  WS_TRY(sample_check("ws_store_sample", !st || ((lo == nullptr) != (hi == nullptr)) || band <= 0, points, n, res, flags, [&] {
    WS_TRY(store_query_box(st, "ws_store_sample", lo, hi, true, lock, c.lo, c.hi));
    return res <= 0 ? invalid("ws_store_sample: map_resolution <= 0") : (int)WS_OK;
  }));
  ws_store::Sample &q = st->sample;
  std::vector<StoreRaySlot> listed;
  store_list(st, lo, hi, listed); // (without a box: every written chunk)
  if (listed.size() >= STORE_LIST_LIMIT) return range_error("ws_store_sample", ": the call lists 2^19 present chunks or more");
  c.n_chunks = (uint32_t)listed.size();
  store_live_box(listed, c.lo, c.hi, c.blo, c.bhi);
  // (no listed chunk: the call still launches and answers UNKNOWN for every point)
  return sample_run(
      q, st->ctx->stream, points, points_on_host, n, flags, counts, store_lookup_places(listed.size()) > q.table_host.cap,
      [&] { return store_lookup_fill(q.table_host, q.table_dev, listed); },
      [&](const int32_t *pts_dev) { return store_enqueued(st, launch_store_sample(st, q, c, pts_dev, n, band, flags)); });
}

int ws_store_sample(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *points_host, size_t n, int32_t band_mm, int32_t map_resolution,
                    uint32_t flags, uint64_t counts[4])
{
  return store_sample(st, lo, hi, points_host, true, n, band_mm, map_resolution, flags, counts);
}

int ws_store_sample_dev(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *points_dev, size_t n, int32_t band_mm, int32_t map_resolution,
                        uint32_t flags, uint64_t counts[4])
{
  return store_sample(st, lo, hi, points_dev, false, n, band_mm, map_resolution, flags, counts);
}

const void *ws_store_sample_records_dev(const ws_store *st, size_t *n) { return sample_records_dev(st ? &st->sample : nullptr, n); }

const int32_t *ws_store_sample_gradient_dev(const ws_store *st, size_t *n) { return sample_gradient_dev(st ? &st->sample : nullptr, n); }

const int32_t *ws_store_sample_selected_dev(const ws_store *st, size_t *n) { return sample_selected_dev(st ? &st->sample : nullptr, n); }

int ws_store_sample_download(ws_store *st, void *records_host, int32_t *gradient_host, int32_t *selected_host, size_t capacity_points, size_t capacity_selected,
                             size_t *n_out, size_t *n_selected)
{
  if (!st || !n_out) return invalid("ws_store_sample_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return sample_download(st->sample, st->ctx->stream, "ws_store_sample_download", "ws_store_sample", records_host, gradient_host, selected_host, capacity_points,
                         capacity_selected, n_out, n_selected);
}

int ws_debug_store_sample_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  return store_timing(st, "ws_debug_store_sample_timing", &ws_store::sample, enable, ms_out, SAMPLE_PAIRS);
}

// ---- the distance field of the store: the rules and the host flow of ws_map_distance over the chunks, store_distance.hip
int ws_store_distance(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t max_dist_vox, uint32_t flags, size_t *n_sites)
{
  StoreColumns p;
  WS_TRY(store_columns(st, "ws_store_distance", lo, hi, st ? &st->dist.timer : nullptr, p, [&](auto box) {
    return distance_check("ws_store_distance", !st, lo, hi, max_dist_vox, flags, box, p.ext, &p.n);
  }));
  ws_store::Dist &q = st->dist;
  return store_enqueued(st, distance_run(q, st->ctx->stream, p.c.lo, p.ext, max_dist_vox, flags, p.n, n_sites, [&] {
    WS_TRY(store_columns_lookup(st, q.table_host, q.table_dev, p.listed));
    return launch_store_dist_classify(st, q, p.c, max_dist_vox, flags);
  }));
}

const uint32_t *ws_store_distance_dev(const ws_store *st, size_t *n) { return distance_dev(st ? &st->dist : nullptr, n); }

int ws_store_distance_download(ws_store *st, uint32_t *host, size_t capacity, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_distance_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return distance_download(st->dist, st->ctx->stream, host, capacity, n_out);
}

int ws_debug_store_distance_timing(ws_store *st, int32_t enable, float ms_out[4])
{
  return store_timing(st, "ws_debug_store_distance_timing", &ws_store::dist, enable, ms_out, DIST_PAIRS);
}

// ---- the ground of the store: the rules and the host flow of ws_map_ground over the chunks, store_ground.hip
int ws_store_ground(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t clear_vox, uint32_t flags, uint64_t counts[4])
{
  StoreColumns p;
  WS_TRY(store_columns(st, "ws_store_ground", lo, hi, st ? &st->ground.timer : nullptr, p, [&](auto box) {
    return ground_check("ws_store_ground", !st, lo, hi, clear_vox, flags, box, p.ext, &p.n);
  }));
  ws_store::Ground &q = st->ground;
  return store_enqueued(st, ground_run(q, st->ctx->stream, p.c.lo, p.ext, p.n, counts, [&] {
    WS_TRY(store_columns_lookup(st, q.table_host, q.table_dev, p.listed));
    return launch_store_ground_levels(st, q, p.c, clear_vox, flags);
  }));
}

const void *ws_store_ground_dev(const ws_store *st, size_t *n) { return ground_dev(st ? &st->ground : nullptr, n); }

int ws_store_ground_download(ws_store *st, void *host, size_t capacity, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_ground_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return ground_download(st->ground, st->ctx->stream, host, capacity, n_out);
}

int ws_store_ground_box(ws_store *st, int32_t lo[3], uint32_t ext[3])
{
  if (!st) return invalid("ws_store_ground_box: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return ground_box(st->ground, "ws_store_ground_box", lo, ext);
}

int ws_debug_store_ground_timing(ws_store *st, int32_t enable, float ms_out[2])
{
  return store_timing(st, "ws_debug_store_ground_timing", &ws_store::ground, enable, ms_out, GROUND_PAIRS);
}

// the bridge to the planner: a column distance call whose pass 0 reads the last ground result of the store
int ws_store_ground_distance(ws_store *st, int32_t max_step_q8, int32_t max_dist_vox, uint32_t flags, size_t *n_sites)
{
  std::unique_lock<std::mutex> lock;
  int32_t l[3] = {0, 0, 0};
  uint32_t ext[3];
  size_t n = 0;
  WS_TRY(ground_distance_check(
      "ws_store_ground_distance", !st, max_step_q8, max_dist_vox, flags,
      [&](uint64_t e[3]) {
        lock = std::unique_lock<std::mutex>(st->mu);
        if (!st->ground.have) return invalid("ws_store_ground_distance: no ground result yet (the call runs on the records of the last ws_store_ground)");
        WS_TRY(st->dist.timer.arm());
        for (int k = 0; k < 3; ++k) e[k] = st->ground.n ? (uint64_t)st->ground.ext[k] : 0u, l[k] = st->ground.lo[k];
        return (int)WS_OK;
      },
      ext, &n));
  ws_store::Dist &q = st->dist;
  hipStream_t s = st->ctx->stream;
  const uint32_t dflags = flags | WS_DISTANCE_COLUMNS;
  return store_enqueued(st, distance_run(q, s, l, ext, max_dist_vox, dflags, n, n_sites,
                                         [&] { return launch_ground_sites(s, st->ground, q, (uint32_t)max_step_q8, max_dist_vox, dflags); }));
}

int ws_debug_store_raycast_table(const int32_t *keys_slots, size_t n, int32_t *table, size_t capacity_places, size_t *n_places)
{
  if ((n && table && !keys_slots) || !n_places || n >= STORE_LIST_LIMIT) return invalid("ws_debug_store_raycast_table: bad argument");
  *n_places = store_ray_table_slots(n);
  if (!table) return WS_OK;
  if (capacity_places < *n_places) return invalid("ws_debug_store_raycast_table: the table does not fit");
  std::vector<StoreRaySlot> in(n), out(*n_places);
  if (n) std::memcpy(in.data(), keys_slots, n * sizeof(StoreRaySlot));
  store_ray_table_fill(in.data(), n, out.data());
  std::memcpy(table, out.data(), out.size() * sizeof(StoreRaySlot));
  return WS_OK;
}

uint32_t ws_debug_store_raycast_find(const int32_t *table, size_t n_places, const int32_t key[3])
{
  if (!table || !key || n_places < 2 || (n_places & (n_places - 1))) return STORE_ABSENT;
  std::vector<StoreRaySlot> t(n_places);
  std::memcpy(t.data(), table, n_places * sizeof(StoreRaySlot));
  return store_ray_find(t.data(), (uint32_t)n_places - 1u, key[0], key[1], key[2]);
}

// ---- the frontier of the store: the rules and the host flow of ws_map_frontier over the chunks, store_frontier.hip
int ws_store_frontier(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t min_value, uint32_t flags, size_t *n_out, size_t *n_clusters)
{
  WS_TRY(frontier_check("ws_store_frontier", !st, lo, hi, min_value, flags));
  std::unique_lock<std::mutex> lock;
  StoreFrontierCall c;
  WS_TRY(store_query_box(st, "ws_store_frontier", lo, hi, false, lock, c.lo, c.hi));
  ws_store::Frontier &q = st->frontier;
  std::vector<StoreRaySlot> listed;
  if (c.lo[0] <= c.hi[0]) store_list(st, c.lo, c.hi, listed); // (else: no box and no chunk)
  if (listed.size() >= STORE_LIST_LIMIT) return range_error("ws_store_frontier", ": the box overlaps 2^19 present chunks or more (4096 words each must stay below 2^31)");
  WS_TRY(q.timer.arm());
  if (listed.empty()) // an empty store, or the box meets no present chunk: nothing in it is free
    return frontier_publish(q, 0, 0, (flags & WS_FRONTIER_CLUSTERS) != 0, n_out, n_clusters);
  c.n_chunks = (uint32_t)listed.size();
  c.min_value = min_value, c.flags = flags;
  const size_t n_words = (size_t)c.n_chunks * 4096u;
  WS_TRY(store_frontier_tables(st, listed));
  return frontier_run(
      q, st->ctx->stream, "ws_store_frontier", store_surface_blocks(c.n_chunks), flags, n_out, n_clusters, n_words > q.mask.cap,
      [&] { return q.mask.grow(n_words, sizeof(uint64_t)); }, [&] { return store_enqueued(st, launch_store_frontier_count(st, q, c)); },
      [&](size_t cap) { return store_enqueued(st, launch_store_frontier_emit(st, q, c, cap)); });
}

const void *ws_store_frontier_records_dev(const ws_store *st, size_t *n) { return surface_records_dev(st ? &st->frontier : nullptr, n); }

const uint32_t *ws_store_frontier_labels_dev(const ws_store *st, size_t *n) { return frontier_labels_dev(st ? &st->frontier : nullptr, n); }

const void *ws_store_frontier_clusters_dev(const ws_store *st, size_t *n) { return frontier_clusters_dev(st ? &st->frontier : nullptr, n); }

int ws_store_frontier_download(ws_store *st, void *records_host, uint32_t *labels_host, void *clusters_host, size_t cap_records, size_t cap_clusters, size_t *n_out,
                               size_t *n_clusters)
{
  if (!st || !n_out) return invalid("ws_store_frontier_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return frontier_download(st->frontier, st->ctx->stream, "ws_store_frontier_download", "ws_store_frontier", records_host, labels_host, clusters_host, cap_records,
                           cap_clusters, n_out, n_clusters);
}

int ws_debug_store_frontier_timing(ws_store *st, int32_t enable, float ms_out[4])
{
  return store_timing(st, "ws_debug_store_frontier_timing", &ws_store::frontier, enable, ms_out, FRONTIER_PAIRS);
}

// ---- the reach of the store: ws_map_reach over the last ws_store_distance result (map_reach.hip reads its records alone)
int ws_store_reach(ws_store *st, const int32_t *seeds_host, size_t n_seeds, int32_t clear_d2, uint32_t flags, uint32_t max_rounds, size_t *n_seeded, size_t *n_reached,
                   uint32_t *rounds)
{
  if (!st) return invalid("ws_store_reach: bad argument");
  std::unique_lock<std::mutex> lock;
  return reach_run(st->reach, st->dist, st->ctx->stream, "ws_store_reach", seeds_host, n_seeds, clear_d2, flags, max_rounds, n_seeded, n_reached, rounds, [&] {
    servers_leave(st->ctx);
    lock = std::unique_lock<std::mutex>(st->mu);
    return (int)WS_OK;
  });
}

const uint32_t *ws_store_reach_dev(const ws_store *st, size_t *n) { return reach_dev(st ? &st->reach : nullptr, n); }

int ws_store_reach_download(ws_store *st, uint32_t *host, size_t capacity, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_reach_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_download(st->reach, st->ctx->stream, host, capacity, n_out);
}

int ws_store_reach_box(ws_store *st, int32_t lo[3], uint32_t ext[3], int32_t *columns)
{
  if (!st) return invalid("ws_store_reach_box: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_box(st->reach, lo, ext, columns);
}

int ws_store_reach_lookup(ws_store *st, const int32_t *points_host, size_t n, int32_t stride, uint32_t *cost_host)
{
  if (!st) return invalid("ws_store_reach_lookup: bad argument");
  servers_leave(st->ctx);
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_lookup(st->reach, st->ctx->stream, "ws_store_reach_lookup", points_host, true, n, stride, cost_host);
}

int ws_store_reach_lookup_dev(ws_store *st, const int32_t *points_dev, size_t n, int32_t stride, uint32_t *cost_dev)
{
  if (!st) return invalid("ws_store_reach_lookup_dev: bad argument");
  servers_leave(st->ctx);
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_lookup(st->reach, st->ctx->stream, "ws_store_reach_lookup_dev", points_dev, false, n, stride, cost_dev);
}

int ws_store_reach_paths(ws_store *st, const int32_t *goals_host, size_t g, uint32_t cap_steps, void *headers_host, void *records_host)
{
  if (!st) return invalid("ws_store_reach_paths: bad argument");
  servers_leave(st->ctx);
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_paths(st->reach, st->ctx->stream, "ws_store_reach_paths", goals_host, g, cap_steps, headers_host, records_host);
}

int ws_debug_store_reach_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  return store_timing(st, "ws_debug_store_reach_timing", &ws_store::reach, enable, ms_out, REACH_PAIRS);
}

// ---- the view gain of the store: the rules and the host flow of ws_map_view_gain over the chunks, store_gain.hip
int ws_store_view_gain(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *origins_host, size_t n_views, const int32_t *dirs_host, size_t n,
                       int32_t max_range_mm, int32_t map_resolution, int32_t min_value, uint32_t flags, uint64_t *best_unknown_k2)
{
  std::unique_lock<std::mutex> lock;
  GainCall c;
  WS_TRY(gain_check("ws_store_view_gain", !st, lo, hi, origins_host, n_views, dirs_host, n, max_range_mm, min_value, map_resolution, flags, best_unknown_k2, [&] {
    if (map_resolution <= 0) return invalid("ws_store_view_gain: map_resolution <= 0");
    return store_box_refuse("ws_store_view_gain", lo, hi);
  }));
  servers_leave(st->ctx);
  WS_TRY(store_query_box(st, "ws_store_view_gain", lo, hi, false, lock, c.lo, c.hi)); // (without a box: the bounding box of the chunks; none: empty)
  if (n_views == 0 || n == 0) return WS_OK; // nothing written, the last result stays
  ws_store::Gain &q = st->gain;
  std::vector<StoreRaySlot> listed;
  if (c.lo[0] <= c.hi[0]) store_list(st, c.lo, c.hi, listed);
  if (listed.size() >= STORE_LIST_LIMIT) return range_error("ws_store_view_gain", ": the box overlaps 2^19 present chunks or more");
  c.m = n_views, c.n = n;
  c.res = map_resolution, c.max_range = max_range_mm, c.min_value = min_value, c.flags = flags;
  return gain_run(
      q, st->ctx->stream, c, origins_host, dirs_host, best_unknown_k2, store_lookup_places(listed.size()) > q.table_host.cap,
      [&] { return store_lookup_fill(q.table_host, q.table_dev, listed); }, [&] { return store_enqueued(st, launch_store_gain(st, q, c, (uint32_t)listed.size())); });
}

const void *ws_store_view_gain_records_dev(const ws_store *st, size_t *n) { return gain_records_dev(st ? &st->gain : nullptr, n); }

const void *ws_store_view_gain_rays_dev(const ws_store *st, size_t *n) { return gain_rays_dev(st ? &st->gain : nullptr, n); }

int ws_store_view_gain_download(ws_store *st, void *records_host, void *rays_host, size_t cap_views, size_t cap_rays, size_t *n_views, size_t *n_rays)
{
  if (!st || !n_views) return invalid("ws_store_view_gain_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return gain_download(st->gain, st->ctx->stream, "ws_store_view_gain_download", "ws_store_view_gain", records_host, rays_host, cap_views, cap_rays, n_views, n_rays);
}

int ws_debug_store_view_gain_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  return store_timing(st, "ws_debug_store_view_gain_timing", &ws_store::gain, enable, ms_out, GAIN_PAIRS);
}

// ---- the clearance of the store: ws_map_clearance over the last ws_store_distance result (map_clearance.hip reads its records alone)
static int store_clearance(ws_store *st, const char *name, const int32_t *poses, bool poses_on_host, size_t t, size_t p, const int32_t *body, size_t k, int32_t soft,
                           int32_t map_resolution, uint32_t flags, int64_t *best)
{
  if (!st) return invalid(std::string(name) + ": bad argument");
  std::unique_lock<std::mutex> lock;
  return clearance_run(st->clear, st->dist, st->ctx->stream, name, false, poses, poses_on_host, t, p, body, k, soft, map_resolution, flags, best, [&] {
    servers_leave(st->ctx);
    lock = std::unique_lock<std::mutex>(st->mu);
    return (int)WS_OK;
  });
}

int ws_store_clearance(ws_store *st, const int32_t *poses_host, size_t n_traj, size_t n_poses, const int32_t *body_host, size_t k, int32_t soft_mm,
                       int32_t map_resolution, uint32_t flags, int64_t *best)
{
  return store_clearance(st, "ws_store_clearance", poses_host, true, n_traj, n_poses, body_host, k, soft_mm, map_resolution, flags, best);
}

int ws_store_clearance_dev(ws_store *st, const int32_t *poses_dev, size_t n_traj, size_t n_poses, const int32_t *body_host, size_t k, int32_t soft_mm,
                           int32_t map_resolution, uint32_t flags, int64_t *best)
{
  return store_clearance(st, "ws_store_clearance_dev", poses_dev, false, n_traj, n_poses, body_host, k, soft_mm, map_resolution, flags, best);
}

const void *ws_store_clearance_records_dev(const ws_store *st, size_t *n) { return clearance_records_dev(st ? &st->clear : nullptr, n); }

const void *ws_store_clearance_poses_dev(const ws_store *st, size_t *n) { return clearance_poses_dev(st ? &st->clear : nullptr, n); }

int ws_store_clearance_download(ws_store *st, void *records_host, void *poses_host, size_t cap_traj, size_t cap_poses, size_t *n_traj, size_t *n_poses)
{
  if (!st || !n_traj) return invalid("ws_store_clearance_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return clearance_download(st->clear, st->ctx->stream, "ws_store_clearance_download", "ws_store_clearance", records_host, poses_host, cap_traj, cap_poses, n_traj,
                            n_poses);
}

int ws_debug_store_clearance_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  return store_timing(st, "ws_debug_store_clearance_timing", &ws_store::clear, enable, ms_out, CLEAR_PAIRS);
}
