// ws_api.h — what the host files of the C API (api_*.hip) share, and nothing else: the refusals, the map's settle-and-report
// steps, the box rules, what the three host files of the chunk store share (api_store.hip: the store itself; api_store_query.hip:
// the calls that read one store; api_store_pair.hip: the calls over two stores) with each other and with api_pack.hip, and the host
// cores that the queries of a map window (api_query.hip) and of the chunk store (api_store_query.hip) both run.  What one file
// uses alone is static in that file.  Everything here is in namespace ws or a template: it mangles, so the library exports no
// unprefixed C name beside the ws_* entry points (tests/test_abi_and_host.py holds that).
#pragma once

#include <algorithm>
#include <string>

#include "ws_internal.h"
#include "ws_store_list.h"

namespace ws
{
// ---- api_core.hip: the refusals (the text goes to the thread's last error), and the two things a call owes the context
int invalid(const char *msg);
int invalid(const std::string &msg);
int range_error(const char *name, const char *what);
void servers_leave(ws_context *ctx); // a resident server of ws_reg_iterate leaves the stream to whoever enqueues other work
int ctx_take_errors(ws_context *ctx);
// every entry point that takes a map looks at the verdict of the scan in flight first (settle_tsdf, tsdf_update.hip: the host logic of the scatter)
#define WS_SETTLE(map_ptr)                                                   \
  do                                                                         \
  {                                                                          \
    ws::servers_leave((map_ptr)->ctx);                                       \
    const int rc_settle__ = ws::settle_tsdf(const_cast<ws_map *>(map_ptr));  \
    if (rc_settle__ != WS_OK) return rc_settle__;                            \
  } while (0)

inline void copy3(int32_t dst[3], const int32_t src[3])
{
  dst[0] = src[0];
  dst[1] = src[1];
  dst[2] = src[2];
}

// ---- api_map.hip: the sticky device error word of a map, the box rules, the plan and the axis step of a shift
int map_take_error(ws_map *m);
int resolve_box(const ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], bool allow_whole, const char *name, int32_t l[3], int32_t ext[3]);
int plan_shift(const int32_t size[3], const int32_t pos0[3], const int32_t offset0[3], const int32_t new_pos[3], const char *name, ws_shift_plan_t *out);
void move_axis(MapParams par[2], int axis, int32_t d);

// ---- api_query.hip: the parts of the query cores that are no templates
int query_timing(hipStream_t s, QueryTimer &t, int32_t enable, float *ms_out, const int (*pairs)[2], int n);
int mesh_corners_fit(const int32_t lo[3], const int32_t hi[3], int32_t res, const char *name);
int mesh_publish(MeshResult &q, size_t nv, size_t nf, size_t *n_vertices, size_t *n_faces);
const void *surface_records_dev(const SurfResult *q, size_t *n);
const float *surface_marker_dev(const SurfResult *q, size_t *n);
int surface_download(const SurfResult &q, hipStream_t s, const char *name, const char *call, void *records_host, float *marker_host, size_t capacity_points,
                     size_t *n_out);
const void *mesh_vertices_dev(const MeshResult *q, size_t *n);
const uint32_t *mesh_faces_dev(const MeshResult *q, size_t *n);
int mesh_download(const MeshResult &q, hipStream_t s, void *vertices_host, uint32_t *faces_host, size_t cap_vertices, size_t cap_faces, size_t *n_vertices,
                  size_t *n_faces);
const void *raycast_records_dev(const RayResult *q, size_t *n);
const int32_t *raycast_gradient_dev(const RayResult *q, size_t *n);
int raycast_download(const RayResult &q, hipStream_t s, const char *name, const char *call, void *records_host, int32_t *gradient_host, size_t capacity_rays,
                     size_t *n_out);
const void *sample_records_dev(const SampleResult *q, size_t *n);
const int32_t *sample_gradient_dev(const SampleResult *q, size_t *n);
const int32_t *sample_selected_dev(const SampleResult *q, size_t *n);
int sample_download(const SampleResult &q, hipStream_t s, const char *name, const char *call, void *records_host, int32_t *gradient_host, int32_t *selected_host,
                    size_t capacity_points, size_t capacity_selected, size_t *n_out, size_t *n_selected);
const uint32_t *distance_dev(const DistResult *q, size_t *n);
int distance_download(const DistResult &q, hipStream_t s, uint32_t *host, size_t capacity, size_t *n_out);
// the event pairs of ws_debug_*_timing (QueryTimer::read)
constexpr int SURF_PAIRS[3][2] = {{0, 1}, {1, 2}, {3, 4}}, MESH_PAIRS[3][2] = {{0, 1}, {1, 2}, {3, 4}}, RAY_PAIRS[3][2] = {{0, 1}, {1, 2}, {2, 3}}, SAMPLE_PAIRS[3][2] = {{0, 1}, {1, 2}, {2, 3}}, DIST_PAIRS[4][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}};

// ---- api_store.hip: the directory, the segments and the slot-table ring, for the calls that create chunks or take a slot table
// (api_store_pair.hip, api_pack.hip).  The caller holds the store's lock.  (StoreKey and the chunk list: ws_store_list.h)
int store_make_room(ws_store *st, uint64_t fresh, const char *name); // room for `fresh` more chunks: WS_ERR_CAPACITY beyond max_chunks, segments where they are missing (which waits for the stream)
uint32_t store_take_slot(ws_store *st);                              // (store_make_room has been asked)
void store_evict(ws_store *st, const std::set<StoreKey> &fresh);     // the chunks of `fresh` leave the directory, their slots are free again
int store_table(ws_store *st, size_t n, ws_store::Table **out);      // the next slot table of the ring, for n words
uint32_t *store_slot_ptr(const ws_store *st, uint32_t slot);         // the 64^3 words of a slot

// ---- api_store_query.hip: the box, the list and the chunk tables of a call that reads a store, for the calls over two stores too
// (api_store_pair.hip).  But for store_box_refuse the caller holds the store's lock.
int store_box_refuse(const char *name, const int32_t lo[3], const int32_t hi[3]);                             // a box whose hi < lo, in the name of the entry point
void store_box_of(const ws_store *st, const int32_t lo[3], const int32_t hi[3], bool everything, int32_t l[3], int32_t h[3]); // the call's box, or the default without one
void store_list(const ws_store *st, const int32_t *lo, const int32_t *hi, std::vector<StoreRaySlot> &listed); // the written chunks the box overlaps (all without one), ascending
int store_enqueued(const ws_store *st, int rc);                                                               // waits for the stream after a failed enqueue, whose error it returns
// the tables of a call over the listed chunks into host (dev: its twin): the word-space tables, then the neighbour positions at n_off offsets; bytes(n): their size
int store_chunk_tables(ws_store *st, HostBlock &host, DevBuf &dev, const std::vector<StoreRaySlot> &listed, size_t (*bytes)(size_t), const int32_t (*off)[3], int n_off);
// a ws_debug_store_*_timing entry point: the timer of the result holder `q` of the store
template <typename Q, int N> int store_timing(ws_store *st, const char *name, Q ws_store::*q, int32_t enable, float *ms_out, const int (&pairs)[N][2])
{
  if (!st) return invalid(std::string(name) + ": store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, (st->*q).timer, enable, ms_out, pairs, N);
}

// ---- surface cloud, mesh, ray cast and distance field: one host core each for the window of a map (map_surface.hip, map_mesh.hip,
// map_raycast.hip, map_distance.hip) and for the chunks of the store (store_surface.hip, store_mesh.hip, store_raycast.hip,
// store_distance.hip).  An entry point checks what is its own, takes
// its lock and hands the shared flow its result holder, its stream and, as lambdas, the launchers of its source; `name` starts the
// refusal texts.

// The flow of a surface call whose count pass leaves `blocks` workgroup totals, from the scratch to the publish.  own_room: the source
// has scratch of its own that must grow; grow() grows it (the stream has been synchronised then).  count() enqueues the count pass
// and the scan, emit(cap) the emit pass, which writes no record at or beyond `cap`; both return at once.
// sized(total): the caller's word on the counted total before any output is sized from it (a refusal leaves an empty result).
template <typename Grow, typename Count, typename Emit, typename Sized>
int surface_run(SurfResult &q, hipStream_t s, size_t blocks, bool marker, size_t *n_out, bool own_room, Grow grow, Count count, Emit emit, Sized sized)
{
  WS_TRY(q.total.alloc(1));
  if (own_room || blocks > q.blk_tot.cap || blocks > q.blk_off.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(grow());
    WS_TRY(q.blk_tot.grow(blocks, sizeof(uint32_t)));
    WS_TRY(q.blk_off.grow(blocks, sizeof(unsigned long long)));
  }
  q.n = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  q.has_marker = false;
  WS_TRY(count());
  WS_HIP(hipStreamSynchronize(s)); // the one host read the call needs: the output is sized from the counted total
  const size_t total = (size_t)*q.total.host;
  WS_TRY(sized(total));
  WS_TRY(q.rec.grow(total, 16));
  if (marker) WS_TRY(q.marker.grow(total, 7 * sizeof(float)));
  if (total)
  {
    WS_TRY(emit(marker ? std::min(q.rec.cap, q.marker.cap) : q.rec.cap)); // (the kernel's bound holds for both buffers)
    WS_HIP(hipStreamSynchronize(s));
  }
  q.n = total;
  q.has_marker = marker;
  if (n_out) *n_out = total;
  return WS_OK;
}

template <typename Grow, typename Count, typename Emit>
int surface_run(SurfResult &q, hipStream_t s, size_t blocks, bool marker, size_t *n_out, bool own_room, Grow grow, Count count, Emit emit)
{
  return surface_run(q, s, blocks, marker, n_out, own_room, grow, count, emit, [](size_t) { return (int)WS_OK; });
}

// The flow of a mesh call over `n_words` words (< 2^31), from "the old result is dropped" to the publish.  count() and emit() enqueue
// the passes of the source and return at once; what a source owes its caller after a failed enqueue is theirs (store_enqueued).
template <typename Count, typename Emit>
int mesh_run(MeshResult &q, hipStream_t s, const char *name, uint64_t n_words, size_t *n_vertices, size_t *n_faces, Count count, Emit emit)
{
  mesh_publish(q, 0, 0, n_vertices, n_faces); // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  WS_TRY(q.total.alloc(2, false));
  const size_t need = mesh_scratch_bytes(n_words);
  if (need > q.scratch.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.scratch.grow(need, 1));
  }
  WS_TRY(count());
  WS_HIP(hipStreamSynchronize(s)); // the one host read the call needs: the outputs are sized from the two totals
  const unsigned long long nv = q.total.host[0], nq = q.total.host[1];
  if (nv > 0xffffffffull) return range_error(name, ": more than 2^32 - 1 vertices");
  WS_TRY(q.vert.grow((size_t)nv, 16));
  WS_TRY(q.face.grow((size_t)nq * 2, 12));
  if (nv)
  {
    WS_TRY(emit());
    WS_HIP(hipStreamSynchronize(s));
  }
  return mesh_publish(q, (size_t)nv, (size_t)nq * 2, n_vertices, n_faces);
}

// The argument check of a ray cast.  `bad`: what the entry point found wrong with its own leading arguments; more(): its further
// checks, which come before those of the ranges.
template <typename More>
int raycast_check(const char *name, bool bad, const int32_t *origin, const int32_t *dirs, size_t n, int32_t max_range, int32_t res, uint32_t flags, More more)
{
  const uint32_t known = WS_RAYCAST_ANY_WEIGHT | WS_RAYCAST_GRADIENT | WS_RAYCAST_TARGETS;
  if (bad || (flags & ~known) || !origin || (n && !dirs)) return invalid(std::string(name) + ": bad argument");
  WS_TRY(more());
  if (max_range <= 0) return invalid(std::string(name) + ": max_range_mm <= 0");
  if (res > 1024) return range_error(name, ": the resolution must not exceed 1024 mm (the interpolant is carried times res^3 in 64 bits)");
  if (n > ((size_t)1 << 27)) return range_error(name, ": more than 2^27 rays");
  for (int k = 0; k < 3; ++k)
  {
    const int64_t o = origin[k];
    if ((o < 0 ? -o : o) + (int64_t)max_range + 2 * (int64_t)res > (int64_t)INT32_MAX) return range_error(name, ": |origin| + max_range + 2 res does not fit int32");
  }
  return WS_OK;
}

// The flow of a ray cast whose arguments have passed raycast_check: arm, drop the old result, grow, upload the directions, launch,
// synchronise, publish.  own_room: the source has buffers of its own that must grow; prepare() grows them (the stream has been
// synchronised then) and fills them; launch(directions on the device) enqueues the passes of the source, like count() of mesh_run.
template <typename Prepare, typename Launch>
int raycast_run(RayResult &q, hipStream_t s, const int32_t *dirs, bool dirs_on_host, size_t n, uint32_t flags, size_t *n_hits, bool own_room, Prepare prepare,
                Launch launch)
{
  WS_TRY(q.timer.arm());
  if (n_hits) *n_hits = 0;
  q.n = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  q.has_grad = false;
  if (n == 0) return WS_OK;
  const bool grad = (flags & WS_RAYCAST_GRADIENT) != 0;
  WS_TRY(q.hits.alloc(1));
  if (n > q.rec.cap || (grad && n > q.grad.cap) || (dirs_on_host && n > q.dirs.cap) || own_room)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.rec.grow(n, 16));
    if (grad) WS_TRY(q.grad.grow(n, 3 * sizeof(int32_t)));
    if (dirs_on_host) WS_TRY(q.dirs.grow(n, 3 * sizeof(int32_t)));
  }
  WS_TRY(prepare());
  q.timer.mark(0, s);
  if (dirs_on_host)
  {
    WS_HIP(hipMemcpyAsync(q.dirs.p, dirs, n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    dirs = static_cast<const int32_t *>(q.dirs.p);
  }
  WS_TRY(launch(dirs));
  WS_HIP(hipStreamSynchronize(s));
  q.n = n;
  q.has_grad = grad;
  if (n_hits) *n_hits = (size_t)*q.hits.host;
  return WS_OK;
}

// The argument check of a point sample.  `bad`: what the entry point found wrong with its own leading arguments; more(): its further
// checks, which come before those of the ranges.
template <typename More> int sample_check(const char *name, bool bad, const int32_t *points, size_t n, int32_t res, uint32_t flags, More more)
{
  const uint32_t known = WS_SAMPLE_ANY_WEIGHT | WS_SAMPLE_GRADIENT | WS_SAMPLE_SELECT_UNKNOWN | WS_SAMPLE_SELECT_FREE | WS_SAMPLE_SELECT_SURFACE | WS_SAMPLE_SELECT_INSIDE;
  if (bad || (flags & ~known) || (n && !points)) return invalid(std::string(name) + ": bad argument");
  WS_TRY(more());
  if (res > 1024) return range_error(name, ": the resolution must not exceed 1024 mm (the interpolant is carried times res^3 in 64 bits)");
  if (n > ((size_t)1 << 27)) return range_error(name, ": more than 2^27 points");
  return WS_OK;
}

// The flow of a point sample whose arguments have passed sample_check: arm, drop the old result, grow, upload the points, launch,
// synchronise, publish.  own_room, prepare() and launch(points on the device) are those of raycast_run.  The selection is sized for
// every point of the call, so nothing is read back before the one synchronise at the end.
template <typename Prepare, typename Launch>
int sample_run(SampleResult &q, hipStream_t s, const int32_t *points, bool points_on_host, size_t n, uint32_t flags, uint64_t counts[4], bool own_room,
               Prepare prepare, Launch launch)
{
  WS_TRY(q.timer.arm());
  if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
  q.n = q.n_sel = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  q.has_grad = q.has_sel = false;
  if (n == 0) return WS_OK;
  const bool grad = (flags & WS_SAMPLE_GRADIENT) != 0;
  const uint32_t select = (flags / WS_SAMPLE_SELECT_UNKNOWN) & 15u;
  const size_t blocks = (n + 255) / 256; // (SAMPLE_WG, ws_sample.h)
  WS_TRY(q.counts.alloc(5));
  if (n > q.rec.cap || (grad && n > q.grad.cap) || (points_on_host && n > q.pts.cap) || (select && (n > q.sel.cap || blocks > q.blk_tot.cap || blocks > q.blk_off.cap)) ||
      own_room)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.rec.grow(n, 16));
    if (grad) WS_TRY(q.grad.grow(n, 3 * sizeof(int32_t)));
    if (points_on_host) WS_TRY(q.pts.grow(n, 3 * sizeof(int32_t)));
    if (select)
    {
      WS_TRY(q.sel.grow(n, 3 * sizeof(int32_t)));
      WS_TRY(q.blk_tot.grow(blocks, sizeof(uint32_t)));
      WS_TRY(q.blk_off.grow(blocks, sizeof(unsigned long long)));
    }
  }
  WS_TRY(prepare());
  q.timer.mark(0, s);
  if (points_on_host)
  {
    WS_HIP(hipMemcpyAsync(q.pts.p, points, n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    points = static_cast<const int32_t *>(q.pts.p);
  }
  WS_TRY(launch(points));
  WS_HIP(hipStreamSynchronize(s));
  q.n = n;
  q.has_grad = grad;
  q.has_sel = select != 0;
  for (int c = 0; c < 4; ++c)
  {
    if (counts) counts[c] = q.counts.host[c];
    if ((select >> c) & 1u) q.n_sel += (size_t)q.counts.host[c];
  }
  return WS_OK;
}

// The argument check of a distance call.  `bad`: what the entry point found wrong with its own leading arguments; box(e): its lock and
// its box, which come behind the checks of the flags and of R -- the extents in 64 bits, all zero for "nothing to do".  ext and *n
// receive the extents the passes take and the number of records.
template <typename Box>
int distance_check(const char *name, bool bad, const int32_t *lo, const int32_t *hi, int32_t R, uint32_t flags, Box box, uint32_t ext[3], size_t *n)
{
  const uint32_t known = WS_DISTANCE_ANY_WEIGHT | WS_DISTANCE_UNKNOWN_OCCUPIED | WS_DISTANCE_COLUMNS;
  if (bad || (flags & ~known) || ((lo == nullptr) != (hi == nullptr))) return invalid(std::string(name) + ": bad argument");
  if (R < 1 || R > 255) return range_error(name, ": max_dist_vox must be 1 .. 255 (its square is carried in 16 bits)");
  uint64_t e[3] = {0, 0, 0};
  WS_TRY(box(e));
  const bool columns = (flags & WS_DISTANCE_COLUMNS) != 0;
  // (every extent is at most 2^32; one of 2^32 is too many records by itself, and the products of the others fit 64 bits)
  const uint64_t n_cols = e[0] > 0xffffffffull || e[1] > 0xffffffffull ? ~0ull : e[0] * e[1];
  if (n_cols > 0xffffffffull || (!columns && n_cols * e[2] > 0xffffffffull)) return range_error(name, ": more than 2^32 - 1 records");
  if ((columns ? e[1] : e[2]) > (uint64_t)DIST_MAX_LINE) return range_error(name, ": more than 16 776 960 voxels along the fastest axis of the records");
  for (int k = 0; k < 3; ++k) ext[k] = (uint32_t)std::min<uint64_t>(e[k], 0xffffffffull); // (under COLUMNS the passes do not read ext[2])
  *n = (size_t)(columns ? n_cols : n_cols * e[2]);
  return WS_OK;
}

// The flow of a distance call whose arguments have passed distance_check, from "the old result is dropped" to the publish.  pass0()
// enqueues the source's classification into q.rec and the first plane of q.plane and returns at once.
template <typename Pass0>
int distance_run(DistResult &q, hipStream_t s, const int32_t lo[3], const uint32_t ext[3], int32_t R, uint32_t flags, size_t n, size_t *n_sites, Pass0 pass0)
{
  if (n_sites) *n_sites = 0;
  q.n = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  q.have = false;
  // what a reach call needs of this result beside its records: the box and the flags (published with `have`)
  for (int k = 0; k < 3; ++k) q.lo[k] = n ? lo[k] : 0, q.ext[k] = n ? ext[k] : 0u;
  q.flags = flags;
  q.R = R;
  if (n == 0)
  {
    q.have = true;
    return WS_OK;
  }
  WS_TRY(q.sites.alloc(1));
  if (n > q.rec.cap || n > q.plane.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.rec.grow(n, sizeof(uint32_t)));
    WS_TRY(q.plane.grow(n, 2 * sizeof(uint16_t))); // both planes
  }
  WS_TRY(pass0());
  WS_TRY(dist_passes(s, q.timer, q.rec.as<uint32_t>(), q.plane.as<uint16_t>(), ext, R, flags));
  WS_TRY(q.sites.fetch(s));
  WS_HIP(hipStreamSynchronize(s));
  q.n = n;
  q.have = true;
  if (n_sites) *n_sites = (size_t)*q.sites.host;
  return WS_OK;
}

// ---- ground (map_ground.hip for the window of a map, store_ground.hip for the chunks of the store): the checks and the flow of a
// ground call, `bad` and box(e) as for distance_check, and the check of the bridge to the distance field, whose flow is distance_run.
const void *ground_dev(const GroundResult *q, size_t *n);
int ground_download(const GroundResult &q, hipStream_t s, void *host, size_t capacity, size_t *n_out);
int ground_box(const GroundResult &q, const char *name, int32_t lo[3], uint32_t ext[3]);
constexpr int GROUND_PAIRS[2][2] = {{0, 1}, {1, 2}};

template <typename Box>
int ground_check(const char *name, bool bad, const int32_t *lo, const int32_t *hi, int32_t clear_vox, uint32_t flags, Box box, uint32_t ext[3], size_t *n)
{
  const uint32_t known = WS_GROUND_ANY_WEIGHT | WS_GROUND_UNKNOWN_HEADROOM | WS_GROUND_TOP;
  if (bad || (flags & ~known) || ((lo == nullptr) != (hi == nullptr))) return invalid(std::string(name) + ": bad argument");
  if (clear_vox < 1 || clear_vox > GROUND_MAX_CLEAR) return range_error(name, ": clear_vox must be 1 .. 64 (a step of the column walk carries one 64-bit word of the step above)");
  uint64_t e[3] = {0, 0, 0};
  WS_TRY(box(e));
  const uint64_t n_cols = e[0] > 0xffffffffull || e[1] > 0xffffffffull ? ~0ull : e[0] * e[1];
  if (n_cols > 0xffffffffull) return range_error(name, ": more than 2^32 - 1 columns");
  for (int k = 0; k < 3; ++k) ext[k] = (uint32_t)std::min<uint64_t>(e[k], 0xffffffffull);
  *n = e[2] ? (size_t)n_cols : 0;
  return WS_OK;
}

// The flow of a ground call whose arguments have passed ground_check, from "the old result is dropped" to the publish.  pass1()
// enqueues the source's levels into q.lvl and returns at once.
template <typename Pass1> int ground_run(GroundResult &q, hipStream_t s, const int32_t lo[3], const uint32_t ext[3], size_t n, uint64_t counts[4], Pass1 pass1)
{
  if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
  q.n = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  q.have = false;
  for (int k = 0; k < 3; ++k) q.lo[k] = n ? lo[k] : 0, q.ext[k] = n ? ext[k] : 0u;
  if (n == 0)
  {
    q.have = true;
    return WS_OK;
  }
  WS_TRY(q.counts.alloc(4));
  if (n > q.lvl.cap || n > q.rec.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.lvl.grow(n, 8));
    WS_TRY(q.rec.grow(n, 8));
  }
  WS_TRY(pass1());
  WS_TRY(ground_steps(s, q, ext[0], ext[1]));
  WS_TRY(q.counts.fetch(s, 4));
  WS_HIP(hipStreamSynchronize(s));
  q.n = n;
  q.have = true;
  for (int c = 0; c < 4 && counts; ++c) counts[c] = (uint64_t)q.counts.host[c];
  return WS_OK;
}

// The argument check of ws_*_ground_distance: its own refusals, then those of a distance call under WS_DISTANCE_COLUMNS.  box(e):
// the locks, the look at the ground result ("none yet" is the entry point's refusal) and its extents.
template <typename Box>
int ground_distance_check(const char *name, bool bad, int32_t max_step_q8, int32_t R, uint32_t flags, Box box, uint32_t ext[3], size_t *n)
{
  if (bad || (flags & ~WS_DISTANCE_UNKNOWN_OCCUPIED)) return invalid(std::string(name) + ": bad argument");
  if (max_step_q8 < 0 || max_step_q8 > 65535) return range_error(name, ": max_step_q8 must be 0 .. 65535 (the step of a ground record)");
  return distance_check(name, false, nullptr, nullptr, R, flags | WS_DISTANCE_COLUMNS, box, ext, n);
}

// ---- frontier (map_frontier.hip for the window of a map, store_frontier.hip for the chunks of the store): its extraction is the
// flow of a surface call, its clustering works on the records alone.  frontier_check: the refusals that come before the lock and the
// box, `bad` as above.  frontier_run: grow(), count() and emit(cap) are those of surface_run.
int frontier_check(const char *name, bool bad, const int32_t *lo, const int32_t *hi, int32_t min_value, uint32_t flags);
const uint32_t *frontier_labels_dev(const FrontierResult *q, size_t *n);
const void *frontier_clusters_dev(const FrontierResult *q, size_t *n);
int frontier_download(const FrontierResult &q, hipStream_t s, const char *name, const char *call, void *records_host, uint32_t *labels_host, void *clusters_host,
                      size_t cap_records, size_t cap_clusters, size_t *n_out, size_t *n_clusters);
int frontier_publish(FrontierResult &q, size_t n, size_t k, bool clusters, size_t *n_out, size_t *n_clusters);
constexpr int FRONTIER_PAIRS[4][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};

template <typename Grow, typename Count, typename Emit>
int frontier_run(FrontierResult &q, hipStream_t s, const char *name, size_t blocks, uint32_t flags, size_t *n_out, size_t *n_clusters, bool own_room, Grow grow,
                 Count count, Emit emit)
{
  const bool clusters = (flags & WS_FRONTIER_CLUSTERS) != 0;
  frontier_publish(q, 0, 0, false, n_out, n_clusters); // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  WS_TRY(surface_run(q, s, blocks, false, nullptr, own_room, grow, count, emit, [&](size_t total) {
    // (before the record buffer grows: q.n is 0 here, the refusal leaves an empty result and allocates nothing)
    if (clusters && total > 0x7fffffffull) return range_error(name, ": more than 2^31 - 1 records under WS_FRONTIER_CLUSTERS");
    return (int)WS_OK;
  }));
  const size_t n = q.n;
  if (clusters && n)
  {
    q.n = 0;
    WS_TRY(frontier_clusters(q, s, n));
  }
  return frontier_publish(q, n, clusters ? q.n_clusters : 0, clusters, n_out, n_clusters);
}

// ---- reach (map_reach.hip): the geodesic field over the records of a distance result.  The window of a map and the store differ in
// nothing but their locks.  reach_run: enter() settles the
// owner and takes its locks -- behind the refusals that need neither, in front of the look at the distance result.  The others are no
// templates (api_query.hip): their callers hold the lock.
const uint32_t *reach_dev(const ReachResult *q, size_t *n);
int reach_box(const ReachResult &q, int32_t lo[3], uint32_t ext[3], int32_t *columns);
int reach_download(const ReachResult &q, hipStream_t s, uint32_t *host, size_t capacity, size_t *n_out);
int reach_lookup(ReachResult &q, hipStream_t s, const char *name, const int32_t *points, bool on_host, size_t n, int32_t stride, uint32_t *cost);
int reach_paths(ReachResult &q, hipStream_t s, const char *name, const int32_t *goals_host, size_t g, uint32_t cap_steps, void *headers_host, void *records_host);
int reach_rounds(ReachResult &q, const DistResult &d, hipStream_t s, const char *name, const int32_t *seeds, size_t n_seeds, int32_t clear_d2, uint32_t flags,
                 uint32_t max_rounds, size_t *n_seeded, size_t *n_reached, uint32_t *rounds);
constexpr int REACH_PAIRS[3][2] = {{0, 1}, {1, 2}, {2, 3}};

template <typename Enter>
int reach_run(ReachResult &q, const DistResult &d, hipStream_t s, const char *name, const int32_t *seeds, size_t n_seeds, int32_t clear_d2, uint32_t flags,
              uint32_t max_rounds, size_t *n_seeded, size_t *n_reached, uint32_t *rounds, Enter enter)
{
  if ((flags & ~WS_REACH_UNKNOWN_FREE) || !seeds || n_seeds == 0 || n_seeds > ((size_t)1 << 20)) return invalid(std::string(name) + ": bad argument");
  if (clear_d2 < 0 || clear_d2 > 65025) return range_error(name, ": clear_d2 must be 0 .. 65025 (255 squared, the largest d2 of a distance record)");
  WS_TRY(enter());
  if (!d.have) return invalid(std::string(name) + ": no distance result yet (the reach runs on the records of the last distance call)");
  return reach_rounds(q, d, s, name, seeds, n_seeds, clear_d2, flags, max_rounds, n_seeded, n_reached, rounds);
}

// ---- view gain (map_gain.hip for the window of a map, store_gain.hip for the chunks of the store).  gain_check: every refusal that
// needs neither a lock nor the box, `bad` and more() as above; among these the INVALID ones come first.  The box's own refusals (outside
// the window, more voxels than the ring holds) follow under the lock, behind the ranges, as in ws_map_frontier.  gain_run: the flow of a checked call with
// m, n > 0, from "the old result is dropped" to the publish; own_room, prepare() and launch() are those of raycast_run.
const void *gain_records_dev(const GainResult *q, size_t *n);
const void *gain_rays_dev(const GainResult *q, size_t *n);
int gain_download(const GainResult &q, hipStream_t s, const char *name, const char *call, void *records_host, void *rays_host, size_t cap_views, size_t cap_rays,
                  size_t *n_views, size_t *n_rays);
constexpr int GAIN_PAIRS[3][2] = {{0, 1}, {1, 2}, {2, 3}};

template <typename More>
int gain_check(const char *name, bool bad, const int32_t *lo, const int32_t *hi, const int32_t *origins, size_t m, const int32_t *dirs, size_t n, int32_t max_range,
               int32_t min_value, int32_t res, uint32_t flags, const uint64_t *best, More more)
{
  const uint32_t known = WS_GAIN_ANY_WEIGHT | WS_GAIN_RAYS;
  if (bad || (flags & ~known) || ((lo == nullptr) != (hi == nullptr)) || (m && !origins) || (n && !dirs)) return invalid(std::string(name) + ": bad argument");
  if (max_range <= 0) return invalid(std::string(name) + ": max_range_mm <= 0");
  if (m == 0 && best) return invalid(std::string(name) + ": no view, but a result is asked for");
  WS_TRY(more());
  if (min_value < 0 || min_value > 32767) return range_error(name, ": min_value must be 0 .. 32767 (a raw int16 value; 0: any non-negative value)");
  if (res > 1024) return range_error(name, ": the resolution must not exceed 1024 mm");
  if (max_range / (res / 2 > 1 ? res / 2 : 1) > 8191) return range_error(name, ": more than 8192 samples per ray (max_range / step > 8191)");
  if (n > ((size_t)1 << 19)) return range_error(name, ": more than 2^19 rays in the fan");
  if (m > 65535) return range_error(name, ": more than 65535 views");
  if ((flags & WS_GAIN_RAYS) && m * n > ((size_t)1 << 27)) return range_error(name, ": more than 2^27 ray records under WS_GAIN_RAYS");
  for (size_t j = 0; j < 3 * m; ++j)
  {
    const int64_t o = origins[j];
    if ((o < 0 ? -o : o) + (int64_t)max_range + 2 * (int64_t)res > (int64_t)INT32_MAX) return range_error(name, ": |origin| + max_range + 2 res does not fit int32");
  }
  return WS_OK;
}

template <typename Prepare, typename Launch>
int gain_run(GainResult &q, hipStream_t s, const GainCall &c, const int32_t *origins, const int32_t *dirs, uint64_t *best, bool own_room, Prepare prepare, Launch launch)
{
  WS_TRY(q.timer.arm());
  q.m = q.n = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  q.has_rays = false;
  const bool rays = (c.flags & WS_GAIN_RAYS) != 0;
  WS_TRY(q.best.alloc(1));
  if (c.m > q.org.cap || c.m > q.rec.cap || c.n > q.dirs.cap || c.n > q.prep.cap || (rays && c.m * c.n > q.rays.cap) || own_room)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.org.grow(c.m, 3 * sizeof(int32_t)));
    WS_TRY(q.rec.grow(c.m, 32));
    WS_TRY(q.dirs.grow(c.n, 3 * sizeof(int32_t)));
    WS_TRY(q.prep.grow(c.n, 32));
    if (rays) WS_TRY(q.rays.grow(c.m * c.n, 8));
  }
  WS_TRY(prepare());
  q.timer.mark(0, s);
  WS_HIP(hipMemcpyAsync(q.org.p, origins, c.m * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  WS_HIP(hipMemcpyAsync(q.dirs.p, dirs, c.n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  WS_TRY(launch());
  WS_HIP(hipStreamSynchronize(s));
  q.m = c.m, q.n = c.n;
  q.has_rays = rays;
  if (best) *best = (uint64_t)*q.best.host;
  return WS_OK;
}

// ---- clearance (map_clearance.hip): trajectories of a body of spheres against the records of a distance result.  The window of a map
// and the store differ in their locks and in where the resolution comes from.  clearance_run: the refusals that need no lock, then
// enter() settles the owner and takes its locks, then clearance_flow (api_query.hip): the look at the distance result, its refusal, and
// the flow from "the old result is dropped" to the publish.
const void *clearance_records_dev(const ClearanceResult *q, size_t *n);
const void *clearance_poses_dev(const ClearanceResult *q, size_t *n);
int clearance_download(const ClearanceResult &q, hipStream_t s, const char *name, const char *call, void *records_host, void *poses_host, size_t cap_traj,
                       size_t cap_poses, size_t *n_traj, size_t *n_poses);
int clearance_check(const char *name, bool bad, const int32_t *poses, size_t t, size_t p, const int32_t *body, size_t k, int32_t soft, int32_t res, uint32_t flags,
                    int32_t *reach_mm);
int clearance_flow(ClearanceResult &q, const DistResult &d, hipStream_t s, const char *name, const int32_t *poses, bool poses_on_host, size_t t, size_t p,
                   const int32_t *body, size_t k, int32_t soft, int32_t res, uint32_t flags, int32_t reach_mm, int64_t *best);
constexpr int CLEAR_PAIRS[3][2] = {{0, 1}, {1, 2}, {2, 3}};

template <typename Enter>
int clearance_run(ClearanceResult &q, const DistResult &d, hipStream_t s, const char *name, bool bad, const int32_t *poses, bool poses_on_host, size_t t, size_t p,
                  const int32_t *body, size_t k, int32_t soft, int32_t res, uint32_t flags, int64_t *best, Enter enter)
{
  int32_t reach_mm = 0; // the largest radius + soft_mm: how far a penalty looks
  WS_TRY(clearance_check(name, bad, poses, t, p, body, k, soft, res, flags, &reach_mm));
  WS_TRY(enter());
  return clearance_flow(q, d, s, name, poses, poses_on_host, t, p, body, k, soft, res, flags, reach_mm, best);
}

// ---- map shift: one shift of both maps' windows, for ws_shift_begin (api_map.hip) and ws_shift_device (api_store.hip), which
// differ in what happens to a slab that leaves and to one that enters.  `name` is the entry point and `open_text` its words for a
// ticket in flight.  After the shared refusals and the plan (into `plan`): ready() before the first launch; per step leave(i, par),
// the axis step, enter(i, par), on a COPY of the parameters (the box kernels take them by value); done() behind the last step.  The
// copy is committed only when all of it has been enqueued: the first error is returned with the host's view of both maps as it was
// (ADVICE r2).
template <class Ready, class Leave, class Enter, class Done>
int run_shift(ws_map *m, const int32_t new_pos[3], const char *name, const char *open_text, ws_shift_plan_t &plan, Ready ready, Leave leave,
              Enter enter, Done done)
{
  WS_SETTLE(m);
  if (m->shift_open) return invalid((std::string(name) + open_text).c_str());
  // only new_map's WINDOW moves (DeviceMapMemWrapper::update_params), which is right iff it holds (tau, 0) everywhere -- not between
  // ws_tsdf_scatter_dev and ws_tsdf_integrate, nor for a map created from non-default host data that has not been integrated yet
  if (!m->new_is_default)
    return invalid((std::string(name) + ": new_map holds entries that have not been integrated (ws_tsdf_integrate first)").c_str());
  const MapParams &p0 = m->par[WS_MAP_AVG];
  WS_TRY(plan_shift(p0.size, p0.pos, p0.offset, new_pos, name, &plan));
  WS_TRY(ready());
  MapParams par[2] = {m->par[0], m->par[1]};
  int rc = WS_OK;
  for (int i = 0; i < plan.n && rc == WS_OK; ++i)
  {
    rc = leave(i, par[WS_MAP_AVG]);
    move_axis(par, plan.axis[i], plan.d[i]);
    if (rc == WS_OK) rc = enter(i, par[WS_MAP_AVG]);
  }
  if (rc == WS_OK) rc = done();
  if (rc == WS_OK) m->par[0] = par[0], m->par[1] = par[1];
  return rc;
}
} // namespace ws
