// api.hip — the extern "C" surface of libwarpsense_hip.so (include/warpsense_hip.h): handle
// management, host<->HBM transfers, stream ordering and hipEvent profiling.  No kernels here.
#include <cmath>
#include <chrono>
#include <atomic>
#include <algorithm>
#include <array>
#include <cstring>
#include <new>
#include <set>

#include "ws_internal.h"

namespace ws
{
static thread_local std::string g_last_error;

void set_error(const std::string &msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
  char buf[512];
  snprintf(buf, sizeof buf, "HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
  set_error(buf);
  return WS_ERR_HIP;
}

static int invalid(const char *msg)
{
  set_error(msg);
  return WS_ERR_INVALID;
}
static int invalid(const std::string &msg) { return invalid(msg.c_str()); }

static hipEvent_t take_event(ws_context *ctx)
{
  if (!ctx->pool.empty())
  {
    hipEvent_t e = ctx->pool.back();
    ctx->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void prof_begin(ws_context *ctx, int cls)
{
  if (!(ctx->prof_mask & (1u << cls))) return;
  ws_context::Span sp;
  sp.a = take_event(ctx);
  sp.b = take_event(ctx);
  sp.cls = cls;
  (void)hipEventRecord(sp.a, ctx->stream);
  ctx->spans.push_back(sp);
}

void prof_end(ws_context *ctx, int cls)
{
  if (!(ctx->prof_mask & (1u << cls))) return;
  for (size_t i = ctx->spans.size(); i-- > 0;)
  {
    if (ctx->spans[i].cls == cls)
    {
      (void)hipEventRecord(ctx->spans[i].b, ctx->stream);
      return;
    }
  }
}

static void prof_resolve(ws_context *ctx)
{
  for (auto &sp : ctx->spans)
  {
    float ms = 0.f;
    if (hipEventSynchronize(sp.b) == hipSuccess && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess)
    {
      ctx->prof_ms[sp.cls] += ms;
      ctx->prof_n[sp.cls] += 1;
    }
    ctx->pool.push_back(sp.a);
    ctx->pool.push_back(sp.b);
  }
  ctx->spans.clear();
}

int check_all_equal_host(const uint32_t *data, int64_t n, uint32_t value)
{
  for (int64_t i = 0; i < n; ++i)
    if (data[i] != value) return 0;
  return 1;
}

static void copy3(int32_t dst[3], const int32_t src[3])
{
  dst[0] = src[0];
  dst[1] = src[1];
  dst[2] = src[2];
}

size_t reg_partials_bytes();
} // namespace ws
static int ctx_take_errors(ws_context *ctx);
// A resident server of ws_reg_iterate (reg_server_kernel) holds the context's stream until it has been idle for 50 us: whoever
// enqueues other work there asks it to leave first (one store into host-mapped memory; the work is ordered behind the kernel
// anyway).  The next ws_reg_iterate waits until that server is really gone and starts a new one -- behind the other work.
static void servers_leave(ws_context *ctx)
{
  if (!ctx) return;
  std::lock_guard<std::mutex> lock(ctx->lists_mu);
  for (ws_reg *r : ctx->regs)
  {
    const uint32_t id = r->srv_launch.load(std::memory_order_acquire);
    if (id == 0 || ws::reg_server_mail_exited(r->srv_mail.p) == id) continue;
    ws::reg_server_mail_stop(r->srv_mail.p, id);
    r->srv_stopping.store(true, std::memory_order_release);
  }
}
// every entry point that takes a map looks at the verdict of the scan in flight first (settle_tsdf, tsdf_update.hip)
#define WS_SETTLE(map_ptr)                                                   \
  do                                                                         \
  {                                                                          \
    servers_leave((map_ptr)->ctx);                                           \
    const int rc_settle__ = ws::settle_tsdf(const_cast<ws_map *>(map_ptr));  \
    if (rc_settle__ != WS_OK) return rc_settle__;                            \
  } while (0)

namespace ws
{
constexpr size_t AZ_ALLOC = 1024 * 64 + 8; // direction-bin histogram / offsets (tsdf_update.hip: AZ_BINS + 2 entries)
} // namespace ws

using namespace ws;

// the Gauss-Newton state a registration starts from (tsdf_registration.cpp:28-33)
static GnCore gn_init(const float T_in[16], int32_t max_iterations, float it_weight_gradient, float epsilon)
{
  GnCore c;
  std::memset(&c, 0, sizeof c);
  std::memcpy(c.T, T_in, 16 * sizeof(float));
  for (int k = 0; k < 3; ++k) c.center[k] = (int32_t)T_in[12 + k]; // Point center = total_transform.block<3,1>(0,3).cast<int>()
  c.it_weight_gradient = it_weight_gradient;
  c.epsilon = epsilon;
  c.max_iterations = max_iterations;
  return c;
}

// Spin until done() -- a word a kernel writes into host-mapped memory: a microsecond or two, where waking up from
// hipStreamSynchronize costs tens.  Bounded: after 20 ms the stream is synchronised the ordinary way (a kernel that never ends
// is the runtime's to report), and if done() is still false then, the wait fails with `what`.
template <typename Done>
static int spin_wait(ws_reg *r, Done done, const char *what)
{
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spins = 0; !done();)
    if ((++spins & 0xfffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20))
    {
      WS_HIP(hipStreamSynchronize(r->ctx->stream));
      if (done()) break;
      set_error(what);
      return WS_ERR_INTERNAL;
    }
  std::atomic_thread_fence(std::memory_order_acquire);
  return WS_OK;
}

extern "C" {

const char *ws_last_error(void) { return g_last_error.c_str(); }
int ws_version(void) { return 1; }

int ws_ctx_create(int device_id, ws_context **out)
{
  if (!out) return invalid("ws_ctx_create: out is NULL");
  // the constant the kernels use for dz_per_distance must be what the reference computes (update_tsdf.cu:49-50)
  {
    float angle = 45.f / 128.f;
    int dz = (int)(std::tan(angle / 180 * M_PI) / 2.0 * MATRIX_RESOLUTION);
    if (dz != DZ_PER_DISTANCE) return invalid("ws_ctx_create: dz_per_distance constant mismatch");
  }
  if (device_id >= 0) WS_HIP(hipSetDevice(device_id));
  int dev = 0;
  WS_HIP(hipGetDevice(&dev));
  ws_context *ctx = new (std::nothrow) ws_context();
  if (!ctx) return invalid("ws_ctx_create: out of host memory");
  ctx->device = dev;
  hipError_t e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess)
  {
    delete ctx;
    return hip_fail(e, "hipStreamCreateWithFlags", __FILE__, __LINE__);
  }
  ctx->stream = ctx->own_stream;
  *out = ctx;
  return WS_OK;
}

int ws_ctx_destroy(ws_context *ctx)
{
  if (!ctx) return WS_OK;
  (void)hipStreamSynchronize(ctx->stream);
  prof_resolve(ctx);
  for (auto e : ctx->pool) (void)hipEventDestroy(e);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  return WS_OK;
}

int ws_ctx_set_stream(ws_context *ctx, void *hip_stream)
{
  if (!ctx) return invalid("ws_ctx_set_stream: ctx is NULL");
  servers_leave(ctx);
  hipStream_t next = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  // work already enqueued on the old stream finishes before anything goes to the new one -- unless one of them is
  // being captured into a graph (a synchronisation would invalidate the capture; the graph orders its own nodes)
  hipStreamCaptureStatus a = hipStreamCaptureStatusNone, b = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(ctx->stream, &a);
  (void)hipStreamIsCapturing(next, &b);
  if (a == hipStreamCaptureStatusNone && b == hipStreamCaptureStatusNone) WS_HIP(hipStreamSynchronize(ctx->stream));
  ctx->stream = next;
  return WS_OK;
}

int ws_sync(ws_context *ctx)
{
  if (!ctx) return invalid("ws_sync: ctx is NULL");
  servers_leave(ctx);
  std::vector<ws_map *> maps;
  {
    std::lock_guard<std::mutex> lock(ctx->lists_mu);
    maps = ctx->maps;
  }
  for (ws_map *m : maps)
  {
    const int rc = settle_tsdf(m); // (an aborted scan is repeated before the stream is drained)
    if (rc != WS_OK) return rc;
  }
  WS_HIP(hipStreamSynchronize(ctx->stream));
  return ctx_take_errors(ctx);
}

int ws_device_reset(void)
{
  WS_HIP(hipDeviceReset());
  return WS_OK;
}

// ------------------------------------------------------------------ maps
// candidate records of the ray tails: the pool of sub-chunks (32 x 8 bytes, one tile each) and the (tile, entry number) ->
// entry hash for tiles of more than TILE_DIRECT sub-chunks (two slots per sub-chunk of the pool; keys, then uint32 values)
static int map_alloc_records(ws_map *m, uint64_t subs)
{
  if (subs < 32768) subs = 32768;
  if (subs > SUB_ID_LIMIT) subs = SUB_ID_LIMIT;
  m->rec.release();
  m->big_keys.release();
  m->sub_cap = 0;
  m->big_slots = 0;
  uint64_t slots = 1u << 16;
  while (slots < 2 * subs && slots < (1ull << 31)) slots <<= 1;
  WS_TRY(m->rec.alloc((size_t)subs * SUB_RECS, sizeof(unsigned long long)));
  WS_TRY(m->big_keys.alloc((size_t)slots, sizeof(unsigned long long) + sizeof(uint32_t)));
  m->sub_cap = (uint32_t)subs;
  m->big_slots = (uint32_t)slots;
  m->prepped = false; // the new hash is filled by the stand-alone preparation pass
  return WS_OK;
}

static int map_free(ws_map *m)
{
  if (!m) return WS_OK;
  (void)hipStreamSynchronize(m->ctx->stream);
  if (m->shift_stream) (void)hipStreamSynchronize(m->shift_stream);
  {
    std::lock_guard<std::mutex> lock(m->ctx->lists_mu);
    for (size_t i = 0; i < m->ctx->maps.size(); ++i)
      if (m->ctx->maps[i] == m)
      {
        m->ctx->maps.erase(m->ctx->maps.begin() + (long)i);
        break;
      }
  }
  m->release();
  if (m->shift_open) delete m->shift_open;
  if (m->shift_event) (void)hipEventDestroy(m->shift_event);
  if (m->shift_stream) (void)hipStreamDestroy(m->shift_stream);
  delete m;
  return WS_OK;
}

// Device-side error bits (a ray outside the record's step / fan range, an aborted scan that was not repeated, internal
// checks) are OR-ed into a host-mapped word by the kernels.  Every entry point that has just synchronised the stream
// looks at it: an inexact map is reported ONCE, by the first such call after the update that produced it.
static int map_take_error(ws_map *m)
{
  if (!m || !m->status.p) return WS_OK;
  volatile uint32_t *st = m->status.as<uint32_t>();
  const uint32_t bits = st[0];
  if (!bits) return WS_OK;
  __atomic_fetch_and(m->status.as<uint32_t>(), ~bits, __ATOMIC_RELAXED);
  m->last_error_bits |= bits;
  if (bits & 8u)
  {
    set_error("TSDF update: internal consistency check failed on the device (record tables); the map is not exact");
    return WS_ERR_INTERNAL;
  }
  if (bits & 4u)
  {
    set_error("TSDF update: a free-space step produced a candidate that is not free space; the map is not exact");
    return WS_ERR_INTERNAL;
  }
  if (bits & 1u)
  {
    set_error("TSDF update: record capacity exceeded, a TSDF update since the last check is not exact");
    return WS_ERR_CAPACITY;
  }
  set_error("TSDF update: a ray needs more ray steps or fan steps than the key of a scan of this many points holds (outside the range of the record fields: "
            "65 536 steps / 255 fan steps for small scans, 32 768 / 63 for 131 072 points, 8192 / 31 for a million) and was dropped");
  return WS_ERR_RANGE;
}

static int ctx_take_errors(ws_context *ctx)
{
  int rc = WS_OK;
  std::lock_guard<std::mutex> lock(ctx->lists_mu);
  for (ws_map *m : ctx->maps)
  {
    const int r = map_take_error(m);
    if (rc == WS_OK) rc = r;
  }
  return rc;
}

// the allocations and first contents of a map whose geometry is set; on an error ws_map_create frees what is there
static int map_build(ws_map *m, const uint32_t *host_data)
{
  hipStream_t s = m->ctx->stream;
  const size_t map_bytes = (size_t)m->n_vox * sizeof(uint32_t);
  // 16 bytes of slack: the tile kernels read the four voxels of a column as one access, also at the very end
  WS_TRY(m->data[0].alloc(map_bytes + 16));
  WS_TRY(m->data[1].alloc(map_bytes + 16));
  WS_TRY(m->vstate.alloc(2 * vstate_plane_bytes(m->n_tiles)));
  WS_HIP(hipMemsetAsync(m->vstate.p, 0, 2 * vstate_plane_bytes(m->n_tiles), s));
  WS_TRY(m->rays.alloc(MAX_SCAN_POINTS, ray_setup_bytes()));
  WS_TRY(m->az_hist.alloc(AZ_ALLOC, sizeof(uint32_t)));
  WS_TRY(m->az_off.alloc(AZ_ALLOC, sizeof(uint32_t)));
  WS_TRY(m->ray_bin.alloc(MAX_SCAN_POINTS, 2 * sizeof(uint32_t)));
  WS_TRY(m->ray_order.alloc(MAX_SCAN_POINTS, sizeof(uint32_t)));
  WS_TRY(m->fan_steps.alloc(WS_FAN_TABLE, sizeof(int32_t)));
  ws::fill_fan_steps(m->fan_steps_host, m->res, m->ntz, m->nty);
  WS_HIP(hipMemcpyAsync(m->fan_steps.p, m->fan_steps_host, WS_FAN_TABLE * sizeof(int32_t), hipMemcpyHostToDevice, s));
  WS_HIP(hipMemsetAsync(m->az_hist.p, 0, AZ_ALLOC * sizeof(uint32_t), s));
  WS_HIP(hipMemsetAsync(m->az_off.p, 0, AZ_ALLOC * sizeof(uint32_t), s));
  WS_TRY(m->scan_dev.alloc(MAX_SCAN_POINTS, 3 * sizeof(int32_t)));
  WS_TRY(m->counters.alloc(1, sizeof(TsdfCounters)));
  WS_HIP(hipMemsetAsync(m->counters.p, 0, sizeof(TsdfCounters), s));
  // per-tile bookkeeping of the scatter: entry count, entry table (64 x 4 bytes), two bytes, one 16-byte list entry per 1024 voxels
  WS_TRY(m->tile_nsub.alloc((size_t)m->n_tiles, sizeof(uint32_t)));
  WS_TRY(m->tile_ent.alloc((size_t)m->n_tiles * TILE_DIRECT * sizeof(uint32_t) + 256));
  WS_TRY(m->tile_dirty.alloc(2 * tile_flag_plane_bytes(m->n_tiles)));
  WS_TRY(m->tile_list.alloc((size_t)m->n_tiles, sizeof(TileEntry)));
  WS_HIP(hipMemsetAsync(m->tile_nsub.p, 0, (size_t)m->n_tiles * sizeof(uint32_t), s));
  WS_HIP(hipMemsetAsync(m->tile_dirty.p, 0, 2 * tile_flag_plane_bytes(m->n_tiles), s));
  WS_TRY(m->block_stats.alloc(WS_BLOCK_STATS, sizeof(uint32_t)));
  WS_HIP(hipMemsetAsync(m->block_stats.p, 0, (size_t)WS_BLOCK_STATS * sizeof(uint32_t), s));
  WS_TRY(m->counters_host.alloc(1, sizeof(TsdfCounters), HostBlock::PINNED));
  WS_TRY(m->status.alloc(16, sizeof(uint32_t), HostBlock::MAPPED, true));
  // the pool of the ray tails' records: what a 131 072-point scan can need on a map of the reference's size (its record bound is
  // ~75 M at 50 mm) -- scaled down for small maps (1.1 GB for a 64^3 map): 32 records per voxel, scans of 16 384
  // points.  Only a first guess: a scan that needs more is aborted and repeated with a larger pool (settle_tsdf),
  // ws_tsdf_set_capacity() reserves up front.
  {
    const bool small_map = m->n_vox < (16ll << 20);
    const unsigned long long need0 = small_map ? std::max<unsigned long long>(1ull << 20, 32ull * (unsigned long long)m->n_vox) : (80ull << 20);
    WS_TRY(map_alloc_records(m, subs_for_scan(m, std::min<unsigned long long>(need0, 80ull << 20), small_map ? 16384 : 131072)));
  }
  const uint32_t def = ((uint32_t)m->tau & 0xffffu);
  if (host_data)
  {
    // DeviceMapMemWrapper(existing_map) x2: avg_map_ and new_map_ both start as the host map (update_tsdf.cu:135-136)
    WS_HIP(hipMemcpyAsync(m->data[0].p, host_data, map_bytes, hipMemcpyHostToDevice, s));
    WS_HIP(hipMemcpyAsync(m->data[1].p, m->data[0].p, map_bytes, hipMemcpyDeviceToDevice, s));
    WS_HIP(hipStreamSynchronize(s));
    m->new_is_default = check_all_equal_host(host_data, m->n_vox, def) != 0;
  }
  else
  {
    WS_TRY(fill_u32(m->ctx, m->data[0].as<uint32_t>(), def, m->n_vox));
    WS_TRY(fill_u32(m->ctx, m->data[1].as<uint32_t>(), def, m->n_vox));
    m->new_is_default = true;
  }
  return WS_OK;
}

int ws_map_create(ws_context *ctx, const int32_t size[3], const int32_t pos[3], const int32_t offset[3],
                  const uint32_t *host_data, int32_t tau, int32_t max_weight, int32_t res, ws_map **out)
{
  if (!ctx || !size || !pos || !offset || !out) return invalid("ws_map_create: NULL argument");
  if (size[0] < 3 || size[1] < 3 || size[2] < 3) return invalid("ws_map_create: map sizes must be >= 3");
  if ((int64_t)size[0] * size[1] >= (1ll << 31) || size[2] > (1 << 20)) return invalid("ws_map_create: map too large (x*y must stay below 2^31 voxels)");
  if (size[0] >= (1 << 24) || size[1] >= (1 << 24) ||
      (int64_t)((size[0] + (1 << TILE_XB) - 1) >> TILE_XB) * ((size[1] + (1 << TILE_YB) - 1) >> TILE_YB) >= (1ll << 24) ||
      ((size[2] + (1 << TILE_ZB) - 1) >> TILE_ZB) >= (1 << 24))
    return invalid("ws_map_create: map too large (more than 2^24 tile columns)");
  if (res < 2) return invalid("ws_map_create: map_resolution must be >= 2 mm (the ray step is resolution/2)");
  if (tau <= 0 || tau > 32767) return invalid("ws_map_create: tau must fit the int16 TSDF value");
  ws_map *m = new (std::nothrow) ws_map();
  if (!m) return invalid("ws_map_create: out of host memory");
  m->ctx = ctx;
  for (int w = 0; w < 2; ++w)
  {
    copy3(m->par[w].size, size);
    copy3(m->par[w].pos, pos);
    copy3(m->par[w].offset, offset);
  }
  m->n_vox = (int64_t)size[0] * size[1] * size[2];
  m->ntx = (size[0] + (1 << TILE_XB) - 1) >> TILE_XB;
  m->nty = (size[1] + (1 << TILE_YB) - 1) >> TILE_YB;
  m->ntz = (size[2] + (1 << TILE_ZB) - 1) >> TILE_ZB;
  m->n_tiles = (int64_t)m->ntx * m->nty * m->ntz;
  if (m->n_tiles >= 0x7fffffffll)
  {
    delete m;
    return invalid("ws_map_create: more than 2^31 tiles");
  }
  m->tau = tau;
  m->max_weight = max_weight;
  m->res = res;

  const int rc = map_build(m, host_data);
  if (rc != WS_OK)
  {
    map_free(m);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lock(ctx->lists_mu);
    ctx->maps.push_back(m);
  }
  *out = m;
  return WS_OK;
}

int ws_map_destroy(ws_map *map) { return map_free(map); }

int ws_map_set_params(ws_map *m, int which, const int32_t size[3], const int32_t pos[3], const int32_t offset[3])
{
  if (!m || !size || !pos || !offset || (which != WS_MAP_AVG && which != WS_MAP_NEW)) return invalid("ws_map_set_params: bad argument");
  WS_SETTLE(m);
  if ((int64_t)size[0] * size[1] * size[2] != m->n_vox) return invalid("ws_map_set_params: voxel count differs from the allocation");
  // parameters are kernel arguments: order against work already enqueued is automatic
  copy3(m->par[which].size, size);
  copy3(m->par[which].pos, pos);
  copy3(m->par[which].offset, offset);
  return WS_OK;
}

int ws_map_upload(ws_map *m, int which, const int32_t size[3], const int32_t pos[3], const int32_t offset[3],
                  const uint32_t *host_data)
{
  if (!host_data) return invalid("ws_map_upload: host_data is NULL");
  int rc = ws_map_set_params(m, which, size, pos, offset);
  if (rc != WS_OK) return rc;
  WS_HIP(hipMemcpyAsync(m->data[which].p, host_data, (size_t)m->n_vox * sizeof(uint32_t), hipMemcpyHostToDevice, m->ctx->stream));
  WS_HIP(hipStreamSynchronize(m->ctx->stream)); // cudaMemcpy of the reference is synchronous; the host buffer may be reused
  if (which == WS_MAP_NEW) m->new_is_default = check_all_equal_host(host_data, m->n_vox, ((uint32_t)m->tau & 0xffffu)) != 0;
  return WS_OK;
}

int ws_map_download(ws_map *m, int which, int32_t size[3], int32_t pos[3], int32_t offset[3], uint32_t *host_data)
{
  if (!m || (which != WS_MAP_AVG && which != WS_MAP_NEW)) return invalid("ws_map_download: bad argument");
  WS_SETTLE(m);
  if (size) copy3(size, m->par[which].size);
  if (pos) copy3(pos, m->par[which].pos);
  if (offset) copy3(offset, m->par[which].offset);
  if (host_data)
  {
    WS_HIP(hipMemcpyAsync(host_data, m->data[which].p, (size_t)m->n_vox * sizeof(uint32_t), hipMemcpyDeviceToHost, m->ctx->stream));
  }
  WS_HIP(hipStreamSynchronize(m->ctx->stream));
  return map_take_error(m);
}

// ---- box transfers: the device side of the map shift (only the slabs that leave / enter move)
static int range_error(const char *name, const char *what)
{
  set_error(std::string(name) + what);
  return WS_ERR_RANGE;
}

// The one rule for where a window may be: pos - size/2 .. pos - size/2 + size - 1 lies in int32 on every axis.  The kernels carry
// world voxels in int32 and only ever form differences inside the window; the host computes the ends in 64 bits here and nowhere
// else.  Its first voxel into lo, its last into hi (64 bits: they are also what the caller compares with), else WS_ERR_RANGE in
// the name of the entry point.  ws_map_create, ws_map_set_params and ws_map_upload do not ask (the update has its own domain).
static int window_fits(const int32_t size[3], const int32_t pos[3], const char *name, int64_t lo[3], int64_t hi[3])
{
  for (int k = 0; k < 3; ++k)
  {
    lo[k] = (int64_t)pos[k] - size[k] / 2;
    hi[k] = lo[k] + size[k] - 1;
    if (lo[k] < (int64_t)INT32_MIN || hi[k] > (int64_t)INT32_MAX) return range_error(name, ": the window pos - size/2 .. pos - size/2 + size - 1 does not fit int32");
  }
  return WS_OK;
}

// The one copy of the box rules.  [lo, hi] in world voxels, both ends included, against the window of map `which`: its first voxel
// into l, its extent into ext.  lo == hi == NULL is the whole window where `allow_whole`.  `name` starts the error texts.
static int resolve_box(const ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], bool allow_whole, const char *name, int32_t l[3], int32_t ext[3])
{
  const auto bad = [name](const char *what) { return invalid((std::string(name) + what).c_str()); };
  if (!allow_whole && (!lo || !hi)) return bad(": bad argument");
  const MapParams &p = m->par[which];
  int64_t wlo[3], whi[3];
  WS_TRY(window_fits(p.size, p.pos, name, wlo, whi));
  for (int k = 0; k < 3; ++k)
  {
    if (!lo)
    {
      l[k] = (int32_t)wlo[k];
      ext[k] = p.size[k];
      continue;
    }
    if (hi[k] < lo[k]) return bad(": hi < lo");
    // within size/2 of pos, in 64 bits (INT32_MIN - pos wraps in 32)
    const int64_t half = p.size[k] / 2;
    if (std::llabs((long long)lo[k] - p.pos[k]) > half || std::llabs((long long)hi[k] - p.pos[k]) > half) return bad(": box outside the local map window");
    l[k] = lo[k];
    ext[k] = (int32_t)((int64_t)hi[k] - lo[k] + 1); // <= size + 1
    // (an even size admits pos - size/2 .. pos + size/2: size + 1 voxels, the first and the last the same ring cell -- two lanes
    // of an insert would store to one address)
    if (ext[k] > p.size[k]) return bad(": box wraps onto itself (more voxels than the ring holds along an axis)");
  }
  return WS_OK;
}

static int box_check(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], int32_t ext[3], size_t *n)
{
  if (!m || (which != WS_MAP_AVG && which != WS_MAP_NEW)) return invalid("box transfer: bad argument");
  int32_t l[3];
  const int rc = resolve_box(m, which, lo, hi, false, "box transfer", l, ext);
  if (rc != WS_OK) return rc;
  const size_t cnt = (size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2];
  *n = cnt;
  if (cnt > m->box_stage.cap)
  {
    WS_HIP(hipStreamSynchronize(m->ctx->stream));
    WS_TRY(m->box_stage.grow(cnt, sizeof(uint32_t), DevBuf::EXACT));
  }
  return WS_OK;
}

int ws_map_extract_box(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], uint32_t *host_out)
{
  if (!host_out) return invalid("ws_map_extract_box: host_out is NULL");
  WS_SETTLE(m);
  int32_t ext[3];
  size_t n = 0;
  int rc = box_check(m, which, lo, hi, ext, &n);
  if (rc != WS_OK) return rc;
  rc = launch_box_copy(m, m->par[which], which, lo, ext, m->box_stage.as<uint32_t>(), true, m->ctx->stream);
  if (rc != WS_OK) return rc;
  WS_HIP(hipMemcpyAsync(host_out, m->box_stage.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, m->ctx->stream));
  WS_HIP(hipStreamSynchronize(m->ctx->stream));
  return WS_OK;
}

int ws_map_insert_box(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], const uint32_t *host_in)
{
  if (!host_in) return invalid("ws_map_insert_box: host_in is NULL");
  WS_SETTLE(m);
  int32_t ext[3];
  size_t n = 0;
  int rc = box_check(m, which, lo, hi, ext, &n);
  if (rc != WS_OK) return rc;
  WS_HIP(hipMemcpyAsync(m->box_stage.p, host_in, n * sizeof(uint32_t), hipMemcpyHostToDevice, m->ctx->stream));
  rc = launch_box_copy(m, m->par[which], which, lo, ext, m->box_stage.as<uint32_t>(), false, m->ctx->stream);
  if (rc != WS_OK) return rc;
  WS_HIP(hipStreamSynchronize(m->ctx->stream)); // the host buffer may be reused by the caller
  if (which == WS_MAP_NEW) m->new_is_default = false;
  return WS_OK;
}

// ---- surface cloud: publish_local_map's extraction (visualization/map.h:14-121) on the device, map_surface.hip
int ws_map_surface(ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], int32_t band, uint32_t flags, size_t *n_out)
{
  if (!m || (which != WS_MAP_AVG && which != WS_MAP_NEW) || (flags & ~WS_SURFACE_MARKER) || ((lo == nullptr) != (hi == nullptr)))
    return invalid("ws_map_surface: bad argument");
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(m->surf.mu);
  ws_map::Surface &q = m->surf;
  int rc = q.timer.arm();
  int32_t l[3], ext[3];
  if (rc == WS_OK) rc = resolve_box(m, which, lo, hi, true, "ws_map_surface", l, ext);
  if (rc == WS_OK) rc = q.total.alloc(1);
  if (rc != WS_OK) return rc;
  if (band <= 0) band = m->tau;
  const bool marker = (flags & WS_SURFACE_MARKER) != 0;
  hipStream_t s = m->ctx->stream;
  const size_t n_cols = (size_t)ext[0] * (size_t)ext[1], blocks = surface_blocks_for((int64_t)n_cols); // n_cols < 2^31 (ws_map_create)
  if (n_cols > q.col_cnt.cap || blocks > q.blk_tot.cap || blocks > q.blk_off.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    rc = q.col_cnt.grow(n_cols, sizeof(uint32_t));
    if (rc == WS_OK) rc = q.blk_tot.grow(blocks, sizeof(uint32_t));
    if (rc == WS_OK) rc = q.blk_off.grow(blocks, sizeof(unsigned long long));
    if (rc != WS_OK) return rc;
  }
  q.n = 0;
  q.has_marker = false;
  rc = launch_surface_count(m, which, l, ext, band);
  if (rc != WS_OK) return rc;
  WS_HIP(hipStreamSynchronize(s)); // the one host read the call needs: the output is sized from the counted total
  const size_t total = (size_t)*q.total.host;
  rc = q.rec.grow(total, 16);
  if (rc == WS_OK && marker) rc = q.marker.grow(total, 7 * sizeof(float));
  if (rc != WS_OK) return rc;
  if (total)
  {
    // (the kernel's bound holds for both buffers)
    rc = launch_surface_emit(m, which, l, ext, band, marker, marker ? std::min(q.rec.cap, q.marker.cap) : q.rec.cap);
    if (rc != WS_OK) return rc;
    WS_HIP(hipStreamSynchronize(s));
  }
  q.n = total;
  q.has_marker = marker;
  if (n_out) *n_out = total;
  return map_take_error(m);
}

const void *ws_map_surface_records_dev(const ws_map *m, size_t *n)
{
  if (n) *n = m ? m->surf.n : 0;
  return m && m->surf.n ? m->surf.rec.p : nullptr;
}

const float *ws_map_surface_marker_dev(const ws_map *m, size_t *n)
{
  const bool have = m && m->surf.has_marker && m->surf.n;
  if (n) *n = have ? m->surf.n : 0;
  return have ? static_cast<const float *>(m->surf.marker.p) : nullptr;
}

int ws_map_surface_download(ws_map *m, void *records_host, float *marker_host, size_t capacity_points, size_t *n_out)
{
  if (!m || !n_out) return invalid("ws_map_surface_download: NULL argument");
  std::lock_guard<std::mutex> lock(m->surf.mu);
  *n_out = m->surf.n;
  const size_t k = std::min(capacity_points, m->surf.n);
  if (k == 0) return WS_OK;
  if (marker_host && !m->surf.has_marker) return invalid("ws_map_surface_download: the last ws_map_surface did not ask for WS_SURFACE_MARKER");
  if (records_host) WS_HIP(hipMemcpyAsync(records_host, m->surf.rec.p, k * 16, hipMemcpyDeviceToHost, m->ctx->stream));
  if (marker_host) WS_HIP(hipMemcpyAsync(marker_host, m->surf.marker.p, k * 7 * sizeof(float), hipMemcpyDeviceToHost, m->ctx->stream));
  WS_HIP(hipStreamSynchronize(m->ctx->stream));
  return WS_OK;
}

// ws_debug_*_timing: the times of the last call between the event pairs of `pairs`, then the switch
static int query_timing(hipStream_t s, QueryTimer &t, int32_t enable, float *ms_out, const int (*pairs)[2], int n)
{
  const int rc = t.read(ms_out, pairs, n, s);
  if (rc == WS_OK) t.set(enable);
  return rc;
}

int ws_debug_surface_timing(ws_map *m, int32_t enable, float ms_out[3])
{
  if (!m) return invalid("ws_debug_surface_timing: map is NULL");
  std::lock_guard<std::mutex> lock(m->surf.mu);
  static const int pairs[3][2] = {{0, 1}, {1, 2}, {3, 4}};
  return query_timing(m->ctx->stream, m->surf.timer, enable, ms_out, pairs, 3);
}

// ---- mesh and ray cast: one host core for the window of a map (map_mesh.hip, map_raycast.hip) and for the chunks of the store
// (store_mesh.hip, store_raycast.hip; their entry points are further down).  An entry point checks what is its own, takes its lock and
// hands the shared flow its result holder, its stream and, as lambdas, the launchers of its source; `name` starts the refusal texts.
extern "C++" {
static int mesh_corners_fit(const int32_t lo[3], const int32_t hi[3], int32_t res, const char *name)
{
  for (int k = 0; k < 3; ++k)
    for (int64_t c : {(int64_t)lo[k], (int64_t)hi[k]})
      if (((c < 0 ? -c : c) + 1) * (int64_t)res > (int64_t)INT32_MAX) return range_error(name, ": a box corner in millimetres does not fit int32");
  return WS_OK;
}

static int mesh_publish(MeshResult &q, size_t nv, size_t nf, size_t *n_vertices, size_t *n_faces)
{
  q.nv = nv, q.nf = nf;
  if (n_vertices) *n_vertices = nv;
  if (n_faces) *n_faces = nf;
  return WS_OK;
}

// The flow of a mesh call over `n_words` words (< 2^31), from "the old result is dropped" to the publish.  count() and emit() enqueue
// the passes of the source and return at once; what a source owes its caller after a failed enqueue is theirs (store_enqueued).
template <typename Count, typename Emit>
static int mesh_run(MeshResult &q, hipStream_t s, const char *name, uint64_t n_words, size_t *n_vertices, size_t *n_faces, Count count, Emit emit)
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

static const void *mesh_vertices_dev(const MeshResult *q, size_t *n)
{
  if (n) *n = q ? q->nv : 0;
  return q && q->nv ? q->vert.p : nullptr;
}

static const uint32_t *mesh_faces_dev(const MeshResult *q, size_t *n)
{
  if (n) *n = q ? q->nf : 0;
  return q && q->nf ? static_cast<const uint32_t *>(q->face.p) : nullptr;
}

static int mesh_download(const MeshResult &q, hipStream_t s, void *vertices_host, uint32_t *faces_host, size_t cap_vertices, size_t cap_faces, size_t *n_vertices,
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
static const int MESH_PAIRS[3][2] = {{0, 1}, {1, 2}, {3, 4}};

// The argument check of a ray cast.  `bad`: what the entry point found wrong with its own leading arguments; more(): its further
// checks, which come before those of the ranges.
template <typename More>
static int raycast_check(const char *name, bool bad, const int32_t *origin, const int32_t *dirs, size_t n, int32_t max_range, int32_t res, uint32_t flags, More more)
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
static int raycast_run(RayResult &q, hipStream_t s, const int32_t *dirs, bool dirs_on_host, size_t n, uint32_t flags, size_t *n_hits, bool own_room, Prepare prepare,
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

static const void *raycast_records_dev(const RayResult *q, size_t *n)
{
  if (n) *n = q ? q->n : 0;
  return q && q->n ? q->rec.p : nullptr;
}

static const int32_t *raycast_gradient_dev(const RayResult *q, size_t *n)
{
  const bool have = q && q->has_grad && q->n;
  if (n) *n = have ? q->n : 0;
  return have ? static_cast<const int32_t *>(q->grad.p) : nullptr;
}

// `name`, `call`: the download entry point, and the entry point whose flag it misses
static int raycast_download(const RayResult &q, hipStream_t s, const char *name, const char *call, void *records_host, int32_t *gradient_host, size_t capacity_rays,
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
static const int RAY_PAIRS[3][2] = {{0, 1}, {1, 2}, {2, 3}};
} // extern "C++"

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

// ---- distance field: one host core for the window of a map (map_distance.hip) and for the chunks of the store (store_distance.hip;
// its entry points are further down), in the way of mesh_run and raycast_run above.  The sources differ in pass 0 only.
extern "C++" {
// The argument check of a distance call.  `bad`: what the entry point found wrong with its own leading arguments; box(e): its lock and
// its box, which come behind the checks of the flags and of R -- the extents in 64 bits, all zero for "nothing to do".  ext and *n
// receive the extents the passes take and the number of records.
template <typename Box>
static int distance_check(const char *name, bool bad, const int32_t *lo, const int32_t *hi, int32_t R, uint32_t flags, Box box, uint32_t ext[3], size_t *n)
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
static int distance_run(DistResult &q, hipStream_t s, const uint32_t ext[3], int32_t R, uint32_t flags, size_t n, size_t *n_sites, Pass0 pass0)
{
  if (n_sites) *n_sites = 0;
  q.n = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  if (n == 0) return WS_OK;
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
  if (n_sites) *n_sites = (size_t)*q.sites.host;
  return WS_OK;
}

static const uint32_t *distance_dev(const DistResult *q, size_t *n)
{
  if (n) *n = q ? q->n : 0;
  return q && q->n ? static_cast<const uint32_t *>(q->rec.p) : nullptr;
}

static int distance_download(const DistResult &q, hipStream_t s, uint32_t *host, size_t capacity, size_t *n_out)
{
  *n_out = q.n;
  const size_t k = host ? std::min(capacity, q.n) : 0;
  if (k == 0) return WS_OK;
  WS_HIP(hipMemcpyAsync(host, q.rec.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}
static const int DIST_PAIRS[4][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}};
} // extern "C++"

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
  WS_TRY(distance_run(q, m->ctx->stream, e32, max_dist_vox, flags, n, n_sites, [&] { return launch_dist_classify(m, q, which, l, ext, max_dist_vox, flags); }));
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

// ---- map shift
// The plan of a shift (ws_shift_plan; `name` is the entry point the refusal speaks for): per axis, like HDF5LocalMap::shift
// (hdf5_local_map.cpp:53-118), with the window as it is when that axis moves.  The window is pos - size/2 .. pos - size/2 + size - 1,
// every ring cell once: the reference's pos + size/2 for its odd sizes; for an even size pos + size/2 would be the ring cell of
// pos - size/2 again, filed under a second world position.
static int plan_shift(const int32_t size[3], const int32_t pos0[3], const int32_t offset0[3], const int32_t new_pos[3], const char *name,
                      ws_shift_plan_t *out)
{
  int32_t *pos = out->pos;
  copy3(pos, pos0);
  copy3(out->offset, offset0);
  out->n = 0;
  // Every window of the plan fits int32 (window_fits), the one the shift starts from included.  An axis moves once, so a window
  // between two axis steps is per axis the first window's range or the last one's: asking after every step asks for all of them.
  // Per axis, x then y then z: the step's size first (WS_ERR_INVALID), then the window behind it (WS_ERR_RANGE).
  int64_t lo[3], hi[3];
  WS_TRY(window_fits(size, pos, name, lo, hi));
  for (int axis = 0; axis < 3; ++axis)
  {
    const int64_t d = (int64_t)new_pos[axis] - pos[axis];
    if (d == 0) continue;
    if (std::llabs((long long)d) > size[axis]) return invalid((std::string(name) + ": shift larger than the window").c_str());
    int64_t start[3] = {lo[0], lo[1], lo[2]}, end[3] = {hi[0], hi[1], hi[2]}; // the window before the step
    pos[axis] = new_pos[axis];
    WS_TRY(window_fits(size, pos, name, lo, hi)); // ... and behind it
    const int i = out->n++;
    out->axis[i] = axis;
    out->d[i] = (int32_t)d;
    if (d > 0)
      end[axis] = start[axis] + d - 1;
    else
      start[axis] = end[axis] + d + 1;
    for (int k = 0; k < 3; ++k) out->leave_lo[i][k] = (int32_t)start[k], out->leave_hi[i][k] = (int32_t)end[k];
    out->offset[axis] = (int32_t)((((int64_t)out->offset[axis] + d) % size[axis] + size[axis]) % size[axis]);
    for (int k = 0; k < 3; ++k) start[k] = lo[k], end[k] = hi[k];
    if (d > 0)
      start[axis] = end[axis] - (d - 1);
    else
      end[axis] = start[axis] - d - 1;
    for (int k = 0; k < 3; ++k) out->enter_lo[i][k] = (int32_t)start[k], out->enter_hi[i][k] = (int32_t)end[k];
  }
  return WS_OK;
}

int ws_shift_plan(const int32_t size[3], const int32_t pos[3], const int32_t offset[3], const int32_t new_pos[3], ws_shift_plan_t *out)
{
  if (!size || !pos || !offset || !new_pos || !out) return invalid("ws_shift_plan: NULL argument");
  for (int k = 0; k < 3; ++k)
    if (size[k] < 1) return invalid("ws_shift_plan: size < 1");
  return plan_shift(size, pos, offset, new_pos, "ws_shift_plan", out);
}

// the axis step of both maps' windows between the save and the load of a slab (pos and offset, DeviceMapMemWrapper::update_params)
static void move_axis(MapParams par[2], int axis, int32_t d)
{
  for (int w = 0; w < 2; ++w)
  {
    MapParams &p = par[w];
    p.pos[axis] += d;
    p.offset[axis] = (int32_t)((((int64_t)p.offset[axis] + d) % p.size[axis] + p.size[axis]) % p.size[axis]);
  }
}

// One shift of both maps' windows, for ws_shift_begin and ws_shift_device, which differ in what happens to a slab that leaves and
// to one that enters.  `name` is the entry point and `open_text` its words for a ticket in flight.  After the shared refusals and
// the plan (into `plan`): ready() before the first launch; per step leave(i, par), the axis step, enter(i, par), on a COPY of the
// parameters (the box kernels take them by value); done() behind the last step.  The copy is committed only when all of it has
// been enqueued: the first error is returned with the host's view of both maps as it was.
extern "C++" {
template <class Ready, class Leave, class Enter, class Done>
static int run_shift(ws_map *m, const int32_t new_pos[3], const char *name, const char *open_text, ws_shift_plan_t &plan, Ready ready, Leave leave,
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
} // extern "C++"

static int shift_reserve(ws_map *m, size_t total)
{
  if (total <= m->shift_stage_dev.cap && total <= m->shift_stage_host.cap) return WS_OK;
  WS_HIP(hipStreamSynchronize(m->ctx->stream));
  WS_TRY(m->shift_stage_dev.grow(total, sizeof(uint32_t), DevBuf::EXACT));
  WS_TRY(m->shift_stage_host.grow(total, sizeof(uint32_t), HostBlock::PINNED));
  if (!m->shift_stream) WS_HIP(hipStreamCreateWithFlags(&m->shift_stream, hipStreamNonBlocking));
  if (!m->shift_event) WS_HIP(hipEventCreateWithFlags(&m->shift_event, hipEventDisableTiming));
  return WS_OK;
}

int ws_shift_reserve(ws_map *m, uint64_t voxels)
{
  if (!m) return invalid("ws_shift_reserve: map is NULL");
  if (m->shift_open) return invalid("ws_shift_reserve: a shift is in flight");
  return shift_reserve(m, (size_t)voxels);
}

static size_t box_extent(const int32_t lo[3], const int32_t hi[3], int32_t ext[3]) // the voxels of the box
{
  for (int k = 0; k < 3; ++k) ext[k] = hi[k] - lo[k] + 1;
  return (size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2];
}

int ws_shift_begin(ws_map *m, const int32_t new_pos[3], uint32_t fill_entry, ws_shift **out)
{
  if (!m || !new_pos || !out) return invalid("ws_shift_begin: NULL argument");
  ws_shift *sh = new (std::nothrow) ws_shift();
  if (!sh) return invalid("ws_shift_begin: out of host memory");
  sh->map = m;
  const ws_shift_plan_t &plan = sh->plan;
  hipStream_t s = m->ctx->stream;
  const int rc = run_shift(
      m, new_pos, "ws_shift_begin", ": the previous shift of this map has not been ended (ws_shift_end)", sh->plan,
      [&]() -> int {
        // the leaving slabs lie packed in the staging buffers (a shift larger than anything reserved: they grow, which waits for the
        // stream once)
        int32_t ext[3];
        sh->total = 0;
        for (int i = 0; i < plan.n; ++i) sh->offset[i] = sh->total, sh->total += box_extent(plan.leave_lo[i], plan.leave_hi[i], ext);
        return shift_reserve(m, sh->total ? sh->total : 1);
      },
      [&](int i, const MapParams &par) -> int {
        int32_t ext[3];
        box_extent(plan.leave_lo[i], plan.leave_hi[i], ext);
        return launch_box_copy(m, par, WS_MAP_AVG, plan.leave_lo[i], ext, m->shift_stage_dev.as<uint32_t>() + sh->offset[i], true, s);
      },
      [&](int i, const MapParams &par) -> int {
        int32_t ext[3];
        box_extent(plan.enter_lo[i], plan.enter_hi[i], ext);
        return launch_box_fill(m, par, WS_MAP_AVG, plan.enter_lo[i], ext, fill_entry, s);
      },
      [&]() -> int { // the staged slabs travel to the host on the second stream
        if (!sh->total) return WS_OK;
        hipError_t e = hipEventRecord(m->shift_event, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(m->shift_stream, m->shift_event, 0);
        if (e == hipSuccess)
          e = hipMemcpyAsync(m->shift_stage_host.p, m->shift_stage_dev.p, sh->total * sizeof(uint32_t), hipMemcpyDeviceToHost, m->shift_stream);
        return e == hipSuccess ? WS_OK : hip_fail(e, "ws_shift_begin copy", __FILE__, __LINE__);
      });
  if (rc == WS_OK)
    m->shift_open = *out = sh;
  else
    delete sh;
  return rc;
}

int ws_shift_count(const ws_shift *sh) { return sh ? sh->plan.n : 0; }

int ws_shift_entering(const ws_shift *sh, int i, int32_t lo[3], int32_t hi[3])
{
  if (!sh || i < 0 || i >= sh->plan.n || !lo || !hi) return invalid("ws_shift_entering: bad argument");
  copy3(lo, sh->plan.enter_lo[i]);
  copy3(hi, sh->plan.enter_hi[i]);
  return WS_OK;
}

int ws_shift_wait(ws_shift *sh)
{
  if (!sh) return invalid("ws_shift_wait: shift is NULL");
  if (sh->map->shift_stream) WS_HIP(hipStreamSynchronize(sh->map->shift_stream));
  return WS_OK;
}

int ws_shift_slab(const ws_shift *sh, int i, int32_t lo[3], int32_t hi[3], const uint32_t **host_data)
{
  if (!sh || i < 0 || i >= sh->plan.n || !lo || !hi || !host_data) return invalid("ws_shift_slab: bad argument");
  copy3(lo, sh->plan.leave_lo[i]);
  copy3(hi, sh->plan.leave_hi[i]);
  *host_data = sh->map->shift_stage_host.as<uint32_t>() + sh->offset[i];
  return WS_OK;
}

int ws_shift_end(ws_shift *sh)
{
  if (!sh) return WS_OK;
  if (sh->map->shift_stream) (void)hipStreamSynchronize(sh->map->shift_stream);
  if (sh->map->shift_open == sh) sh->map->shift_open = nullptr;
  delete sh;
  return WS_OK;
}

// ---- the chunk store: the global map in device memory (map_store.hip)
namespace
{
using StoreKey = std::array<int32_t, 3>;
inline int32_t chunk_of(int32_t v) { return v >= 0 ? v / STORE_CS : -((-(int64_t)v + STORE_CS - 1) / STORE_CS); } // floor(v / 64)

// the chunks an inclusive world box overlaps: first key and count per axis
struct ChunkRange
{
  int32_t c0[3], nc[3];
  size_t n;
  ChunkRange(const int32_t lo[3], const int32_t hi[3])
  {
    n = 1;
    for (int k = 0; k < 3; ++k)
    {
      c0[k] = chunk_of(lo[k]);
      nc[k] = chunk_of(hi[k]) - c0[k] + 1;
      n *= (size_t)nc[k];
    }
  }
  StoreKey key(size_t i) const // x major, like the slot table
  {
    const size_t plane = (size_t)nc[1] * (size_t)nc[2];
    return {c0[0] + (int32_t)(i / plane), c0[1] + (int32_t)(i % plane / (size_t)nc[2]), c0[2] + (int32_t)(i % (size_t)nc[2])};
  }
};

uint64_t store_capacity(const ws_store *st) { return (uint64_t)st->segs.size() << st->seg_shift; }

uint32_t *store_slot_ptr(const ws_store *st, uint32_t slot)
{
  return st->seg_ptr[slot >> st->seg_shift] + (size_t)(slot & ((1u << st->seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
}

// Segments for `chunks` chunks in all.  Adding one waits for the stream (the kernels in flight read the old segment table); a failed
// allocation gives back what this call added, so the store is as it was.
int store_grow(ws_store *st, uint64_t chunks)
{
  if (chunks <= store_capacity(st)) return WS_OK;
  if (chunks >= 0x7fffffffull) return invalid("ws_store: more than 2^31 - 1 chunks");
  const size_t had = st->segs.size(), want = (size_t)((chunks + (1ull << st->seg_shift) - 1) >> st->seg_shift);
  WS_HIP(hipStreamSynchronize(st->ctx->stream));
  int rc = WS_OK;
  DevBuf tab;
  for (size_t i = had; i < want && rc == WS_OK; ++i)
  {
    st->segs.emplace_back();
    rc = st->segs.back().alloc((size_t)STORE_CHUNK_WORDS << st->seg_shift, sizeof(uint32_t));
    if (rc == WS_OK) st->seg_ptr.push_back(st->segs.back().as<uint32_t>());
  }
  if (rc == WS_OK) rc = tab.alloc(want, sizeof(uint32_t *));
  if (rc == WS_OK)
  {
    const hipError_t e = hipMemcpy(tab.p, st->seg_ptr.data(), want * sizeof(uint32_t *), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy (segment table)", __FILE__, __LINE__);
  }
  if (rc != WS_OK)
  {
    tab.release();
    for (size_t i = had; i < st->segs.size(); ++i) st->segs[i].release();
    st->segs.resize(had);
    st->seg_ptr.resize(had);
    return rc;
  }
  st->seg_tab.release();
  st->seg_tab = tab; // (DevBuf is a plain pair: the store owns the new table now)
  return WS_OK;
}

// chunks that can still be created without a new segment / at all
uint64_t store_unused(const ws_store *st) { return st->free_slots.size() + (store_capacity(st) - st->next_slot); }

// Room for `fresh` more chunks: WS_ERR_CAPACITY beyond max_chunks, segments where they are missing.  Nothing else changes.
int store_make_room(ws_store *st, uint64_t fresh, const char *name)
{
  if (st->max_chunks && st->dir.size() + fresh > st->max_chunks)
  {
    set_error(std::string(name) + ": the store would hold more than max_chunks chunks");
    return WS_ERR_CAPACITY;
  }
  if (fresh <= store_unused(st)) return WS_OK;
  return store_grow(st, (uint64_t)st->next_slot + (fresh - st->free_slots.size()));
}

uint32_t store_take_slot(ws_store *st) // (store_make_room has been asked)
{
  if (!st->free_slots.empty())
  {
    const uint32_t s = st->free_slots.back();
    st->free_slots.pop_back();
    return s;
  }
  return st->next_slot++;
}

// room for n words in one slot table (pinned + device) and its event
int store_table_reserve(ws_store::Table &t, size_t n)
{
  if (!t.done) WS_HIP(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  if (n <= t.host.cap) return WS_OK;
  WS_TRY(t.host.alloc(n, sizeof(uint32_t), HostBlock::PINNED));
  return t.dev.alloc(n, sizeof(uint32_t));
}

// The next slot table of the ring, for n words: waits only for the launch that read this table STORE_TABLES calls ago.  The tables are
// sized when the store is created (STORE_TABLE_WORDS); a box that overlaps more chunks makes one grow here, which allocates.
int store_table(ws_store *st, size_t n, ws_store::Table **out)
{
  ws_store::Table &t = st->tab[st->tab_next];
  st->tab_next = (st->tab_next + 1) % STORE_TABLES;
  if (t.used) WS_HIP(hipEventSynchronize(t.done));
  t.used = false;
  WS_TRY(store_table_reserve(t, n > t.host.cap ? n + n / 8 : n));
  *out = &t;
  return WS_OK;
}

// One launch: the box of `which` (window `par`) into the chunks or back.  The directory already holds every chunk a save needs (a
// save table never holds STORE_ABSENT: the kernel would read that word as slot 2^31 - 1, flagged new).  A chunk this call created
// and nothing has written yet is flagged STORE_NEW by the first save that meets it -- that launch writes it whole -- and is absent
// to a load: a later slab of the same shift will write it.
int store_enqueue(ws_store *st, ws_map *m, const MapParams &par, int which, const int32_t lo[3], const int32_t hi[3], bool save)
{
  const ChunkRange cr(lo, hi);
  ws_store::Table *t = nullptr;
  WS_TRY(store_table(st, cr.n, &t));
  uint32_t *w = t->host.as<uint32_t>();
  bool any_new = false;
  for (size_t i = 0; i < cr.n; ++i)
  {
    const auto it = st->dir.find(cr.key(i));
    if (it == st->dir.end() || (!save && !it->second.written))
    {
      if (save)
      {
        set_error("ws_store: internal error, a save met a chunk without a slot");
        return WS_ERR_INTERNAL;
      }
      w[i] = STORE_ABSENT;
      continue;
    }
    w[i] = it->second.slot | (it->second.written ? 0u : STORE_NEW);
    any_new |= !it->second.written;
    it->second.written = true;
  }
  hipStream_t s = st->ctx->stream;
  WS_HIP(hipMemcpyAsync(t->dev.p, t->host.p, cr.n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  WS_TRY(launch_store_copy(st, m, par, which, lo, hi, cr.c0, cr.nc, t->dev.as<uint32_t>(), save, any_new, s));
  WS_HIP(hipEventRecord(t->done, s));
  t->used = true;
  return WS_OK;
}

// the keys of `lo .. hi` the directory does not hold yet, into `fresh` (a set: each once)
void store_missing(const ws_store *st, const int32_t lo[3], const int32_t hi[3], std::set<StoreKey> &fresh)
{
  const ChunkRange cr(lo, hi);
  for (size_t i = 0; i < cr.n; ++i)
  {
    const StoreKey key = cr.key(i);
    if (!st->dir.count(key)) fresh.insert(key);
  }
}

// gives the chunks of `fresh` their slots (unwritten) / takes them back after a failure half-way
void store_admit(ws_store *st, const std::set<StoreKey> &fresh)
{
  for (const StoreKey &k : fresh) st->dir[k] = ws_store::Entry{store_take_slot(st), false};
}
void store_evict(ws_store *st, const std::set<StoreKey> &fresh)
{
  for (const StoreKey &k : fresh)
  {
    const auto it = st->dir.find(k);
    if (it == st->dir.end()) continue;
    st->free_slots.push_back(it->second.slot);
    st->dir.erase(it);
  }
}

int store_args(const ws_store *st, const ws_map *m, int which, const char *name)
{
  if (!st || !m || (which != WS_MAP_AVG && which != WS_MAP_NEW)) return invalid((std::string(name) + ": bad argument").c_str());
  if (st->ctx != m->ctx) return invalid((std::string(name) + ": the store belongs to another context").c_str());
  return WS_OK;
}
} // namespace

int ws_store_create(ws_context *ctx, uint32_t fill_entry, uint64_t max_chunks, uint32_t segment_chunks, ws_store **out)
{
  if (!ctx || !out) return invalid("ws_store_create: NULL argument");
  if (segment_chunks > (1u << 16)) return invalid("ws_store_create: segment_chunks beyond 65 536 (64 GB per segment)");
  ws_store *st = new (std::nothrow) ws_store();
  if (!st) return invalid("ws_store_create: out of host memory");
  st->ctx = ctx;
  st->fill = fill_entry;
  st->max_chunks = max_chunks;
  // the default: 256 chunks = 256 MB per segment; any other value is rounded up to a power of two (the kernels shift and mask)
  const uint32_t want = segment_chunks ? segment_chunks : 256u;
  while ((1u << st->seg_shift) < want) ++st->seg_shift;
  // the slot tables and their events now: no shift allocates them
  for (ws_store::Table &t : st->tab)
  {
    const int rc = store_table_reserve(t, STORE_TABLE_WORDS);
    if (rc != WS_OK)
    {
      st->release();
      delete st;
      return rc;
    }
  }
  *out = st;
  return WS_OK;
}

int ws_store_destroy(ws_store *st)
{
  if (!st) return WS_OK;
  (void)hipStreamSynchronize(st->ctx->stream);
  st->release();
  delete st;
  return WS_OK;
}

int ws_store_reserve(ws_store *st, uint64_t chunks)
{
  if (!st) return invalid("ws_store_reserve: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  if (st->max_chunks && chunks > st->max_chunks) chunks = st->max_chunks;
  return store_grow(st, chunks);
}

int ws_store_count(const ws_store *st, uint64_t *chunks, uint64_t *capacity_chunks)
{
  if (!st) return invalid("ws_store_count: store is NULL");
  std::lock_guard<std::mutex> lock(const_cast<ws_store *>(st)->mu);
  if (chunks) *chunks = st->dir.size();
  if (capacity_chunks) *capacity_chunks = store_capacity(st);
  return WS_OK;
}

int ws_store_keys(const ws_store *st, int32_t *keys, size_t capacity, size_t *n_out)
{
  if (!st || (!keys && capacity)) return invalid("ws_store_keys: bad argument");
  std::lock_guard<std::mutex> lock(const_cast<ws_store *>(st)->mu);
  size_t i = 0;
  for (const auto &kv : st->dir)
  {
    if (i >= capacity) break;
    for (int k = 0; k < 3; ++k) keys[3 * i + k] = kv.first[k];
    ++i;
  }
  if (n_out) *n_out = st->dir.size();
  return WS_OK;
}

int ws_store_has(const ws_store *st, const int32_t key[3])
{
  if (!st || !key) return 0;
  std::lock_guard<std::mutex> lock(const_cast<ws_store *>(st)->mu);
  return st->dir.count({key[0], key[1], key[2]}) ? 1 : 0;
}

int ws_store_get_chunk(ws_store *st, const int32_t key[3], uint32_t *host, int32_t *found)
{
  if (!st || !key || !host) return invalid("ws_store_get_chunk: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  const auto it = st->dir.find({key[0], key[1], key[2]});
  if (found) *found = it != st->dir.end();
  if (it == st->dir.end()) return WS_OK;
  WS_HIP(hipMemcpyAsync(host, store_slot_ptr(st, it->second.slot), (size_t)STORE_CHUNK_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st->ctx->stream));
  WS_HIP(hipStreamSynchronize(st->ctx->stream));
  return WS_OK;
}

int ws_store_put_chunk(ws_store *st, const int32_t key[3], const uint32_t *host)
{
  if (!st || !key || !host) return invalid("ws_store_put_chunk: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  const StoreKey k = {key[0], key[1], key[2]};
  auto it = st->dir.find(k);
  if (it == st->dir.end())
  {
    WS_TRY(store_make_room(st, 1, "ws_store_put_chunk"));
    it = st->dir.emplace(k, ws_store::Entry{store_take_slot(st), true}).first;
  }
  WS_HIP(hipMemcpyAsync(store_slot_ptr(st, it->second.slot), host, (size_t)STORE_CHUNK_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, st->ctx->stream));
  WS_HIP(hipStreamSynchronize(st->ctx->stream)); // the host buffer may be reused by the caller
  return WS_OK;
}

int ws_store_drop_chunk(ws_store *st, const int32_t key[3])
{
  if (!st || !key) return invalid("ws_store_drop_chunk: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  const auto it = st->dir.find({key[0], key[1], key[2]});
  if (it == st->dir.end()) return invalid("ws_store_drop_chunk: the store has no such chunk");
  // whatever still reads or writes the slot was enqueued before whatever the next owner of the slot enqueues
  st->free_slots.push_back(it->second.slot);
  st->dir.erase(it);
  return WS_OK;
}

const uint32_t *ws_store_chunk_dev(const ws_store *st, const int32_t key[3])
{
  if (!st || !key) return nullptr;
  std::lock_guard<std::mutex> lock(const_cast<ws_store *>(st)->mu);
  const auto it = st->dir.find({key[0], key[1], key[2]});
  return it == st->dir.end() ? nullptr : store_slot_ptr(st, it->second.slot);
}

static int store_box(ws_store *st, ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], bool save, const char *name)
{
  WS_TRY(store_args(st, m, which, name));
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(st->mu);
  int32_t l[3], ext[3];
  WS_TRY(resolve_box(m, which, lo, hi, false, name, l, ext));
  WS_TRY(st->timer[0].arm());
  st->timer[1].marked = st->timer[2].marked = 0;
  std::set<StoreKey> fresh;
  if (save)
  {
    store_missing(st, lo, hi, fresh);
    WS_TRY(store_make_room(st, fresh.size(), name));
    store_admit(st, fresh); // (nothing below can fail before the launch is being enqueued)
  }
  st->timer[0].mark(save ? 0 : 1, st->ctx->stream);
  const int rc = store_enqueue(st, m, m->par[which], which, lo, hi, save);
  st->timer[0].mark(save ? 1 : 2, st->ctx->stream);
  if (rc != WS_OK)
  {
    store_evict(st, fresh);
    return rc;
  }
  if (!save && which == WS_MAP_NEW) m->new_is_default = false;
  return WS_OK;
}

int ws_store_save_box(ws_store *st, ws_map *m, int which, const int32_t lo[3], const int32_t hi[3])
{
  return store_box(st, m, which, lo, hi, true, "ws_store_save_box");
}

int ws_store_load_box(ws_store *st, ws_map *m, int which, const int32_t lo[3], const int32_t hi[3])
{
  return store_box(st, m, which, lo, hi, false, "ws_store_load_box");
}

int ws_shift_device(ws_map *m, ws_store *st, const int32_t new_pos[3])
{
  WS_TRY(store_args(st, m, WS_MAP_AVG, "ws_shift_device"));
  if (!new_pos) return invalid("ws_shift_device: new_pos is NULL");
  std::unique_lock<std::mutex> lock(st->mu, std::defer_lock); // taken in ready(), after the refusals, and held to the end of the call
  ws_shift_plan_t plan;
  std::set<StoreKey> fresh; // the chunks this call has created
  hipStream_t s = m->ctx->stream;
  const int rc = run_shift(
      m, new_pos, "ws_shift_device", ": a shift of this map is in flight (ws_shift_end)", plan,
      [&]() -> int {
        lock.lock();
        for (QueryTimer &t : st->timer) WS_TRY(t.arm());
        // every chunk the leaving slabs of ALL axes create, before the first launch: a call that cannot get them changes nothing
        std::set<StoreKey> missing;
        for (int i = 0; i < plan.n; ++i) store_missing(st, plan.leave_lo[i], plan.leave_hi[i], missing);
        WS_TRY(store_make_room(st, missing.size(), "ws_shift_device"));
        store_admit(st, missing);
        fresh.swap(missing);
        return WS_OK;
      },
      [&](int i, const MapParams &par) -> int {
        st->timer[i].mark(0, s);
        const int rc_save = store_enqueue(st, m, par, WS_MAP_AVG, plan.leave_lo[i], plan.leave_hi[i], true);
        st->timer[i].mark(1, s);
        if (rc_save != WS_OK) st->timer[i].mark(2, s); // the step ends here, its load is never enqueued: close its second interval too
        return rc_save;
      },
      [&](int i, const MapParams &par) -> int {
        const int rc_load = store_enqueue(st, m, par, WS_MAP_AVG, plan.enter_lo[i], plan.enter_hi[i], false);
        st->timer[i].mark(2, s);
        return rc_load;
      },
      []() -> int { return WS_OK; });
  if (rc != WS_OK) store_evict(st, fresh); // (after a refusal, which holds no lock, `fresh` is empty)
  return rc;
}

int ws_store_chunks_of_box(const int32_t lo[3], const int32_t hi[3], int32_t *keys, size_t capacity, size_t *n_out)
{
  if (!lo || !hi || (!keys && capacity)) return invalid("ws_store_chunks_of_box: bad argument");
  for (int k = 0; k < 3; ++k)
    if (hi[k] < lo[k]) return invalid("ws_store_chunks_of_box: hi < lo");
  const ChunkRange cr(lo, hi);
  for (size_t i = 0; i < cr.n && i < capacity; ++i)
  {
    const StoreKey key = cr.key(i); // x major, z fastest: ascending (cx, cy, cz)
    for (int k = 0; k < 3; ++k) keys[3 * i + k] = key[k];
  }
  if (n_out) *n_out = cr.n;
  return WS_OK;
}

int ws_debug_store_timing(ws_store *st, int32_t enable, float ms_out[2])
{
  if (!st) return invalid("ws_debug_store_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  static const int pairs[2][2] = {{0, 1}, {1, 2}};
  float sum[2] = {0.f, 0.f};
  for (QueryTimer &t : st->timer)
  {
    float ms[2] = {0.f, 0.f};
    WS_TRY(t.read(ms_out ? ms : nullptr, pairs, 2, st->ctx->stream));
    sum[0] += ms[0], sum[1] += ms[1];
    t.set(enable);
  }
  if (ms_out) ms_out[0] = sum[0], ms_out[1] = sum[1];
  return WS_OK;
}

// ---- the mesh, the ray cast and the distance field of the store: the rules and the host flow of ws_map_mesh, ws_map_raycast and
// ws_map_distance over the chunks, store_mesh.hip, store_raycast.hip and store_distance.hip (the semantics are stated in warpsense_hip.h)
namespace
{
// The written chunks the box overlaps, ascending (cx, cy, cz) like the directory: visit(key, slot).  The directory is ordered by cx
// first and only the keys of the box's cx range are visited: nothing here follows the volume of the box.
extern "C++" template <typename Visit> void store_walk_box(const ws_store *st, const int32_t lo[3], const int32_t hi[3], Visit visit)
{
  const ChunkRange cr(lo, hi);
  for (auto it = st->dir.lower_bound(StoreKey{cr.c0[0], INT32_MIN, INT32_MIN}); it != st->dir.end() && it->first[0] - cr.c0[0] < cr.nc[0]; ++it)
  {
    bool in = it->second.written;
    for (int k = 1; k < 3; ++k) in = in && it->first[k] >= cr.c0[k] && it->first[k] - cr.c0[k] < cr.nc[k];
    if (in) visit(it->first, it->second.slot);
  }
}

// A store call waits for the stream even after a failed enqueue (whose error it reports): the pinned table of the call must be free
// again when the call returns.
int store_enqueued(const ws_store *st, int rc)
{
  if (rc != WS_OK) (void)hipStreamSynchronize(st->ctx->stream);
  return rc;
}

// The call's tables, into st->mesh.table_host: the chunks store_walk_box lists; per chunk the four counts that place its 4096 words
// in world order, its key and slot, and the list positions of its 26 neighbours.  Everything is O(listed chunks x log).
int store_mesh_tables(ws_store *st, const int32_t lo[3], const int32_t hi[3], std::vector<StoreKey> &keys)
{
  keys.clear();
  std::vector<uint32_t> slots;
  store_walk_box(st, lo, hi, [&](const StoreKey &key, uint32_t slot) { keys.push_back(key), slots.push_back(slot); });
  const size_t n = keys.size();
  if (n == 0 || n >= (1u << 19)) return WS_OK; // (the caller decides: nothing to do / WS_ERR_RANGE)
  if (store_mesh_table_bytes(n) > st->mesh.table_host.cap)
  {
    WS_HIP(hipStreamSynchronize(st->ctx->stream));
    const size_t want = store_mesh_table_bytes(n + n / 8);
    WS_TRY(st->mesh.table_host.alloc(want, 1, HostBlock::PINNED));
    WS_TRY(st->mesh.table_dev.alloc(want, 1));
  }
  uint32_t *grp = st->mesh.table_host.as<uint32_t>();
  int32_t *key = reinterpret_cast<int32_t *>(grp + 4 * n);
  uint32_t *nb = grp + 8 * n;
  for (size_t b = 0; b < n;) // the chunks of one cx: [b, e)
  {
    size_t e = b;
    while (e < n && keys[e][0] == keys[b][0]) ++e;
    for (size_t p = b; p < e;) // the chunks of one (cx, cy): [p, q)
    {
      size_t q = p;
      while (q < e && keys[q][1] == keys[p][1]) ++q;
      for (size_t i = p; i < q; ++i)
      {
        grp[4 * i + 0] = (uint32_t)b, grp[4 * i + 1] = (uint32_t)(e - b), grp[4 * i + 2] = (uint32_t)(p - b), grp[4 * i + 3] = (uint32_t)(q - p);
        for (int k = 0; k < 3; ++k) key[4 * i + k] = keys[i][k];
        key[4 * i + 3] = (int32_t)slots[i];
      }
      p = q;
    }
    b = e;
  }
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 27; ++c)
    {
      // (keys are floor(int32 / 64): a step of one cannot overflow)
      const StoreKey k = {keys[i][0] + c / 9 - 1, keys[i][1] + c / 3 % 3 - 1, keys[i][2] + c % 3 - 1};
      const auto it = std::lower_bound(keys.begin(), keys.end(), k);
      nb[27 * i + c] = it != keys.end() && *it == k ? (uint32_t)(it - keys.begin()) : 0xffffffffu;
    }
  return WS_OK;
}
} // namespace

int ws_store_mesh(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t map_resolution, uint32_t flags, size_t *n_vertices, size_t *n_faces)
{
  if (!st || (flags & ~WS_MESH_ANY_WEIGHT) || ((lo == nullptr) != (hi == nullptr)) || map_resolution <= 0) return invalid("ws_store_mesh: bad argument");
  if (lo)
    for (int k = 0; k < 3; ++k)
      if (hi[k] < lo[k]) return invalid("ws_store_mesh: hi < lo");
  std::lock_guard<std::mutex> lock(st->mu);
  ws_store::Mesh &q = st->mesh;
  WS_TRY(q.timer.arm());
  int32_t l[3], h[3];
  if (lo)
    copy3(l, lo), copy3(h, hi);
  else
  {
    if (st->dir.empty()) return mesh_publish(q, 0, 0, n_vertices, n_faces);
    // the bounding box of the present chunks (keys are floor(int32 / 64): 64 k + 63 fits)
    for (int k = 0; k < 3; ++k) l[k] = INT32_MAX, h[k] = INT32_MIN;
    for (const auto &kv : st->dir)
      for (int k = 0; k < 3; ++k) l[k] = std::min(l[k], kv.first[k] * STORE_CS), h[k] = std::max(h[k], kv.first[k] * STORE_CS + STORE_CS - 1);
  }
  WS_TRY(mesh_corners_fit(l, h, map_resolution, "ws_store_mesh"));
  if (h[0] == l[0] || h[1] == l[1] || h[2] == l[2]) return mesh_publish(q, 0, 0, n_vertices, n_faces); // one voxel thick along an axis: no cells
  std::vector<StoreKey> keys;
  WS_TRY(store_mesh_tables(st, l, h, keys));
  if (keys.empty()) return mesh_publish(q, 0, 0, n_vertices, n_faces); // the box meets no present chunk
  if (keys.size() >= (1u << 19)) return range_error("ws_store_mesh", ": the box overlaps 2^19 present chunks or more (4096 words each must stay below 2^31)");
  StoreMeshCall c;
  c.n_chunks = (uint32_t)keys.size();
  c.res = map_resolution;
  c.flags = flags;
  copy3(c.lo, l), copy3(c.hi, h);
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
  if (!st) return invalid("ws_debug_store_mesh_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->mesh.timer, enable, ms_out, MESH_PAIRS, 3);
}

static int store_raycast(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin[3], const int32_t *dirs, bool dirs_on_host, size_t n,
                         int32_t max_range, int32_t res, uint32_t flags, size_t *n_hits)
{
  WS_TRY(raycast_check("ws_store_raycast", !st || ((lo == nullptr) != (hi == nullptr)), origin, dirs, n, max_range, res, flags, [&] {
    if (lo)
      for (int k = 0; k < 3; ++k)
        if (hi[k] < lo[k]) return invalid("ws_store_raycast: hi < lo");
    return res <= 0 ? invalid("ws_store_raycast: map_resolution <= 0") : (int)WS_OK;
  }));
  std::lock_guard<std::mutex> lock(st->mu);
  ws_store::Ray &q = st->ray;
  StoreRayCall c;
  c.res = res;
  std::vector<StoreRaySlot> listed;
  const auto list = [&](const StoreKey &key, uint32_t slot) { listed.push_back(StoreRaySlot{key[0], key[1], key[2], slot}); };
  if (lo)
  {
    copy3(c.lo, lo), copy3(c.hi, hi);
    store_walk_box(st, lo, hi, list);
  }
  else
  {
    for (int k = 0; k < 3; ++k) c.lo[k] = INT32_MIN, c.hi[k] = INT32_MAX; // everything
    for (const auto &kv : st->dir)
      if (kv.second.written) list(kv.first, kv.second.slot);
  }
  if (listed.size() >= (1u << 19)) return range_error("ws_store_raycast", ": the call lists 2^19 present chunks or more");
  c.n_chunks = (uint32_t)listed.size();
  // the live box: the bounding box of the listed chunks (keys are floor(int32 / 64): 64 k + 63 fits), cut to the box
  for (int k = 0; k < 3; ++k) c.blo[k] = INT32_MAX, c.bhi[k] = INT32_MIN;
  for (const StoreRaySlot &e : listed)
  {
    const int32_t key[3] = {e.cx, e.cy, e.cz};
    for (int k = 0; k < 3; ++k) c.blo[k] = std::min(c.blo[k], key[k] * STORE_CS), c.bhi[k] = std::max(c.bhi[k], key[k] * STORE_CS + STORE_CS - 1);
  }
  for (int k = 0; k < 3; ++k) c.blo[k] = std::max(c.blo[k], c.lo[k]), c.bhi[k] = std::min(c.bhi[k], c.hi[k]);
  // (no listed chunk: the call still launches and answers no-hit for every ray)
  const size_t places = c.n_chunks ? store_ray_table_slots(c.n_chunks) : 0;
  return raycast_run(
      q, st->ctx->stream, dirs, dirs_on_host, n, flags, n_hits, places > q.table_host.cap,
      [&] {
        if (places > q.table_host.cap)
        {
          WS_TRY(q.table_host.alloc(places, sizeof(StoreRaySlot), HostBlock::PINNED));
          WS_TRY(q.table_dev.alloc(places, sizeof(StoreRaySlot)));
        }
        if (c.n_chunks) store_ray_table_fill(listed.data(), listed.size(), q.table_host.as<StoreRaySlot>());
        return (int)WS_OK;
      },
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
  if (!st) return invalid("ws_debug_store_raycast_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->ray.timer, enable, ms_out, RAY_PAIRS, 3);
}

// ---- the distance field of the store: the rules and the host flow of ws_map_distance over the chunks, store_distance.hip
int ws_store_distance(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t max_dist_vox, uint32_t flags, size_t *n_sites)
{
  std::unique_lock<std::mutex> lock;
  StoreDistCall c;
  uint32_t ext[3];
  size_t n = 0;
  WS_TRY(distance_check(
      "ws_store_distance", !st, lo, hi, max_dist_vox, flags,
      [&](uint64_t e[3]) {
        if (lo)
          for (int k = 0; k < 3; ++k)
            if (hi[k] < lo[k]) return invalid("ws_store_distance: hi < lo");
        lock = std::unique_lock<std::mutex>(st->mu);
        WS_TRY(st->dist.timer.arm());
        if (lo)
          copy3(c.lo, lo), copy3(c.hi, hi);
        else
        {
          if (st->dir.empty()) return (int)WS_OK; // nothing to do: zero records
          // the bounding box of the present chunks (keys are floor(int32 / 64): 64 k + 63 fits)
          for (int k = 0; k < 3; ++k) c.lo[k] = INT32_MAX, c.hi[k] = INT32_MIN;
          for (const auto &kv : st->dir)
            for (int k = 0; k < 3; ++k) c.lo[k] = std::min(c.lo[k], kv.first[k] * STORE_CS), c.hi[k] = std::max(c.hi[k], kv.first[k] * STORE_CS + STORE_CS - 1);
        }
        for (int k = 0; k < 3; ++k) e[k] = (uint64_t)((int64_t)c.hi[k] - (int64_t)c.lo[k]) + 1u;
        return (int)WS_OK;
      },
      ext, &n));
  ws_store::Dist &q = st->dist;
  hipStream_t s = st->ctx->stream;
  // the present chunks the box overlaps, and the z range they cover inside it
  std::vector<StoreRaySlot> listed;
  if (n) store_walk_box(st, c.lo, c.hi, [&](const StoreKey &key, uint32_t slot) { listed.push_back(StoreRaySlot{key[0], key[1], key[2], slot}); });
  if (listed.size() >= (1u << 19)) return range_error("ws_store_distance", ": the box overlaps 2^19 present chunks or more");
  c.n_chunks = (uint32_t)listed.size();
  c.nx = ext[0], c.ny = ext[1];
  c.zlo = 1, c.zhi = 0;
  if (c.n_chunks)
  {
    c.zlo = INT32_MAX, c.zhi = INT32_MIN;
    for (const StoreRaySlot &e : listed) c.zlo = std::min(c.zlo, e.cz * STORE_CS), c.zhi = std::max(c.zhi, e.cz * STORE_CS + STORE_CS - 1);
    c.zlo = std::max(c.zlo, c.lo[2]), c.zhi = std::min(c.zhi, c.hi[2]);
  }
  return store_enqueued(st, distance_run(q, s, ext, max_dist_vox, flags, n, n_sites, [&] {
    const size_t places = c.n_chunks ? store_ray_table_slots(c.n_chunks) : 0;
    if (places > q.table_host.cap)
    {
      WS_HIP(hipStreamSynchronize(s));
      WS_TRY(q.table_host.alloc(places, sizeof(StoreRaySlot), HostBlock::PINNED));
      WS_TRY(q.table_dev.alloc(places, sizeof(StoreRaySlot)));
    }
    if (c.n_chunks) store_ray_table_fill(listed.data(), listed.size(), q.table_host.as<StoreRaySlot>());
    return launch_store_dist_classify(st, q, c, max_dist_vox, flags);
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
  if (!st) return invalid("ws_debug_store_distance_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->dist.timer, enable, ms_out, DIST_PAIRS, 4);
}

int ws_debug_store_raycast_table(const int32_t *keys_slots, size_t n, int32_t *table, size_t capacity_places, size_t *n_places)
{
  if ((n && table && !keys_slots) || !n_places || n >= (1u << 19)) return invalid("ws_debug_store_raycast_table: bad argument");
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

int ws_map_get_params(const ws_map *m, int which, int32_t size[3], int32_t pos[3], int32_t offset[3])
{
  if (!m || (which != WS_MAP_AVG && which != WS_MAP_NEW)) return invalid("ws_map_get_params: bad argument");
  if (size) copy3(size, m->par[which].size);
  if (pos) copy3(pos, m->par[which].pos);
  if (offset) copy3(offset, m->par[which].offset);
  return WS_OK;
}

void *ws_map_device_data(ws_map *m, int which)
{
  if (!m || (which != WS_MAP_AVG && which != WS_MAP_NEW)) return nullptr;
  return m->data[which].p;
}

int64_t ws_map_n_voxels(const ws_map *m) { return m ? m->n_vox : 0; }

// ------------------------------------------------------------------ TSDF update
int ws_tsdf_set_integrate(ws_map *m, int mode)
{
  if (m) WS_SETTLE(m);
  if (!m || (mode != WS_INTEGRATE_SPARSE && mode != WS_INTEGRATE_DENSE && mode != WS_INTEGRATE_SPARSE_SEPARATE))
    return invalid("ws_tsdf_set_integrate: bad argument");
  m->integrate_mode = mode;
  return WS_OK;
}

int ws_tsdf_set_capacity(ws_map *m, uint64_t records)
{
  if (!m) return invalid("ws_tsdf_set_capacity: map is NULL");
  WS_SETTLE(m);
  WS_HIP(hipStreamSynchronize(m->ctx->stream));
  return map_alloc_records(m, (records + SUB_RECS - 1) / SUB_RECS);
}

int ws_debug_tsdf_chunk_policy(ws_map *m, uint64_t budget_bytes, uint32_t est_shift)
{
  if (!m) return invalid("ws_debug_tsdf_chunk_policy: map is NULL");
  WS_SETTLE(m);
  m->chunk_budget_bytes = budget_bytes;
  m->est_shift = est_shift;
  return WS_OK;
}

static int too_many_points(size_t n)
{
  // update_tsdf.cu:146-150: message, no work
  char buf[160];
  snprintf(buf, sizeof buf, "TSDF update with %zu points, larger than the maximum of %zu", n, MAX_SCAN_POINTS);
  set_error(buf);
  return WS_ERR_TOO_MANY_POINTS;
}

int ws_tsdf_scatter_dev(ws_map *m, const int32_t *xyz_dev, size_t n, const int32_t scanner_pos[3], const int32_t up[3])
{
  if (!m || (!xyz_dev && n) || !scanner_pos || !up) return invalid("ws_tsdf_scatter_dev: NULL argument");
  if (n > MAX_SCAN_POINTS) return too_many_points(n);
  servers_leave(m->ctx);
  int rc = launch_tsdf_scatter(m, xyz_dev, n, scanner_pos, up, false);
  if (rc == WS_OK && n) m->new_is_default = false; // new_map now carries the scan until it is integrated
  return rc;
}

int ws_tsdf_integrate(ws_map *m)
{
  if (!m) return invalid("ws_tsdf_integrate: map is NULL");
  servers_leave(m->ctx);
  const int rc0 = settle_tsdf(m);
  if (rc0 != WS_OK) return rc0;
  return launch_tsdf_integrate(m);
}

int ws_tsdf_update_dev(ws_map *m, const int32_t *xyz_dev, size_t n, const int32_t scanner_pos[3], const int32_t up[3])
{
  if (!m || (!xyz_dev && n) || !scanner_pos || !up) return invalid("ws_tsdf_update_dev: NULL argument");
  if (n > MAX_SCAN_POINTS) return too_many_points(n);
  servers_leave(m->ctx);
  int rc;
  // with the default (sparse) integrate the tile resolve folds cu_avg_tsdf_krnl into its write-back (new_map stays
  // (tau, 0)); a non-default new_map is resolved on top of its entries and integrated by the dense pass
  prof_begin(m->ctx, WS_K_UPDATE);
  rc = launch_tsdf_scatter(m, xyz_dev, n, scanner_pos, up, m->integrate_mode == WS_INTEGRATE_SPARSE);
  if (rc == WS_OK) rc = launch_tsdf_integrate(m);
  if (m->pending.active.load(std::memory_order_relaxed)) m->pending.integrate_after = true; // (what a repeat of this scan has to be followed by; the caller holds the map exclusively here)
  prof_end(m->ctx, WS_K_UPDATE);
  return rc;
}

int ws_tsdf_update(ws_map *m, const int32_t *xyz_host, size_t n, const int32_t scanner_pos[3], const int32_t up[3])
{
  if (!m || (!xyz_host && n) || !scanner_pos || !up) return invalid("ws_tsdf_update: NULL argument");
  if (n > MAX_SCAN_POINTS) return too_many_points(n);
  if (n)
  {
    // (scan_dev is what a repeat of the PREVIOUS scan would read -- its verdict first, then the new points)
    WS_SETTLE(m);
    // pageable source: hipMemcpyAsync stages the data before it returns, like the reference's cudaMemcpy (update_tsdf.cu:152)
    WS_HIP(hipMemcpyAsync(m->scan_dev.p, xyz_host, n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, m->ctx->stream));
  }
  return ws_tsdf_update_dev(m, m->scan_dev.as<int32_t>(), n, scanner_pos, up);
}

int ws_tsdf_stats(ws_map *m, ws_tsdf_stats_t *out)
{
  if (!m || !out) return invalid("ws_tsdf_stats: NULL argument");
  {
    const int rcs = settle_tsdf(m);
    if (rcs != WS_OK) return rcs;
    const int rc0 = launch_tsdf_stats(m);
    if (rc0 != WS_OK) return rc0;
  }
  WS_HIP(hipMemcpyAsync(m->counters_host.p, m->counters.p, sizeof(TsdfCounters), hipMemcpyDeviceToHost, m->ctx->stream));
  WS_HIP(hipStreamSynchronize(m->ctx->stream));
  const TsdfCounters *c = m->counters_host.as<TsdfCounters>();
  out->contested_voxels = c->last_contested;
  out->records = c->last_records;
  out->tiles = (int64_t)c->last_listed + c->last_unlisted;
  out->runs = c->last_runs;
  out->free_space_hits = c->last_free_keyed;
  out->record_slots = (int64_t)c->last_need;
  out->record_capacity = (int64_t)m->sub_cap * SUB_RECS;
  const int rc = map_take_error(m);
  out->error_flags = (int32_t)m->last_error_bits;
  out->hash_entries = (int32_t)m->status.as<uint32_t>()[10];
  m->last_error_bits = 0;
  return rc;
}

// ------------------------------------------------------------------ registration
int ws_reg_destroy(ws_reg *r)
{
  if (!r) return WS_OK;
  servers_leave(r->ctx);
  {
    std::lock_guard<std::mutex> lock(r->ctx->lists_mu);
    auto &v = r->ctx->regs;
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i] == r)
      {
        v.erase(v.begin() + (long)i);
        break;
      }
  }
  (void)hipStreamSynchronize(r->ctx->stream);
  (void)ws_reg_peer_disconnect(r);
  r->release();
  delete r;
  return WS_OK;
}

static int reg_reserve(ws_reg *r, size_t n)
{
  if (n <= r->points.cap) return WS_OK;
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  return r->points.grow(n, 3 * sizeof(int32_t), DevBuf::EXACT);
}

// the allocations and first contents of a registration; on an error ws_reg_create frees what is there
static int reg_build(ws_reg *r, size_t max_points)
{
  WS_TRY(reg_reserve(r, max_points));
  WS_TRY(r->partials.alloc(reg_partials_bytes()));
  WS_TRY(r->state.alloc(2, sizeof(GnState)));
  WS_TRY(r->sums_dev.alloc(44, sizeof(int64_t)));
  WS_TRY(r->state_host.alloc(1, sizeof(GnState), HostBlock::PINNED));
  WS_TRY(r->host_flag.alloc(16, sizeof(int32_t), HostBlock::MAPPED));
  WS_TRY(r->result_host.alloc(1, sizeof(GnState), HostBlock::MAPPED));
  WS_TRY(r->iter_host.alloc(64, sizeof(int64_t), HostBlock::MAPPED, true));
  WS_HIP(hipMemsetAsync(r->state.p, 0, 2 * sizeof(GnState), r->ctx->stream));
  WS_TRY(r->grid_bar.alloc(reg_barrier_bytes()));
  WS_TRY(r->pass_arrived.alloc(1, sizeof(uint32_t)));
  WS_HIP(hipMemset(r->pass_arrived.p, 0, sizeof(uint32_t)));
  r->loop_supported = reg_loop_supported(r->ctx->device);
  WS_TRY(r->srv_mail.alloc(reg_server_mail_bytes(), 1, HostBlock::MAPPED, true));
  WS_TRY(r->srv_ctl.alloc(reg_server_ctl_bytes()));
  WS_HIP(hipMemset(r->srv_ctl.p, 0, reg_server_ctl_bytes()));
  if (const char *env = std::getenv("WS_REG_SERVER")) r->srv_enabled = std::atoi(env) != 0;
  if (const char *env = std::getenv("WS_REG_SERVER_IDLE_US")) r->srv_idle_us = (uint32_t)std::max(1, std::atoi(env));
  r->batch_variant = reg_batch_default_variant();
  if (const char *env = std::getenv("WS_REG_BATCH_VARIANT")) r->batch_variant = std::atoi(env) & 1;
  return WS_OK;
}

int ws_reg_create(ws_context *ctx, size_t max_points, ws_reg **out)
{
  if (!ctx || !out) return invalid("ws_reg_create: NULL argument");
  ws_reg *r = new (std::nothrow) ws_reg();
  if (!r) return invalid("ws_reg_create: out of host memory");
  r->ctx = ctx;
  if (max_points == 0) max_points = 128 * 1024; // registration.cu:261
  const int rc = reg_build(r, max_points);
  if (rc != WS_OK)
  {
    ws_reg_destroy(r);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lock(ctx->lists_mu);
    ctx->regs.push_back(r);
  }
  *out = r;
  return WS_OK;
}

int ws_reg_prepare(ws_reg *r, const int32_t *xyz_host, size_t n)
{
  if (!r || (!xyz_host && n)) return invalid("ws_reg_prepare: NULL argument");
  servers_leave(r->ctx); // (a resident server of ws_reg_iterate keeps the cloud in registers: the copy below is ordered behind it)
  int rc = reg_reserve(r, n);
  if (rc != WS_OK) return rc;
  r->n = n;
  if (n) WS_HIP(hipMemcpyAsync(r->points.p, xyz_host, n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, r->ctx->stream));
  return WS_OK;
}

int ws_reg_prepare_dev(ws_reg *r, const int32_t *xyz_dev, size_t n)
{
  if (!r || (!xyz_dev && n)) return invalid("ws_reg_prepare_dev: NULL argument");
  servers_leave(r->ctx);
  int rc = reg_reserve(r, n);
  if (rc != WS_OK) return rc;
  r->n = n;
  if (n) WS_HIP(hipMemcpyAsync(r->points.p, xyz_dev, n * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, r->ctx->stream));
  return WS_OK;
}

const int32_t *ws_reg_points_dev(const ws_reg *r, size_t *n)
{
  if (n) *n = r ? r->n : 0;
  return r ? r->points.as<int32_t>() : nullptr;
}

// ws_reg_iterate through the resident server (reg_server_kernel): see there.  Returns WS_OK with the 44 sums, or an error.
static int reg_iterate_served(ws_reg *r, const ws_map *m, const float T[16], int32_t res, uint32_t flags, int64_t sums[44])
{
  auto exited = [&]() { return reg_server_mail_exited(r->srv_mail.p); };
  uint32_t id = r->srv_launch.load(std::memory_order_acquire);
  bool alive = id != 0 && exited() != id;
  const MapParams &par = m->par[WS_MAP_AVG];
  const bool same = r->srv_sig.map == m && r->srv_sig.points == r->points.p && r->srv_sig.map_data == m->data[WS_MAP_AVG].p && r->srv_sig.n == r->n &&
                    r->srv_sig.res == res && r->srv_sig.flags == flags && std::memcmp(&r->srv_sig.par, &par, sizeof par) == 0;
  if (alive && (!same || r->srv_stopping.load(std::memory_order_acquire)))
  {
    // somebody has enqueued other work behind that server (or the call is for another map / cloud): it must be gone before a
    // request may be written -- it would answer from the state it was launched with
    reg_server_mail_stop(r->srv_mail.p, id);
    const int rc = spin_wait(r, [&] { return exited() == id; }, "ws_reg_iterate: the resident server did not leave");
    if (rc != WS_OK) return rc;
    alive = false;
  }
  uint32_t seq = r->srv_seq + 1;
  if (seq >= 0x7fffffffu) seq = 1;
  r->srv_seq = seq;
  reg_server_mail_write(r->srv_mail.p, T, seq);
  auto launch = [&]() -> int {
    id = ++r->srv_ids ? r->srv_ids : ++r->srv_ids;
    r->srv_sig.map = m;
    r->srv_sig.points = r->points.p;
    r->srv_sig.map_data = m->data[WS_MAP_AVG].p;
    r->srv_sig.n = r->n;
    r->srv_sig.res = res;
    r->srv_sig.flags = flags;
    r->srv_sig.par = par;
    r->srv_stopping.store(false, std::memory_order_release);
    r->srv_launch.store(id, std::memory_order_release);
    r->srv_launches += 1;
    return launch_reg_server(r, m, res, flags, id, r->srv_served, r->srv_idle_us);
  };
  if (!alive)
  {
    const int rc = launch();
    if (rc != WS_OK) return rc;
  }
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0;
  while (!reg_server_mail_answer(r->srv_mail.p, seq, sums))
  {
    if (exited() == id)
    {
      // the server left (idle for too long, or asked to by another thread's call) without having seen this request
      if (reg_server_mail_answer(r->srv_mail.p, seq, sums)) break;
      const int rc = launch();
      if (rc != WS_OK) return rc;
    }
    if ((++spins & 0xfffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20))
    {
      // Not an error yet: the server may be waiting in the stream behind somebody else's work (another thread's upload of a large
      // map takes longer than this).  Drain the stream the ordinary way -- a server that starts finds the request, answers it and
      // leaves when nothing else comes -- and only then look again; a kernel that never ends is the runtime's to report.
      WS_HIP(hipStreamSynchronize(r->ctx->stream));
      if (reg_server_mail_answer(r->srv_mail.p, seq, sums)) break;
      if (exited() == id)
      {
        // (it left on another thread's request without having seen this one: the next turn of the loop starts a new one)
        const int rc = launch();
        if (rc != WS_OK) return rc;
        WS_HIP(hipStreamSynchronize(r->ctx->stream));
        if (reg_server_mail_answer(r->srv_mail.p, seq, sums)) break;
      }
      set_error("ws_reg_iterate: the resident server did not answer");
      return WS_ERR_INTERNAL;
    }
  }
  r->srv_served = seq;
  return WS_OK;
}

int ws_reg_iterate(ws_reg *r, const ws_map *m, const float T[16], int32_t res, uint32_t flags, int64_t h[36], int64_t g[6],
                   int32_t *e, int32_t *c)
{
  if (!r || !m || !T || !h || !g || !e || !c) return invalid("ws_reg_iterate: NULL argument");
  if (res < 1) return invalid("ws_reg_iterate: map_resolution must be positive");
  int64_t sums[44];
  if (r->srv_enabled && r->loop_supported)
  {
    // (no WS_SETTLE here: that would ask the server to leave.  A scan whose verdict is open was enqueued by a call that has
    // already done so, and is settled now; a living server implies a settled map)
    const int rcs = ws::settle_tsdf(const_cast<ws_map *>(m));
    if (rcs != WS_OK) return rcs;
    const int rc = reg_iterate_served(r, m, T, res, flags, sums);
    if (rc != WS_OK) return rc;
  }
  else
  {
    WS_SETTLE(m);
    // One launch, nothing copied by the runtime: the pose travels in the kernel arguments (registration.cu:351 copies it), the
    // sums come back through host-mapped memory with the call's sequence number behind them (registration.cu:356-365 copies
    // four results and adds 32 partials up on the host).  The caller cannot go on without them, so the wait is a spin on that word.
    const uint32_t seq = ++r->iter_seq ? r->iter_seq : ++r->iter_seq; // (never 0: the block starts zeroed)
    int rc = launch_reg_pass(r, m, res, flags, 0, r->n, r->iter_host.dev_as<int64_t>(), 0, T, seq);
    if (rc != WS_OK) return rc;
    const volatile int64_t *done = r->iter_host.as<int64_t>() + 44;
    rc = spin_wait(r, [&] { return (uint32_t)*done == seq; }, "ws_reg_iterate: the launch ended without its result");
    if (rc != WS_OK) return rc;
    std::memcpy(sums, r->iter_host.p, sizeof sums);
  }
  std::memcpy(h, sums, 36 * sizeof(int64_t));
  std::memcpy(g, sums + 36, 6 * sizeof(int64_t));
  *e = (int32_t)sums[42];
  *c = (int32_t)sums[43];
  return map_take_error(const_cast<ws_map *>(m));
}

// test / tuning entry: the resident server of ws_reg_iterate on or off, its idle time; returns the servers launched so far
int ws_debug_reg_mail_selftest(void) { return reg_server_mail_selftest(); }

int ws_debug_reg_server(ws_reg *r, int32_t enable, int32_t idle_us, int32_t *launches)
{
  if (!r) return invalid("ws_debug_reg_server: reg is NULL");
  servers_leave(r->ctx);
  if (enable >= 0) r->srv_enabled = enable ? 1 : 0;
  if (idle_us > 0) r->srv_idle_us = (uint32_t)idle_us;
  if (launches) *launches = (int32_t)r->srv_launches;
  return WS_OK;
}

int ws_reg_begin(ws_reg *r, const float T_in[16], int32_t max_iterations, float it_weight_gradient, float epsilon)
{
  if (!r || !T_in) return invalid("ws_reg_begin: NULL argument");
  GnState *h = r->state_host.as<GnState>();
  // the pinned staging block may still be read by an earlier async copy
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  std::memset(h, 0, sizeof(GnState));
  h->core = gn_init(T_in, max_iterations, it_weight_gradient, epsilon);
  *r->host_flag.as<volatile int32_t>() = 0;
  WS_HIP(hipMemcpyAsync(&r->state.as<GnState>()[0], h, sizeof(GnState), hipMemcpyHostToDevice, r->ctx->stream));
  WS_HIP(hipMemcpyAsync(&r->state.as<GnState>()[1], h, sizeof(GnState), hipMemcpyHostToDevice, r->ctx->stream));
  r->latest = 0;
  return WS_OK;
}

int ws_reg_accumulate_dev(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t first, size_t count, int64_t *sums_dev)
{
  if (!r || !m || !sums_dev) return invalid("ws_reg_accumulate_dev: NULL argument");
  WS_SETTLE(m);
  return launch_reg_pass(r, m, res, flags, first, count, sums_dev, 0);
}

int ws_reg_iterate_shard_dev(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t first, size_t count, int64_t *sums_dev,
                             int32_t apply_previous)
{
  if (!r || !m || !sums_dev) return invalid("ws_reg_iterate_shard_dev: NULL argument");
  WS_SETTLE(m);
  return launch_reg_pass(r, m, res, flags, first, count, sums_dev, apply_previous);
}

int ws_reg_solve_dev(ws_reg *r, const int64_t *sums_dev)
{
  if (!r || !sums_dev) return invalid("ws_reg_solve_dev: NULL argument");
  return launch_reg_solve(r, sums_dev);
}

int ws_reg_poll(ws_reg *r, int32_t *finished, int32_t *iterations, float T_out[16])
{
  if (!r) return invalid("ws_reg_poll: reg is NULL");
  WS_HIP(hipMemcpyAsync(r->state_host.p, &r->state.as<GnState>()[r->latest], sizeof(GnState), hipMemcpyDeviceToHost, r->ctx->stream));
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  const GnCore *h = &r->state_host.as<GnState>()->core;
  if (finished) *finished = (h->finished || h->iterations >= h->max_iterations) ? 1 : 0;
  if (iterations) *iterations = h->iterations;
  if (T_out) std::memcpy(T_out, h->T, 16 * sizeof(float));
  return WS_OK;
}

// the host side of one resident launch: spin on the flag the kernel raises behind its result (host-mapped memory)
static int wait_resident_loop(ws_reg *r)
{
  const volatile int32_t *done = r->host_flag.as<int32_t>();
  return spin_wait(r, [&] { return *done != 0; }, "the resident registration loop ended without its result");
}

int ws_register_cloud(ws_reg *r, const ws_map *m, const float T_in[16], int32_t max_iterations, float it_weight_gradient,
                      float epsilon, int32_t res, uint32_t flags, float T_out[16], int32_t *iterations)
{
  if (!r || !m || !T_in || !T_out) return invalid("ws_register_cloud: NULL argument");
  WS_SETTLE(m);
  if (res < 1) return invalid("ws_register_cloud: map_resolution must be positive");
  if (r->loop_mode == WS_REG_LOOP_RESIDENT && r->loop_supported)
  {
    // one launch: the 256 workgroups stay resident and meet at a grid barrier between iterations.  The initial state
    // travels in the kernel arguments and the final state comes back through host-mapped memory, so the host neither
    // waits for earlier work on the stream before enqueueing nor copies anything afterwards.
    *r->host_flag.as<volatile int32_t>() = 0; // nothing on the stream writes it any more: every earlier registration was waited for
    int rc = launch_reg_loop(r, m, res, flags, gn_init(T_in, max_iterations, it_weight_gradient, epsilon));
    if (rc != WS_OK) return rc;
    r->latest = 0;
    // The kernel raises the flag in host-mapped memory after its result (release at system scope).  Spinning on it instead of
    // hipStreamSynchronize: 84 -> ~35 us between the end of a registration and the first kernel of the next scan (measured).
    rc = wait_resident_loop(r);
    if (rc != WS_OK) return rc;
    const GnCore *h = &r->result_host.as<GnState>()->core;
    if (!h->error)
    {
      std::memcpy(T_out, h->T, 16 * sizeof(float));
      if (iterations) *iterations = h->iterations;
      return map_take_error(const_cast<ws_map *>(m));
    }
    // The grid barrier timed out: another kernel held compute units the resident grid needs (its workgroups must all
    // be on the chip at once).  Nothing was lost — the loop state is only ever produced from complete sums — so the
    // registration simply runs again with one launch per iteration, which needs no co-residency.
    r->resident_fallbacks += 1;
  }
  int rc = ws_reg_begin(r, T_in, max_iterations, it_weight_gradient, epsilon);
  if (rc != WS_OK) return rc;
  // One launch per iteration: launch k applies update k (from the partial sums launch k-1 left behind) and
  // accumulates for iteration k.  The host just enqueues; the device raises a flag in host-mapped memory on
  // convergence so the host can stop early (launches already enqueued exit at once).
  const volatile int32_t *flag = r->host_flag.as<int32_t>();
  int launched = 0;
  for (int k = 0; k <= max_iterations && !*flag; ++k)
  {
    rc = launch_reg_iteration(r, m, res, flags, k);
    if (rc != WS_OK) return rc;
    launched = k + 1;
  }
  r->latest = launched > 0 ? ((launched - 1) & 1) : 0;
  int fin = 0, iters = 0;
  rc = ws_reg_poll(r, &fin, &iters, T_out);
  if (rc != WS_OK) return rc;
  if (iterations) *iterations = iters;
  return map_take_error(const_cast<ws_map *>(m));
}

// ------------------------------------------------------------------ many start poses, one launch
static int reg_batch_reserve(ws_reg *r, size_t k)
{
  if (k <= r->batch.cap) return WS_OK;
  WS_HIP(hipStreamSynchronize(r->ctx->stream)); // (every batch call has waited for its kernel: nothing reads the old block)
  size_t cap = 64;
  while (cap < k) cap *= 2;
  return r->batch.grow(cap, reg_batch_record_bytes(), HostBlock::MAPPED);
}

int ws_register_cloud_batch(ws_reg *r, const ws_map *m, const float *T_in, size_t k, int32_t max_iterations, float it_weight_gradient,
                            float epsilon, int32_t res, uint32_t flags, float *T_out, int32_t *iterations, int32_t *e_out, int32_t *c_out)
{
  if (!r || !m || (k && (!T_in || !T_out))) return invalid("ws_register_cloud_batch: NULL argument");
  if (res < 1) return invalid("ws_register_cloud_batch: map_resolution must be positive");
  if (k > 0x7fffffffu) return invalid("ws_register_cloud_batch: more than 2^31 - 1 start poses");
  // (a living resident server of ws_reg_iterate is asked to leave here: the launch below is ordered behind it on the stream and
  // must not wait for its idle time to run out)
  WS_SETTLE(m);
  if (k == 0) return map_take_error(const_cast<ws_map *>(m));
  int rc = reg_batch_reserve(r, k);
  if (rc != WS_OK) return rc;
  for (size_t i = 0; i < k; ++i) reg_batch_write(r->batch.p, i, T_in + 16 * i);
  // One launch, nothing copied by the runtime: the start records are read from, and the results written to, host-mapped memory.
  // Neither the state buffers, the loop mode nor the sums of the single route are touched.
  rc = launch_reg_batch(r, m, res, flags, k, max_iterations, it_weight_gradient, epsilon);
  if (rc != WS_OK) return rc;
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  for (size_t i = 0; i < k; ++i)
    reg_batch_read(r->batch.p, k, i, T_out + 16 * i, iterations ? iterations + i : nullptr, e_out ? e_out + i : nullptr, c_out ? c_out + i : nullptr);
  return map_take_error(const_cast<ws_map *>(m));
}

int ws_reg_batch_best(const int32_t *e, const int32_t *c, size_t k, int32_t min_count, int64_t *best)
{
  if (!best || (k && (!e || !c))) return invalid("ws_reg_batch_best: NULL argument");
  int64_t b = -1;
  for (size_t i = 0; i < k; ++i)
  {
    if (c[i] < min_count || c[i] <= 0) continue; // (a mean over no points is no score)
    if (b < 0)
    {
      b = (int64_t)i;
      continue;
    }
    // e[i] / c[i] < e[b] / c[b] with positive counts, exactly: |e| and c are below 2^31, the products below 2^62
    const int64_t lhs = (int64_t)e[i] * (int64_t)c[b], rhs = (int64_t)e[b] * (int64_t)c[i];
    if (lhs < rhs || (lhs == rhs && c[i] > c[b])) b = (int64_t)i;
  }
  *best = b;
  return WS_OK;
}

// ------------------------------------------------------------------ multi-GPU resident loop
static int peer_own_mailbox(ws_reg *r)
{
  if (r->mailbox.p) return WS_OK;
  // fine-grained: coherent for system-scope atomics from every GPU that maps it (and for the polls of the owner).  The one
  // allocation DevBuf does not make itself; it frees it like any other
  WS_HIP(hipExtMallocWithFlags(&r->mailbox.p, 4096, hipDeviceMallocFinegrained));
  r->mailbox.cap = 4096;
  WS_HIP(hipMemset(r->mailbox.p, 0, 4096));
  return WS_OK;
}

int ws_reg_peer_mailbox(ws_reg *r, void *ipc_handle_out)
{
  if (!r) return invalid("ws_reg_peer_mailbox: reg is NULL");
  static_assert(sizeof(hipIpcMemHandle_t) == WS_IPC_HANDLE_BYTES, "WS_IPC_HANDLE_BYTES");
  int rc = peer_own_mailbox(r);
  if (rc != WS_OK) return rc;
  if (ipc_handle_out)
  {
    hipIpcMemHandle_t h;
    WS_HIP(hipIpcGetMemHandle(&h, r->mailbox.p));
    std::memcpy(ipc_handle_out, &h, sizeof h);
  }
  return WS_OK;
}

int ws_reg_peer_disconnect(ws_reg *r)
{
  if (!r) return WS_OK;
  if (r->peer_world) (void)hipStreamSynchronize(r->ctx->stream);
  for (int i = 0; i < 8; ++i)
  {
    if (r->peer_opened[i] && r->peer_mailbox[i]) (void)hipIpcCloseMemHandle(r->peer_mailbox[i]);
    r->peer_opened[i] = false;
    r->peer_mailbox[i] = nullptr;
  }
  r->peer_world = 0;
  return WS_OK;
}

static int peer_finish_connect(ws_reg *r, int rank, int world, int blocks)
{
  if (blocks <= 0) blocks = reg_default_blocks();
  if (blocks % reg_groups() != 0 || blocks > reg_default_blocks()) return invalid("ws_reg_peer_connect: blocks must be a multiple of 8, at most 256");
  std::vector<unsigned char> image(reg_peer_block_bytes());
  reg_peer_block_fill(image.data(), r->peer_mailbox, rank, world);
  if (!r->peer_block_dev.p) WS_TRY(r->peer_block_dev.alloc(reg_peer_block_bytes()));
  WS_HIP(hipMemcpy(r->peer_block_dev.p, image.data(), image.size(), hipMemcpyHostToDevice)); // also zeroes `then`: the mailboxes are fresh
  WS_HIP(hipMemset(r->mailbox.p, 0, reg_mailbox_bytes()));
  r->peer_rank = rank;
  r->peer_world = world;
  r->peer_blocks = blocks;
  r->peer_dirty = false;
  return WS_OK;
}

int ws_reg_peer_connect(ws_reg *r, int32_t rank, int32_t world, const void *ipc_handles, int32_t blocks)
{
  if (!r || !ipc_handles) return invalid("ws_reg_peer_connect: NULL argument");
  if (world < 1 || world > 8 || rank < 0 || rank >= world) return invalid("ws_reg_peer_connect: 1 <= world <= 8, 0 <= rank < world");
  int rc = peer_own_mailbox(r);
  if (rc != WS_OK) return rc;
  (void)ws_reg_peer_disconnect(r);
  // the mailboxes of ranks on other GPUs are reached over xGMI: peer access to every visible device (already enabled / not
  // possible are both fine here: the open below decides)
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess)
    for (int d = 0; d < n_dev; ++d)
      if (d != r->ctx->device)
      {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, r->ctx->device, d) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(d, 0);
      }
  (void)hipGetLastError();
  for (int i = 0; i < world; ++i)
  {
    if (i == rank)
    {
      r->peer_mailbox[i] = r->mailbox.p;
      continue;
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, static_cast<const unsigned char *>(ipc_handles) + (size_t)i * sizeof h, sizeof h);
    void *p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess)
    {
      (void)ws_reg_peer_disconnect(r);
      return hip_fail(e, "hipIpcOpenMemHandle (mailbox of a peer rank)", __FILE__, __LINE__);
    }
    r->peer_mailbox[i] = p;
    r->peer_opened[i] = true;
  }
  return peer_finish_connect(r, rank, world, blocks);
}

int ws_reg_peer_connect_local(ws_reg *r, int32_t rank, int32_t world, ws_reg *const *regs, int32_t blocks)
{
  if (!r || !regs) return invalid("ws_reg_peer_connect_local: NULL argument");
  if (world < 1 || world > 8 || rank < 0 || rank >= world || regs[rank] != r) return invalid("ws_reg_peer_connect_local: regs[rank] must be reg, world <= 8");
  (void)ws_reg_peer_disconnect(r);
  for (int i = 0; i < world; ++i)
  {
    if (!regs[i]) return invalid("ws_reg_peer_connect_local: NULL rank");
    const int rc = peer_own_mailbox(regs[i]);
    if (rc != WS_OK) return rc;
    r->peer_mailbox[i] = regs[i]->mailbox.p;
  }
  return peer_finish_connect(r, rank, world, blocks);
}

int ws_reg_peer_reset(ws_reg *r)
{
  if (!r || !r->peer_world) return invalid("ws_reg_peer_reset: not connected");
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  return peer_finish_connect(r, r->peer_rank, r->peer_world, r->peer_blocks);
}

int ws_register_cloud_peers(ws_reg *r, const ws_map *m, size_t first, size_t count, const float T_in[16], int32_t max_iterations,
                            float it_weight_gradient, float epsilon, int32_t res, uint32_t flags, float T_out[16], int32_t *iterations)
{
  if (!r || !m || !T_in || !T_out) return invalid("ws_register_cloud_peers: NULL argument");
  WS_SETTLE(m);
  if (!r->peer_world) return invalid("ws_register_cloud_peers: ws_reg_peer_connect first");
  // An exchange that was given up leaves partial additions in the mailboxes and no saved snapshot: a rank's stale addition
  // plus its next one would reach count == world and pass for the all-rank total.  Nothing runs until the mailboxes are fresh.
  if (r->peer_dirty) return invalid("ws_register_cloud_peers: the last exchange failed; call ws_reg_peer_reset on every rank (between two barriers) or reconnect first");
  if (res < 1) return invalid("ws_register_cloud_peers: map_resolution must be positive");
  *r->host_flag.as<volatile int32_t>() = 0;
  r->peer_dirty = true; // until this exchange has completed on this rank
  int rc = launch_reg_loop(r, m, res, flags, gn_init(T_in, max_iterations, it_weight_gradient, epsilon), true, first, count);
  if (rc != WS_OK) return rc;
  r->latest = 0;
  rc = wait_resident_loop(r);
  if (rc != WS_OK) return rc;
  const GnCore *h = &r->result_host.as<GnState>()->core;
  if (h->error)
  {
    // a rank did not deliver (its kernel was not on the chip, or the process is gone): every rank times out within one
    // exchange of the first.  The caller re-runs the registration through the RCCL route (warpsense_amd.dist does) after
    // ws_reg_peer_reset on every rank.
    set_error("ws_register_cloud_peers: the exchange with the peer ranks timed out");
    return WS_ERR_TIMEOUT;
  }
  r->peer_dirty = false;
  std::memcpy(T_out, h->T, 16 * sizeof(float));
  if (iterations) *iterations = h->iterations;
  return map_take_error(const_cast<ws_map *>(m));
}

int ws_reg_set_loop(ws_reg *r, int mode)
{
  if (!r || (mode != WS_REG_LOOP_RESIDENT && mode != WS_REG_LOOP_LAUNCHES)) return invalid("ws_reg_set_loop: bad argument");
  r->loop_mode = mode;
  return WS_OK;
}

int ws_debug_block_stats(ws_map *m, uint32_t *out, size_t words)
{
  if (!m || !out) return invalid("ws_debug_block_stats: NULL argument");
  WS_SETTLE(m);
  if (words > WS_BLOCK_STATS) words = WS_BLOCK_STATS;
  WS_HIP(hipMemcpyAsync(out, m->block_stats.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, m->ctx->stream));
  WS_HIP(hipStreamSynchronize(m->ctx->stream));
  return WS_OK;
}

int ws_debug_reg_stall(ws_reg *r, int32_t stall_next, int32_t *fallbacks)
{
  if (!r) return invalid("ws_debug_reg_stall: NULL argument");
  r->debug_stall_next = stall_next ? 1 : 0;
  if (fallbacks) *fallbacks = r->resident_fallbacks;
  return WS_OK;
}

int ws_debug_reg_sums(ws_reg *r, int64_t sums_out[44])
{
  if (!r || !sums_out) return invalid("ws_debug_reg_sums: NULL argument");
  WS_HIP(hipMemcpyAsync(sums_out, r->state.as<GnState>()[r->latest].sums, 44 * sizeof(int64_t), hipMemcpyDeviceToHost, r->ctx->stream));
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  return WS_OK;
}

int ws_debug_solve6(ws_context *ctx, const double *A, const double *b, size_t n, double *x, int32_t *status)
{
  if (!ctx || !A || !b || !x || !status) return invalid("ws_debug_solve6: NULL argument");
  DevBuf dA, db, dx, ds;
  const size_t k = n ? n : 1;
  int rc = dA.alloc(k, 36 * sizeof(double));
  if (rc == WS_OK) rc = db.alloc(k, 6 * sizeof(double));
  if (rc == WS_OK) rc = dx.alloc(k, 6 * sizeof(double));
  if (rc == WS_OK) rc = ds.alloc(k, sizeof(int32_t));
  if (rc == WS_OK && n)
  {
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA.p, A, n * 36 * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db.p, b, n * 6 * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) rc = launch_solve6_test(ctx, dA.as<double>(), db.as<double>(), n, dx.as<double>(), ds.as<int32_t>());
    if (e == hipSuccess && rc == WS_OK) e = hipMemcpyAsync(x, dx.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == WS_OK) e = hipMemcpyAsync(status, ds.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = hip_fail(e, "ws_debug_solve6", __FILE__, __LINE__);
  }
  for (DevBuf *buf : {&dA, &db, &dx, &ds}) buf->release();
  return rc;
}

// ------------------------------------------------------------------ scan pre-processing
int ws_scan_destroy(ws_scan *sc)
{
  if (!sc) return WS_OK;
  (void)hipStreamSynchronize(sc->ctx->stream);
  sc->release();
  delete sc;
  return WS_OK;
}

// the allocations of a scan pre-processor; on an error ws_scan_create frees what is there
static int scan_build(ws_scan *sc)
{
  const size_t blocks = (sc->cap + 255) / 256;
  WS_TRY(sc->tmp.alloc(sc->cap, 3 * sizeof(int32_t)));
  WS_TRY(sc->out.alloc(sc->cap, 3 * sizeof(int32_t)));
  WS_TRY(sc->slot_of.alloc(sc->cap, sizeof(uint32_t)));
  WS_TRY(sc->keys.alloc(sc->table_slots, sizeof(uint64_t)));
  WS_TRY(sc->first.alloc(sc->table_slots, sizeof(uint32_t)));
  WS_TRY(sc->wg_count.alloc(blocks, sizeof(uint32_t)));
  WS_TRY(sc->wg_off.alloc(blocks, sizeof(uint32_t)));
  WS_TRY(sc->counters.alloc(16, sizeof(uint32_t)));
  return sc->host_count.alloc(16, sizeof(uint32_t), HostBlock::MAPPED);
}

int ws_scan_create(ws_context *ctx, size_t max_points, ws_scan **out)
{
  if (!ctx || !out) return invalid("ws_scan_create: NULL argument");
  if (max_points == 0) max_points = 128 * 1024;
  if (max_points > (1u << 30)) return invalid("ws_scan_create: too many points");
  ws_scan *sc = new (std::nothrow) ws_scan();
  if (!sc) return invalid("ws_scan_create: out of host memory");
  sc->ctx = ctx;
  sc->cap = max_points;
  sc->table_slots = pre_table_slots(max_points);
  const int rc = scan_build(sc);
  if (rc != WS_OK)
  {
    ws_scan_destroy(sc);
    return rc;
  }
  *out = sc;
  return WS_OK;
}

// to_int_mat, util/util.h:8-11
static void scan_int_mat(const float pose[16], int32_t M[16])
{
  for (int k = 0; k < 16; ++k) M[k] = (int32_t)(pose[k] * (float)MATRIX_RESOLUTION);
}

// the count and the error bits of the launches before it
static int scan_finish(ws_scan *sc, size_t *n_out)
{
  uint32_t counters[2] = {0, 0};
  WS_HIP(hipMemcpyAsync(counters, sc->counters.p, sizeof counters, hipMemcpyDeviceToHost, sc->ctx->stream));
  WS_HIP(hipStreamSynchronize(sc->ctx->stream));
  sc->n_out = counters[0];
  if (n_out) *n_out = sc->n_out;
  if (counters[1] & 1u)
  {
    set_error("ws_scan_preprocess: a transformed coordinate is beyond +-2^20 mm");
    return WS_ERR_RANGE;
  }
  return WS_OK;
}

static int scan_run(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const float pose[16], int32_t res, size_t *n_out)
{
  int32_t M[16];
  scan_int_mat(pose, M);
  int rc = launch_scan_preprocess(sc, xyz_dev, n, stride, M, res);
  if (rc != WS_OK) return rc;
  return scan_finish(sc, n_out);
}

int ws_scan_preprocess_dev(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const float pose[16], int32_t res, size_t *n_out)
{
  if (!sc || (!xyz_dev && n) || !pose) return invalid("ws_scan_preprocess_dev: NULL argument");
  if (stride < 3) return invalid("ws_scan_preprocess_dev: a point needs at least 3 floats");
  if (res < 1) return invalid("ws_scan_preprocess_dev: map_resolution must be positive");
  if (n > sc->cap) return invalid("ws_scan_preprocess_dev: more points than ws_scan_create reserved");
  return scan_run(sc, xyz_dev, n, stride, pose, res, n_out);
}

int ws_scan_preprocess(ws_scan *sc, const float *xyz_host, size_t n, size_t stride, const float pose[16], int32_t res, size_t *n_out)
{
  if (!sc || (!xyz_host && n) || !pose) return invalid("ws_scan_preprocess: NULL argument");
  if (stride < 3) return invalid("ws_scan_preprocess: a point needs at least 3 floats");
  if (res < 1) return invalid("ws_scan_preprocess: map_resolution must be positive");
  if (n > sc->cap) return invalid("ws_scan_preprocess: more points than ws_scan_create reserved");
  const size_t floats = n * stride;
  if (floats > sc->in_stage.cap)
  {
    WS_HIP(hipStreamSynchronize(sc->ctx->stream));
    WS_TRY(sc->in_stage.grow(floats, sizeof(float), DevBuf::EXACT));
  }
  if (floats) WS_HIP(hipMemcpyAsync(sc->in_stage.p, xyz_host, floats * sizeof(float), hipMemcpyHostToDevice, sc->ctx->stream));
  return scan_run(sc, sc->in_stage.as<float>(), n, stride, pose, res, n_out);
}

// ---- the sweep form: one pose per time bin
static int sweep_check(const char *who, ws_scan *sc, const float *xyz, size_t n, size_t stride, const float *poses, uint32_t k, const ws_sweep_t *rule, int32_t res)
{
  const std::string w(who);
  if (!sc || (!xyz && n) || !poses || !rule) return invalid(w + ": NULL argument");
  if (stride < 3) return invalid(w + ": a point needs at least 3 floats");
  if (res < 1) return invalid(w + ": map_resolution must be positive");
  if (n > sc->cap) return invalid(w + ": more points than ws_scan_create reserved");
  if (k < 1 || k > WS_SWEEP_MAX_BINS) return invalid(w + ": 1 <= k <= 4096 poses");
  if (rule->time_field == -1)
  {
    if (rule->columns < 1 || n % rule->columns != 0) return invalid(w + ": the point count is not a multiple of the sweep's columns");
  }
  else
  {
    if (rule->time_field < 3 || (size_t)rule->time_field >= stride) return invalid(w + ": time_field must be -1 or an index of the record after x y z");
    if (!std::isfinite(rule->t_begin) || !std::isfinite(rule->t_end) || rule->t_begin == rule->t_end) return invalid(w + ": t_begin and t_end must be finite and differ");
  }
  return WS_OK;
}

static int sweep_run(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const float *poses, uint32_t k, const ws_sweep_t *rule, int32_t res, size_t *n_out)
{
  hipStream_t s = sc->ctx->stream;
  if (!sc->sweep_table.p || !sc->sweep_stage.p)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(sc->sweep_table.alloc(WS_SWEEP_MAX_BINS, 16 * sizeof(int32_t)));
    WS_TRY(sc->sweep_stage.alloc(WS_SWEEP_MAX_BINS, 16 * sizeof(int32_t), HostBlock::PINNED));
  }
  // (every call on `sc` ends with a stream synchronise: the staging block of the call before has been read)
  int32_t *rows = sc->sweep_stage.as<int32_t>();
  for (uint32_t b = 0; b < k; ++b) scan_int_mat(poses + 16 * (size_t)b, rows + 16 * (size_t)b);
  WS_HIP(hipMemcpyAsync(sc->sweep_table.p, rows, (size_t)k * 16 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  PreSweep w;
  w.table = sc->sweep_table.as<int32_t>();
  w.k = k;
  const bool by_index = rule->time_field == -1;
  w.columns = by_index ? rule->columns : 1u;
  w.rows = by_index ? (uint32_t)(n / rule->columns) : (uint32_t)n;
  if (w.rows == 0) w.rows = 1; // (n == 0: nothing is launched)
  w.ring_major = rule->ring_major;
  w.time_field = rule->time_field;
  w.t_begin = rule->t_begin;
  w.t_end = rule->t_end;
  int rc = launch_scan_preprocess(sc, xyz_dev, n, stride, nullptr, res, &w);
  if (rc != WS_OK) return rc;
  return scan_finish(sc, n_out);
}

int ws_scan_preprocess_sweep_dev(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const float *poses_host, uint32_t k, const ws_sweep_t *rule,
                                 int32_t res, size_t *n_out)
{
  WS_TRY(sweep_check("ws_scan_preprocess_sweep_dev", sc, xyz_dev, n, stride, poses_host, k, rule, res));
  return sweep_run(sc, xyz_dev, n, stride, poses_host, k, rule, res, n_out);
}

int ws_scan_preprocess_sweep(ws_scan *sc, const float *xyz_host, size_t n, size_t stride, const float *poses_host, uint32_t k, const ws_sweep_t *rule,
                             int32_t res, size_t *n_out)
{
  WS_TRY(sweep_check("ws_scan_preprocess_sweep", sc, xyz_host, n, stride, poses_host, k, rule, res));
  const size_t floats = n * stride;
  if (floats > sc->in_stage.cap)
  {
    WS_HIP(hipStreamSynchronize(sc->ctx->stream));
    WS_TRY(sc->in_stage.grow(floats, sizeof(float), DevBuf::EXACT));
  }
  if (floats) WS_HIP(hipMemcpyAsync(sc->in_stage.p, xyz_host, floats * sizeof(float), hipMemcpyHostToDevice, sc->ctx->stream));
  return sweep_run(sc, sc->in_stage.as<float>(), n, stride, poses_host, k, rule, res, n_out);
}

// pure host code, in double (warpsense_hip.h)
int ws_sweep_poses(const float pose_end[16], const float motion[16], uint32_t k, float *poses_out)
{
  if (!pose_end || !motion || !poses_out) return invalid("ws_sweep_poses: NULL argument");
  if (k < 1 || k > WS_SWEEP_MAX_BINS) return invalid("ws_sweep_poses: 1 <= k <= 4096 poses");
  bool identity = true;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
    {
      if (!std::isfinite(pose_end[4 * c + r]) || !std::isfinite(motion[4 * c + r])) return invalid("ws_sweep_poses: non-finite input");
      identity = identity && motion[4 * c + r] == (r == c ? 1.f : 0.f);
    }
  if (identity)
  {
    for (uint32_t b = 0; b < k; ++b) std::memcpy(poses_out + 16 * (size_t)b, pose_end, 16 * sizeof(float));
    return WS_OK;
  }
  // Q = R_motion^T, u = -Q t_motion: the begin frame seen from the end frame (Q(r, c) = motion[4 r + c])
  double Q[3][3], u[3], P[4][4];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Q[r][c] = (double)motion[4 * r + c];
  for (int r = 0; r < 3; ++r) u[r] = -(Q[r][0] * (double)motion[12] + Q[r][1] * (double)motion[13] + Q[r][2] * (double)motion[14]);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) P[r][c] = (double)pose_end[4 * c + r];
  const double v[3] = {0.5 * (Q[2][1] - Q[1][2]), 0.5 * (Q[0][2] - Q[2][0]), 0.5 * (Q[1][0] - Q[0][1])};
  const double sn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), cs = 0.5 * (Q[0][0] + Q[1][1] + Q[2][2] - 1.0);
  if (cs < 0.0) return invalid("ws_sweep_poses: a rotation of more than 90 degrees within one sweep");
  const double angle = std::atan2(sn, cs);
  double a[3] = {0.0, 0.0, 0.0};
  if (sn > 0.0)
    for (int r = 0; r < 3; ++r) a[r] = v[r] / sn;
  const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
  double K2[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K2[r][c] = K[r][0] * K[0][c] + K[r][1] * K[1][c] + K[r][2] * K[2][c];
  for (uint32_t b = 0; b < k; ++b)
  {
    const double w = 1.0 - ((double)b + 0.5) / (double)k, sw = std::sin(w * angle), cw = 1.0 - std::cos(w * angle);
    double rel[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 1}};
    for (int r = 0; r < 3; ++r)
    {
      for (int c = 0; c < 3; ++c) rel[r][c] = (r == c ? 1.0 : 0.0) + sw * K[r][c] + cw * K2[r][c]; // Rodrigues
      rel[r][3] = w * u[r];
    }
    float *out = poses_out + 16 * (size_t)b;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) out[4 * c + r] = (float)(P[r][0] * rel[0][c] + P[r][1] * rel[1][c] + P[r][2] * rel[2][c] + P[r][3] * rel[3][c]);
  }
  return WS_OK;
}

const int32_t *ws_scan_points_dev(const ws_scan *sc) { return sc ? sc->out.as<int32_t>() : nullptr; }

int ws_scan_download(ws_scan *sc, int32_t *xyz_host, size_t capacity_points, size_t *n_out)
{
  if (!sc || !n_out) return invalid("ws_scan_download: NULL argument");
  *n_out = sc->n_out;
  if (sc->n_out == 0) return WS_OK;
  if (!xyz_host || capacity_points < sc->n_out) return invalid("ws_scan_download: buffer too small");
  WS_HIP(hipMemcpyAsync(xyz_host, sc->out.p, sc->n_out * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, sc->ctx->stream));
  WS_HIP(hipStreamSynchronize(sc->ctx->stream));
  return WS_OK;
}

// ------------------------------------------------------------------ measurement
int ws_prof_enable(ws_context *ctx, uint32_t class_mask)
{
  if (!ctx) return invalid("ws_prof_enable: ctx is NULL");
  WS_HIP(hipStreamSynchronize(ctx->stream));
  prof_resolve(ctx);
  ctx->prof_mask = class_mask;
  return WS_OK;
}

int ws_prof_read(ws_context *ctx, int cls, double *total_ms, int64_t *launches)
{
  if (!ctx || cls < 0 || cls >= WS_K_COUNT) return invalid("ws_prof_read: bad argument");
  WS_HIP(hipStreamSynchronize(ctx->stream));
  prof_resolve(ctx);
  if (total_ms) *total_ms = ctx->prof_ms[cls];
  if (launches) *launches = ctx->prof_n[cls];
  return WS_OK;
}

int ws_prof_reset(ws_context *ctx)
{
  if (!ctx) return invalid("ws_prof_reset: ctx is NULL");
  WS_HIP(hipStreamSynchronize(ctx->stream));
  prof_resolve(ctx);
  for (int k = 0; k < WS_K_COUNT; ++k)
  {
    ctx->prof_ms[k] = 0;
    ctx->prof_n[k] = 0;
  }
  return WS_OK;
}

} // extern "C"

namespace ws
{
int resize_records(ws_map *m, uint64_t sub_chunks)
{
  WS_HIP(hipStreamSynchronize(m->ctx->stream)); // nothing enqueued may still use the old buffers
  return map_alloc_records(m, sub_chunks);
}
} // namespace ws
