// api_map.hip — the host side of a map (ws_map_*, ws_shift_*): creation, upload and download, the record pool of the TSDF update,
// the sticky device error word, the box rules and box transfers, the plan of a shift and its host route (ws_shift_begin .. _end).
#include <algorithm>
#include <cmath>
#include <new>

#include "ws_api.h"

using namespace ws;

constexpr size_t AZ_ALLOC = 1024 * 64 + 8; // direction-bin histogram / offsets
static_assert(AZ_ALLOC >= (size_t)AZ_BINS + 2, "az_hist / az_off: AZ_BINS + 2 entries (ray_sort_kernel, tsdf_setup.hip)");

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

int ws::resize_records(ws_map *m, uint64_t sub_chunks)
{
  WS_HIP(hipStreamSynchronize(m->ctx->stream)); // nothing enqueued may still use the old buffers
  return map_alloc_records(m, sub_chunks);
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
int ws::map_take_error(ws_map *m)
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

int ws::check_all_equal_host(const uint32_t *data, int64_t n, uint32_t value)
{
  for (int64_t i = 0; i < n; ++i)
    if (data[i] != value) return 0;
  return 1;
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

// ---- box transfers: the device side of the map shift (only the slabs that leave / enter move)
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
int ws::resolve_box(const ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], bool allow_whole, const char *name, int32_t l[3], int32_t ext[3])
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

// ---- map shift
// The plan of a shift (ws_shift_plan; `name` is the entry point the refusal speaks for): per axis, like HDF5LocalMap::shift
// (hdf5_local_map.cpp:53-118), with the window as it is when that axis moves.  The window is pos - size/2 .. pos - size/2 + size - 1,
// every ring cell once: the reference's pos + size/2 for its odd sizes; for an even size pos + size/2 would be the ring cell of
// pos - size/2 again, filed under a second world position.
int ws::plan_shift(const int32_t size[3], const int32_t pos0[3], const int32_t offset0[3], const int32_t new_pos[3], const char *name, ws_shift_plan_t *out)
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
void ws::move_axis(MapParams par[2], int axis, int32_t d)
{
  for (int w = 0; w < 2; ++w)
  {
    MapParams &p = par[w];
    p.pos[axis] += d;
    p.offset[axis] = (int32_t)((((int64_t)p.offset[axis] + d) % p.size[axis] + p.size[axis]) % p.size[axis]);
  }
}

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
