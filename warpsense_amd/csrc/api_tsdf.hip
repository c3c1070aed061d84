// api_tsdf.hip — the entry points of the TSDF update (ws_tsdf_*): what they check, settle and enqueue; the kernels and their launchers
// are in tsdf_update.hip (the scatter's host logic; its stages in tsdf_setup / tail / free / resolve.hip) and tsdf_integrate.hip.
#include "ws_api.h"

using namespace ws;

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
  return resize_records(m, (records + SUB_RECS - 1) / SUB_RECS);
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

int ws_debug_block_stats(ws_map *m, uint32_t *out, size_t words)
{
  if (!m || !out) return invalid("ws_debug_block_stats: NULL argument");
  WS_SETTLE(m);
  if (words > WS_BLOCK_STATS) words = WS_BLOCK_STATS;
  WS_HIP(hipMemcpyAsync(out, m->block_stats.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, m->ctx->stream));
  WS_HIP(hipStreamSynchronize(m->ctx->stream));
  return WS_OK;
}
