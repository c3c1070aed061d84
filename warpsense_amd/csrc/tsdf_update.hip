// tsdf_update.hip — TSDF volume update for MI355X (gfx950).
//
// Replaces cu_min_tsdf_krnl + cu_avg_tsdf_krnl (src/warpsense/cuda/update_tsdf.cu:13-128) of the reference.
//
// The reference scatters with a racy CAS ("first positive-weight entry freezes the voxel",
// include/warpsense/cuda/util.h:70-102), so its result depends on thread arrival order.  This
// implementation computes the result of ONE fixed legal schedule — the serial one, ascending
// (point, ray step, fan step) — deterministically, without a single global atomic per candidate:
//
//   ray_setup / ray_sort     per-ray constants (update_tsdf.cu:52-63), rays sorted by the cell of the map their END lies in
//                            (the tail of a ray lies within tau of its end: 64 neighbours in that order put their records
//                            into the same few tiles).
//   march_tail_kernel        walks the ray TAILS once (near-surface and fan candidates: everything whose result
//                            depends on the order).  Every scatter target becomes an 8-byte record and goes STRAIGHT to
//                            its place: records live in 256-byte sub-chunks that belong to one 4x4x64-voxel tile each, a
//                            wave opens sub-chunks out of its own run of ids and counts its records per tile in LDS (the
//                            count is the place), and publishes its sub-chunks when it is through -- one atomic per
//                            (wave, tile).  No wave waits for another, HBM sees a record once.  (Round 4 built two other
//                            shapes first -- through a raw buffer and a copy, and staged in LDS: DESIGN.md §5.)  Off-ray
//                            candidates of value +tau are (tau, -64) whoever makes them and never take part in the
//                            order: a byte in the second voxel plane instead of a record.
//   march_free_kernel        walks the steps before the tails: all free space (tau, +64) whoever comes first ->
//                            one byte per voxel.  A free-space candidate landing on a voxel the tails marked joins that
//                            tile's records instead.
//   tile_resolve_kernel      ONE workgroup per touched 4x4x64-voxel tile: all candidates of the tile are present,
//                            so the canonical accept rule is a local fold in LDS (earliest positive / smallest
//                            negative keys, then exact rounds for the voxels where a negative-weight candidate
//                            may have blocked the earliest positive one).  Writes new_map, or — fused — integrates
//                            straight into avg_map (cu_avg_tsdf_krnl folded into the write-back).
//   integrate_*_kernel       weighted average of new_map into avg_map and reset of new_map, over the touched
//                            tiles only (sparse) or over every voxel (dense, the reference's kernel).
//
// The list of tiles with records is built on the way (the first entries of a tile append it): no scan over the tile grid, no
// descriptors.  new_map after the resolve is bit-identical to what the reference
// kernel leaves there when its threads run one after the other (oracle/ws_oracle.c: wso_update_min).
//
// The device code lies in two layers, each a header that includes the one before it, and a file per stage with its kernels, its own
// switches and the launcher this file calls:
//   tsdf_scatter.h      ScatterArgs, the switches more than one stage reads, error bits, voxel / tile / record addressing, the launchers
//   tsdf_pool.h         the record pool and the tile lists as the marches write them (tail march and free pass only)
//   tsdf_setup.hip      scatter_prep_kernel, ray_setup_kernel, ray_sort_kernel; the fan table (fill_fan_steps)
//   tsdf_tail.hip       march_tail_kernel
//   tsdf_free.hip       march_free_kernel
//   tsdf_resolve.hip    tile_resolve_kernel and its ResolveArgs
// This file is the host logic around them: one attempt of the scatter (enqueue_scatter), the verdict on it and the repeats
// (settle_tsdf), the entry of the update (launch_tsdf_scatter).
// Units: this file, tsdf_setup.hip and tsdf_resolve.hip each; tsdf_tail.hip and tsdf_free.hip together as tsdf_marches.hip, which says why.
#include <atomic>
#include <chrono>

#include "tsdf_scatter.h"

namespace ws
{
// Sub-chunks the pool should hold for a scan of `n_points` rays whose records are bounded by `need`: the block every
// workgroup of the tail march starts with, the records themselves (the bound counts every sample as a candidate, about 2.7 x
// what a scan makes; est_shift > 1 takes a fraction of it: tests), and room for the partly filled ones.  An estimate -- the
// number of (wave, tile) pairs has no useful bound -- and never more than that: a scan that does exhaust the pool is ABORTED
// (nothing of it reaches the maps) and repeated with more (launch_tsdf_scatter).
__host__ inline unsigned long long subs_needed(unsigned long long need, uint32_t est_shift, unsigned long long n_points)
{
  const unsigned long long items = (n_points + 63) / 64 * WS_TAIL_SPLIT + 1; // (TAIL_SPLIT workgroups per 64 rays)
  const unsigned long long free_waves = (n_points + 63) / 64 * 4; // (64 rays per workgroup of the free pass)
  return items * SUB_WG_BLOCK + free_waves * WS_FREE_FIRST + ((need >> SUB_BITS) >> (est_shift ? est_shift - 1 : 0)) + 8192ull;
}

uint64_t subs_for_scan(const ws_map *m, uint64_t need_records, uint64_t n_points) { return subs_needed(need_records, m->est_shift, n_points); }

// one attempt of the scatter: every kernel enqueued, nothing waited for
static int enqueue_scatter(ws_map *m, const int32_t *xyz_dev, size_t n, const int32_t scanner_pos[3], const int32_t up[3], bool fused, bool s0, uint32_t *seq_out)
{
  ws_context *ctx = m->ctx;
  hipStream_t s = ctx->stream;
  // the (tile, entry) hash keeps the keys of released tiles: empty it before it fills up
  if (m->status.as<uint32_t>()[10] > m->big_slots / 4) m->prepped = false;
  ScatterArgs sa;
  sa.xyz = xyz_dev;
  // (a scan, or a piece of one, that already lies in the map's own buffer is not copied there)
  sa.xyz_keep = (xyz_dev >= m->scan_dev.as<int32_t>() && xyz_dev < m->scan_dev.as<int32_t>() + 3 * MAX_SCAN_POINTS) ? nullptr : m->scan_dev.as<int32_t>();
  sa.n = (uint32_t)n;
  for (int k = 0; k < 3; ++k)
  {
    sa.scanner_pos[k] = scanner_pos[k];
    sa.up[k] = up[k];
  }
  sa.map = m->par[WS_MAP_NEW];
  sa.tau = m->tau;
  sa.res = m->res;
  sa.ntx = m->ntx;
  sa.nty = m->nty;
  sa.ntz = m->ntz;
  sa.all_keyed = s0 ? 1 : 0;
  {
    // Negative-weight (off-ray) candidates only exist where iter_steps >= 2, i.e. delta_z*2 >= res
    // (update_tsdf.cu:101-102): len >= ceil(ceil(res/2) * 32768 / 100).
    const int64_t dz_min = (m->res + 1) / 2;
    const int64_t len_neg = (dz_min * MATRIX_RESOLUTION + DZ_PER_DISTANCE - 1) / DZ_PER_DISTANCE;
    sa.keyed_len_neg = (int32_t)(len_neg > INT32_MAX ? INT32_MAX : len_neg);
    sa.keyed_slack = (int32_t)(2 * (dz_min + 1) + 3 * (int64_t)m->res + 4);
  }
  sa.rays = m->rays.as<RaySetup>();
  sa.az_hist = m->az_hist.as<uint32_t>();
  sa.az_off = m->az_off.as<uint32_t>();
  sa.ray_bin = m->ray_bin.as<uint2>();
  sa.ray_order = m->ray_order.as<uint32_t>();
  sa.fan_steps = m->fan_steps.as<int32_t>();
  sa.vstate = m->vstate.as<uint8_t>();
  sa.tile_dirty = m->tile_dirty.as<uint8_t>();
  sa.tile_nsub = m->tile_nsub.as<uint32_t>();
  sa.tile_ent = m->tile_ent.as<uint32_t>();
  sa.tile_list = m->tile_list.as<TileEntry>();
  sa.rec = m->rec.as<unsigned long long>();
  sa.sub_cap = m->sub_cap;
  sa.scan_seq = ++m->scan_seq;
  sa.big_keys = m->big_keys.as<unsigned long long>();
  sa.big_mask = m->big_slots - 1;
  {
    const RecFormat rf = rec_format(n);
    sa.rec_fmt = (uint32_t)rf.S | ((uint32_t)rf.F << 8);
  }
  sa.tail_stats = m->block_stats.as<uint32_t>();
  sa.counters = m->counters.as<TsdfCounters>();
  sa.status = m->status.dev_as<uint32_t>();

  const bool fuse = fused && !s0;
  prof_begin(ctx, WS_K_SETUP);
  // normally the kernels of the previous update have left their scratch zero / empty on their way (m->prepped)
  if (!m->prepped) enqueue_scatter_prep(m, s);
  m->prepped = false;
  launch_ray_setup(sa, s);
  prof_end(ctx, WS_K_SETUP);
  // 32-bit offsets into the voxel bytes and the record pool where both are below 4 GB (vox_ptr / rec_ptr)
  const bool small = 2ull * vstate_plane_bytes(m->n_tiles) < (1ull << 32) && (uint64_t)m->sub_cap * (SUB_RECS * 8ull) < (1ull << 32);
  prof_begin(ctx, WS_K_MARCH_TAILS);
  launch_march_tail(m, sa, small, s);
  prof_end(ctx, WS_K_MARCH_TAILS);
  if (!s0)
  {
    prof_begin(ctx, WS_K_MARCH_FREE);
    launch_march_free(sa, small, s);
    prof_end(ctx, WS_K_MARCH_FREE);
  }
  prof_begin(ctx, WS_K_TILE_RESOLVE);
  launch_tile_resolve(m, sa, s0, fuse, s);
  prof_end(ctx, WS_K_TILE_RESOLVE);
  m->fused_done = fuse;
  m->prepped = true; // every kernel above has put back what it consumed
  *seq_out = sa.scan_seq;
  WS_HIP(hipGetLastError());
  return WS_OK;
}

// The pool of sub-chunks is sized by estimate (subs_needed): a scan that exhausts it raises the abort flag, the resolve --
// which is enqueued already -- then only puts the scratch back and writes nothing to the maps, and the scan is repeated with
// a larger pool: never an inexact map.  The verdict is in host-mapped memory when the resolve starts, ~0.35 ms after the
// launches (the flag, then the sequence number).  Round 4 waited for it inside ws_tsdf_update*; now the update returns after
// the launches -- like the reference's (update_tsdf.cu:165) -- and whoever takes the map next looks first: ws_register_cloud,
// ws_reg_iterate, ws_sync, the downloads, the next update.  By then the word is there; an aborted scan is repeated from the
// arguments kept in ws_map::pending before the caller's own work is enqueued.  (Paced at the sensor's 10 Hz the round-4 wait
// cost the callback 1.3 ms of its 3.5: the GPU runs the marches at idle clocks there.)
int settle_tsdf(ws_map *m)
{
  if (!m || !m->pending.active.load(std::memory_order_acquire)) return WS_OK; // (the fast path: no lock)
  // Two readers of the reference's caller can get here at once (register_cloud and the shift thread's to_host, both under
  // the SHARED lock): one of them settles the scan, the other waits here until the map is whole.
  std::lock_guard<std::mutex> lock(m->settle_mu);
  if (!m->pending.active.load(std::memory_order_acquire)) return WS_OK;
  ws_context *ctx = m->ctx;
  hipStream_t s = ctx->stream;
  volatile uint32_t *st = m->status.as<uint32_t>();
  auto done = [&](int rc) {
    m->pending.active.store(false, std::memory_order_release);
    return rc;
  };
  // the verdict of the scatter numbered `seq`: 0 fine, bit 0 pool exhausted, bit 1 a ray beyond the key range; < 0: error
  auto verdict = [&](uint32_t seq) -> int {
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t spins = 0;
    while (st[8] != seq)
    {
      if ((++spins & 0xfffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50))
      {
        WS_HIP(hipStreamSynchronize(s)); // (a stream busy with much earlier work; the word is there afterwards)
        if (st[8] != seq)
        {
          set_error("TSDF update: the resolve did not report the end of the marches");
          return WS_ERR_INTERNAL;
        }
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return (int)st[9];
  };
  // a larger pool for a scan of n points that has just been aborted for lack of one
  auto grow_pool = [&](size_t n) -> int {
    const unsigned long long need = *reinterpret_cast<volatile unsigned long long *>(m->status.as<uint32_t>() + 4) & ((1ull << 48) - 1ull);
    uint64_t grow_to = subs_for_scan(m, need, n);
    if (grow_to < (uint64_t)m->sub_cap * 2) grow_to = (uint64_t)m->sub_cap * 2;
    if (grow_to > SUB_ID_LIMIT)
    {
      set_error("TSDF update: the scan needs more than 2^27 record sub-chunks");
      return WS_ERR_CAPACITY;
    }
    // (waits for the stream: the aborted update has drained and put its scratch back; leaves prepped == false: the new hash is
    // filled by the preparation pass, the tile tables are zero already)
    return resize_records(m, grow_to);
  };
  for (;;)
  {
    const int v = verdict(m->pending.seq);
    if (v < 0) return done(v);
    if (v == 0) return done(WS_OK); // the normal case
    if (v & 2)
    {
      // A ray with more steps / a wider fan than the record's key holds for a scan of this many points (until
      // round 6 such a ray was dropped with WS_ERR_RANGE; the reference marches it, update_tsdf.cu:67,107).  The scan is repeated
      // in pieces of 16 384 points -- their records carry the widest split, 65 536 steps and 255 fan steps -- one after the
      // other into new_map: the first piece as the scan itself would have gone, every further one on top of what new_map holds
      // (the non-default route: the fold starts from the stored entry), which is the serial schedule of the whole scan.  Then
      // the integrate over the whole map.  Slow (every candidate of the later pieces is a record, the integrate is dense) and
      // exact; beyond 65 536 steps / 255 fan steps WS_ERR_RANGE remains.
      constexpr size_t PIECE = 16384;
      bool s0 = m->pending.s0;
      for (size_t off = 0; off < m->pending.n; off += PIECE)
      {
        const size_t cnt = std::min(PIECE, m->pending.n - off);
        for (int attempt = 0;; ++attempt)
        {
          uint32_t seq = 0;
          int rc = enqueue_scatter(m, m->scan_dev.as<int32_t>() + 3 * off, cnt, m->pending.pos, m->pending.up, false, s0, &seq);
          if (rc != WS_OK) return done(rc);
          const int pv = verdict(seq);
          if (pv < 0) return done(pv);
          if (pv == 0) break;
          if ((pv & 2) || attempt >= 8)
          {
            set_error("TSDF update: a piece of the scan could not be placed");
            return done(WS_ERR_INTERNAL);
          }
          rc = grow_pool(cnt);
          if (rc != WS_OK) return done(rc);
        }
        m->new_is_default = false; // new_map carries the pieces so far
        s0 = true;
      }
      if (m->pending.integrate_after)
      {
        const int rc = launch_tsdf_integrate(m);
        if (rc != WS_OK) return done(rc);
      }
      return done(WS_OK);
    }
    if (++m->pending.attempts > 8)
    {
      set_error("TSDF update: the scan did not fit the record pool it had just been given");
      return done(WS_ERR_INTERNAL);
    }
    // The repeat reads the copy of the scan the set-up pass of the aborted attempt has left in scan_dev, and takes the route
    // (default / non-default new_map) of the first attempt.
    int rc = grow_pool(m->pending.n);
    if (rc == WS_OK) rc = enqueue_scatter(m, m->scan_dev.as<int32_t>(), m->pending.n, m->pending.pos, m->pending.up, m->pending.fused, m->pending.s0, &m->pending.seq);
    if (rc == WS_OK && m->pending.integrate_after) rc = launch_tsdf_integrate(m);
    if (rc != WS_OK) return done(rc);
  }
}

int launch_tsdf_scatter(ws_map *m, const int32_t *xyz_dev, size_t n, const int32_t scanner_pos[3], const int32_t up[3], bool fused)
{
  // (one scan in flight per map: its pool and its verdict words are the map's)
  int rc = settle_tsdf(m);
  if (rc != WS_OK) return rc;
  ws_context *ctx = m->ctx;
  hipStream_t s = ctx->stream;
  m->fused_done = false;
  m->tail_blocks = 0;
  if (n == 0)
  {
    m->resolve_blocks = 0;
    // nothing listed: a following integrate pass has nothing to do
    WS_HIP(hipMemsetAsync(&m->counters.as<TsdfCounters>()->n_listed, 0, sizeof(uint32_t), s));
    WS_HIP(hipMemsetAsync(&m->counters.as<TsdfCounters>()->n_appended, 0, sizeof(uint32_t), s));
    return WS_OK;
  }
  uint32_t seq = 0;
  const bool s0 = !m->new_is_default;
  rc = enqueue_scatter(m, xyz_dev, n, scanner_pos, up, fused, s0, &seq);
  if (rc != WS_OK) return rc;
  m->pending.seq = seq;
  m->pending.n = n;
  m->pending.s0 = s0;
  for (int k = 0; k < 3; ++k)
  {
    m->pending.pos[k] = scanner_pos[k];
    m->pending.up[k] = up[k];
  }
  m->pending.fused = fused;
  m->pending.integrate_after = false;
  m->pending.attempts = 0;
  m->pending.active.store(true, std::memory_order_release);
  // A scan into a NON-default new_map (the first update after a map came from the host, update_tsdf.cu:135-136) is settled here:
  // the dense integrate that follows consumes new_map's stored entries, and must not run on the leftovers of an aborted scan.
  if (!m->new_is_default) return settle_tsdf(m);
  return WS_OK;
}

} // namespace ws
