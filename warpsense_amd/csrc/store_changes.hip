// store_changes.hip — the passes of ws_store_changes (include/warpsense_hip.h; the rules are in ws_changes.h, the host flow in
// api_store_pair.hip): the voxels of the store CUR whose class differs from that of the store REF sampled at their place under a rigid pull
// transform, as ordered records.  The ordered stream compaction is that of store_frontier.hip in the word space of ws_store_words.h;
// the transform and the sample are the fuse's (ws_fuse.h).
//
//   store_changes_count_kernel    chunk order, one wave per four chunk columns of CUR, lane = z: a coalesced 256-byte load of the
//                                 column, the x and y terms of the transform once per column from wave-uniform values, REF gathered
//                                 through StoreField::lookup by the lanes whose CUR entry is known.  The ballot of "record" is the
//                                 word's mask at t; the statistics are summed in the wave, then across the four waves through LDS:
//                                 one atomic per workgroup and counter
//   store_changes_totals_kernel   word order: the masks' popcounts per 256 consecutive words
//   store_changes_scan_kernel     exclusive scan of those totals (one workgroup; 64-bit offsets, the last element is the total)
//   store_changes_emit_kernel     word order, 256 consecutive words per workgroup: a lane of a set bit samples again for the value and
//                                 the kind and writes its record to (workgroup base + words before + set bits below the lane)
//
// Plain launches on the context's stream, nothing waits for another workgroup; the only atomics are the integer adds of the statistics.
// The clustering of the records is frontier_clusters (map_frontier.hip).
#include "ws_changes.h"
#include "ws_mesh.h" // block_scan_256, popc_below

namespace ws
{
// p - pivot_dst on one axis for the world voxel v of CUR; false: outside the reach
__device__ __forceinline__ bool ch_delta(const ChangesArgs &a, int axis, int32_t v, int32_t &d)
{
  const int64_t d64 = (int64_t)v * a.res + a.half - (int64_t)a.pd[axis];
  d = (int32_t)d64;
  return d64 > -FUSE_REACH && d64 < FUSE_REACH;
}

// the x and y terms of the three sums of the transform, with the 2^29: uniform over a column
__device__ __forceinline__ void ch_column(const ChangesArgs &a, int32_t dx, int32_t dy, int64_t base[3])
{
#pragma unroll
  for (int k = 0; k < 3; ++k) base[k] = (int64_t)a.rot[3 * k] * dx + (int64_t)a.rot[3 * k + 1] * dy + (1ll << 29);
}

// the cell of REF at q for a voxel inside the reach: base voxel b, fractions f; false: q is dead
__device__ __forceinline__ bool ch_cell(const ChangesArgs &a, const int64_t base[3], int32_t dz, int32_t b[3], int32_t f[3])
{
  bool live = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    const int64_t q = fuse_pull(base[k], a.rot[3 * k + 2], dz, a.ps[k]);
    live = live && !fuse_dead(q);
    b[k] = floor_div(live ? (int32_t)q - a.half : 0, a.rdiv, f[k]);
  }
  return live;
}

__device__ __forceinline__ uint32_t ch_wave_sum(uint32_t v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- pass 1: the chunks of CUR, once.  A workgroup takes 16 columns of one x plane of a chunk, a wave four of them (the shape of
// store_frontier_count_kernel)
__global__ __launch_bounds__(256) void store_changes_count_kernel(ChangesArgs a)
{
  __shared__ uint32_t sS[4][CH_STATS_DEV];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t i = blockIdx.x >> 8, lx = (blockIdx.x >> 2) & 63u, ly0 = (blockIdx.x & 3u) * 16u + (uint32_t)wave * 4u;
  if (i >= a.n_chunks) return; // (uniform over the workgroup)
  const su32x4 g = a.grp[i];
  const mi32x4 k = a.key[i];
  const uint32_t *column = sm_chunk(a, i) + (lx * (uint32_t)(STORE_CS * STORE_CS) + ly0 * (uint32_t)STORE_CS);
  const int32_t x = k.x * STORE_CS + (int32_t)lx, y0 = k.y * STORE_CS + (int32_t)ly0, z = k.z * STORE_CS + lane;
  int32_t dx, dz;
  const bool in_x = x >= a.lo[0] && x <= a.hi[0] && ch_delta(a, 0, x, dx);
  const bool in_z = z >= a.lo[2] && z <= a.hi[2] && ch_delta(a, 2, z, dz);
  const uint32_t t0 = sm_word(g, i, lx, ly0);
  StoreRayArgs sa; // (only what lookup() reads)
  sa.table = a.ref_table, sa.mask = a.ref_mask, sa.segs = a.ref_segs, sa.seg_shift = a.ref_shift;
  StoreField fld(sa);

  uint32_t n_both = 0, n_app = 0, n_van = 0, n_new = 0, s_diff = 0; // per lane: at most 4 voxels
#pragma unroll 1
  for (int j = 0; j < 4; ++j)
  {
    const int32_t y = y0 + j;
    int32_t dy;
    const bool in_y = y >= a.lo[1] && y <= a.hi[1] && ch_delta(a, 1, y, dy); // (uniform)
    uint32_t raw = 0u; // outside the box or the reach: weight 0, not known
    if (in_x && in_y && in_z) raw = __builtin_nontemporal_load(column + j * STORE_CS + lane);
    const int32_t ev = entry_value(raw), ew = entry_weight(raw);
    const bool known = ew >= a.rule.min_weight;
    bool rec = false;
    if (__ballot(known) != 0ull)
    {
      int64_t base[3];
      ch_column(a, dx, dy, base);
      int32_t b[3], f[3];
      // the corner (0, 0, 0) always takes part: without its chunk there is no valid sample
      bool live = known && ch_cell(a, base, dz, b, f);
      live = live && fuse_src_chunk(fld, b[0] >> 6, b[1] >> 6, b[2] >> 6) != nullptr;
      int32_t nv = 0, nw = 0;
      bool valid = false;
      if (__ballot(live) != 0ull) valid = live && fuse_sample(a, fld, b, f, nv, nw);
      uint32_t diff;
      const uint32_t v = changes_verdict(ev, ew, valid, nv, nw, a.rule, diff);
      const uint32_t kind = v & 3u;
      n_both += (v & CH_BOTH) ? 1u : 0u;
      n_new += (v & CH_NEW) ? 1u : 0u;
      n_app += kind == CH_APPEARED ? 1u : 0u;
      n_van += kind == CH_VANISHED ? 1u : 0u;
      s_diff += diff;
      rec = kind != 0u && ((a.kinds >> (kind - 1u)) & 1u) != 0u;
    }
    const mu64 m = __ballot(rec);
    if (lane == j) a.mask[t0 + (uint32_t)j * g.w] = m;
  }

  // integer adds: exact whatever the order
  n_both = ch_wave_sum(n_both), n_app = ch_wave_sum(n_app), n_van = ch_wave_sum(n_van), n_new = ch_wave_sum(n_new), s_diff = ch_wave_sum(s_diff);
  if (lane == 0) sS[wave][0] = n_both, sS[wave][1] = n_app, sS[wave][2] = n_van, sS[wave][3] = n_new, sS[wave][4] = s_diff;
  __syncthreads();
  if (threadIdx.x < CH_STATS_DEV)
  {
    const uint32_t c = sS[0][threadIdx.x] + sS[1][threadIdx.x] + sS[2][threadIdx.x] + sS[3][threadIdx.x]; // < 2^27
    if (c) atomicAdd(a.stats + threadIdx.x, (unsigned long long)c);
  }
}

// ---- pass 1b: records per workgroup of the emit pass (n_words is a multiple of 4096: every thread has a word)
__global__ __launch_bounds__(256) void store_changes_totals_kernel(ChangesArgs a)
{
  uint32_t c = (uint32_t)__popcll(a.mask[blockIdx.x * CH_WORDS + threadIdx.x]);
  c = ch_wave_sum(c);
  __shared__ uint32_t wtot[4];
  if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) a.blk_tot[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

// ---- pass 2
__global__ __launch_bounds__(1024) void store_changes_scan_kernel(const uint32_t *tot, mu64 *off, uint32_t n, mu64 *total)
{
  scan_block_totals(tot, off, n, total);
}

// ---- pass 3: the records, in word order
__global__ __launch_bounds__(256) void store_changes_emit_kernel(ChangesArgs a)
{
  __shared__ mu64 sM[CH_WORDS];
  __shared__ uint32_t sB[CH_WORDS];
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * CH_WORDS;
  const mu64 Mt = a.mask[t0 + threadIdx.x];
  sM[threadIdx.x] = Mt;
  sB[threadIdx.x] = block_scan_256((uint32_t)__popcll(Mt), wsum);
  __syncthreads();
  const mu64 base_o = a.blk_off[blockIdx.x];
  StoreRayArgs sa; // (only what lookup() reads)
  sa.table = a.ref_table, sa.mask = a.ref_mask, sa.segs = a.ref_segs, sa.seg_shift = a.ref_shift;
  StoreField fld(sa);
  for (int w = 0; w < 64; ++w) // the wave's 64 words, one after the other; lane = z inside the word
  {
    const int idx = wave * 64 + w;
    const mu64 M = sM[idx];
    if (M == 0ull) continue; // (most words hold no change; the same for the whole wave)
    StoreWord p;
    p.find(a, t0 + (uint32_t)idx);
    if (!((M >> lane) & 1ull)) continue;
    const mu64 o = base_o + sB[idx] + popc_below(M, lane);
    if (o >= a.cap) continue; // (the count pass sized the buffer; a store that changed in between must not write beyond it)
    const mi32x4 k = a.key[p.i];
    const int32_t x = k.x * STORE_CS + (int32_t)p.lx, y = k.y * STORE_CS + (int32_t)p.ly, z = k.z * STORE_CS + lane;
    const uint32_t raw = sm_chunk(a, p.i)[p.lx * (uint32_t)(STORE_CS * STORE_CS) + p.ly * (uint32_t)STORE_CS + (uint32_t)lane];
    // the voxel of a set bit lies in the box and within the reach: the three differences fit
    int32_t dx, dy, dz, b[3], f[3], nv = 0, nw = 0;
    bool live = ch_delta(a, 0, x, dx);
    live = ch_delta(a, 1, y, dy) && live;
    live = ch_delta(a, 2, z, dz) && live;
    int64_t base[3];
    ch_column(a, dx, dy, base);
    live = live && ch_cell(a, base, dz, b, f);
    const bool valid = live && fuse_sample(a, fld, b, f, nv, nw);
    uint32_t diff;
    const uint32_t v = changes_verdict(entry_value(raw), entry_weight(raw), valid, nv, nw, a.rule, diff);
    const su32x4 r = {(uint32_t)x, (uint32_t)y, (uint32_t)z, changes_word(nv, v & 3u)};
    a.rec[o] = r;
  }
}

// ---- host side: the workgroups of the emit pass are those of the surface cloud (store_surface_blocks)
static ChangesArgs store_ch_args(const ws_store *cur, const ws_store *ref, const ws_store::Changes &q, const StoreChangesCall &c, size_t cap)
{
  ChangesArgs a;
  store_words_bind(a, cur, static_cast<const char *>(q.table_dev.p), c.n_chunks);
  for (int k = 0; k < 9; ++k) a.rot[k] = c.pull.rot_q30[k];
  for (int k = 0; k < 3; ++k) a.pd[k] = c.pull.pivot_dst_mm[k], a.ps[k] = c.pull.pivot_src_mm[k], a.lo[k] = c.lo[k], a.hi[k] = c.hi[k];
  a.res = c.res, a.half = c.res / 2;
  a.rdiv = make_fastdiv(c.res);
  a.res3 = (int64_t)c.res * c.res * c.res;
  a.tdiv = make_fuse_div(a.res3);
  a.rule.band = c.band, a.rule.free_value = c.free_value, a.rule.min_weight = c.min_weight;
  a.kinds = c.kinds;
  a.ref_table = static_cast<const StoreRaySlot *>(c.ref_table_dev);
  a.ref_mask = (uint32_t)c.ref_places - 1u;
  a.ref_segs = ref->seg_tab.as<uint32_t *>(), a.ref_shift = ref->seg_shift;
  a.mask = static_cast<mu64 *>(q.mask.p);
  a.blk_tot = static_cast<uint32_t *>(q.blk_tot.p);
  a.blk_off = static_cast<const mu64 *>(q.blk_off.p);
  a.rec = static_cast<su32x4 *>(q.rec.p);
  a.cap = cap;
  a.stats = q.stats.dev;
  return a;
}

// the upload of CUR's tables, then passes 1 and 2 (the caller has enqueued the upload of REF's lookup); the total arrives in
// q.total.host and the sums in q.stats.host (pinned) once the stream has been synchronised
int launch_store_changes_count(ws_store *cur, const ws_store *ref, ws_store::Changes &q, const StoreChangesCall &c)
{
  hipStream_t s = cur->ctx->stream;
  WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_word_table_bytes(c.n_chunks), hipMemcpyHostToDevice, s));
  WS_HIP(hipMemsetAsync(q.stats.dev, 0, CH_STATS_DEV * sizeof(unsigned long long), s));
  const ChangesArgs a = store_ch_args(cur, ref, q, c, 0);
  const uint32_t blocks = c.n_chunks * (4096u / CH_WORDS);
  hipLaunchKernelGGL(store_changes_count_kernel, dim3(c.n_chunks * 256u), dim3(256), 0, s, a);
  hipLaunchKernelGGL(store_changes_totals_kernel, dim3(blocks), dim3(256), 0, s, a);
  q.timer.mark(1, s);
  hipLaunchKernelGGL(store_changes_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)a.blk_tot, static_cast<mu64 *>(q.blk_off.p), blocks, q.total.dev);
  q.timer.mark(2, s);
  WS_HIP(hipGetLastError());
  WS_TRY(q.stats.fetch(s, CH_STATS_DEV));
  return q.total.fetch(s);
}

// pass 3: no record at or beyond `cap` is written
int launch_store_changes_emit(ws_store *cur, const ws_store *ref, ws_store::Changes &q, const StoreChangesCall &c, size_t cap)
{
  const ChangesArgs a = store_ch_args(cur, ref, q, c, cap);
  hipStream_t s = cur->ctx->stream;
  q.timer.mark(3, s);
  hipLaunchKernelGGL(store_changes_emit_kernel, dim3(c.n_chunks * (4096u / CH_WORDS)), dim3(256), 0, s, a);
  q.timer.mark(4, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
