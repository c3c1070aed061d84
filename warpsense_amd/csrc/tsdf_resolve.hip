// tsdf_resolve.hip — the resolve of the TSDF scatter (gfx950): exact resolve of one tile in LDS, a workgroup per touched tile.
// (Survey: tsdf_update.hip.)  Of the marches' side it needs the addressing of tsdf_scatter.h only, not the pool.
#include "tsdf_scatter.h"

namespace ws
{
struct ResolveArgs
{
  TileEntry *tile_list; // the tiles with records; the resolve appends the others it finds when a separate integrate pass follows
  uint32_t *tile_nsub;
  const uint32_t *tile_ent;
  uint8_t *tile_dirty;
  const unsigned long long *recs;
  unsigned long long *big_keys;
  uint32_t big_mask;
  uint32_t scan_seq;
  uint32_t sub_cap;
  uint32_t fan_mask, fan_mid; // the fan field of this scan's records (rec_format): the weight is negated iff fan != fan_mid
  uint32_t *new_data;
  uint32_t *avg_data;
  uint8_t *vstate;
  MapParams map;
  int32_t nty, ntz;
  int32_t tau, max_weight;
  uint32_t wM32;     // division by tau - tau/10 of the weight ramp (update_tsdf.cu:92) as one v_mul_hi_u32 + shift
  int32_t wS;
  uint32_t *resolve_stats; // [grid][2]: contested voxels, tiles with records
  TsdfCounters *counters;
  uint32_t *status;
  int64_t n_tiles;
};
static_assert(sizeof(ResolveArgs) <= 256, "ResolveArgs: more than 256 bytes of kernel arguments");

#ifndef WS_RESOLVE_KO
#define WS_RESOLVE_KO 0 // knock-out builds for timing (results wrong): 1 no scan A, 2 no LDS atomics in pass 1, 4 no records at all (fill = 0)
#endif
#ifndef WS_RESOLVE_GRID
#define WS_RESOLVE_GRID 1280 // 256 compute units x five resident workgroups: every workgroup is on the chip from the start (1280 / 2560 / 4096: 124 / 129 / 130 us)
#endif
constexpr int RESOLVE_GRID = WS_RESOLVE_GRID; // (block_stats holds two words per workgroup, 4096 at most)
static_assert(RESOLVE_GRID <= 4096, "resolve_stats");
constexpr uint32_t M_IDLE = 0xffffffffu, M_NONE = 0x10000u; // mstate: voxel not in the ordered rounds / no earlier negative seen
constexpr unsigned long long REC_NONE = ~0ull;

// kneg: smallest |value| wins, the LATEST candidate among equal |value| (a later equal one replaces the entry)
__device__ __forceinline__ uint64_t neg_key(uint64_t rec, int32_t av, int32_t value)
{
  const uint64_t t = rec >> REC_T_SHIFT;
  return ((uint64_t)av << 39) | ((T_MASK - t) << 1) | (value < 0 ? 1u : 0u);
}
__device__ __forceinline__ int32_t neg_key_abs(uint64_t N) { return (int32_t)(N >> 39); }

constexpr uint32_t ENT_NONE = 0xffffffffu;
// entry number j >= TILE_DIRECT of a tile: through the hash (the marches are over: everything is published)
__device__ __forceinline__ uint32_t resolve_entry(const ResolveArgs &a, uint32_t tile, uint32_t j)
{
  const unsigned long long key = big_key(tile, j);
  const uint32_t *vals = reinterpret_cast<const uint32_t *>(a.big_keys + (size_t)a.big_mask + 1);
  uint32_t h = big_slot(key, a.big_mask);
  for (uint32_t probe = 0; probe <= a.big_mask; ++probe)
  {
    const unsigned long long cur = a.big_keys[h];
    if (cur == key) return vals[h] - 1u; // (0: released -> ENT_NONE)
    if (cur == KEY_INF) break;
    h = (h + 1) & a.big_mask;
  }
  return ENT_NONE;
}

// every record of a tile, from memory: tiles of more than 8 * RES_MAXR sub-chunks, and the ordered rounds.  64 entries at a
// time -- lane l of every wave holds entry l of the batch: the first from the prefetched `cid`, the second from the tile's
// table, further ones through the hash, every lane looking up its own -- and of those WS_STREAM_U sub-chunks per half-wave in
// flight together (one after the other, each load waited for on the spot, this route took as long again as the whole fold).
#ifndef WS_STREAM_U
#define WS_STREAM_U 2 // (four: ten spilled registers in the fused resolve, 141 instead of 132 us)
#endif
template <class F>
__device__ __forceinline__ void for_each_record(const ResolveArgs &a, uint32_t tile, uint32_t nsub, uint32_t cid, uint32_t first, F &&f)
{
  const int lane = threadIdx.x & 63;
  const uint32_t half = threadIdx.x >> 5, pos = threadIdx.x & 31u;
  constexpr int U = WS_STREAM_U;
  // (first: a multiple of 8 below or at 64 -- the entries in front of it are in the caller's registers; a batch stays inside one block of
  // 64 entries: lane l of every wave holds entry 64 (b0 / 64) + l)
  for (uint32_t b0 = first; b0 < nsub; b0 = (b0 & ~63u) + 64u)
  {
    const uint32_t blk0 = b0 & ~63u, in0 = b0 & 63u;
    uint32_t ents = cid;
    if (blk0 == 64)
      ents = a.tile_ent[(size_t)tile * TILE_DIRECT + 64u + (uint32_t)lane];
    else if (blk0 > 64)
      ents = blk0 + (uint32_t)lane < nsub ? resolve_entry(a, tile, blk0 + (uint32_t)lane) : ENT_NONE;
    const uint32_t nb = min(64u, nsub - blk0); // entries of this block
    for (uint32_t j0 = in0; j0 < nb; j0 += 8u * U)
    {
      unsigned long long rec[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
      {
        const uint32_t j = j0 + 8u * (uint32_t)u + half;
        const uint32_t ent = (uint32_t)__shfl((int)ents, (int)(j & 63u), 64);
        ok[u] = j < nb && ent != ENT_NONE && pos <= (ent & 31u) && (ent >> SUB_BITS) < a.sub_cap;
        rec[u] = a.recs[ok[u] ? ((size_t)(ent >> SUB_BITS) << SUB_BITS) + pos : (size_t)threadIdx.x];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u])
        {
          const int32_t value = rec_value(rec[u]);
          f((uint64_t)rec[u], value, value < 0 ? -value : value, (int)rec_local(rec[u]));
        }
    }
  }
}

#ifndef WS_RES_MAXR
#define WS_RES_MAXR 8
#endif
#ifndef WS_RESOLVE_WGS
#define WS_RESOLVE_WGS 5 // (107 -> 102 VGPRs without spills, 29 KB of LDS: 4 -> 5 workgroups per CU, 139 -> 130 us)
#endif
constexpr int RES_MAXR = WS_RES_MAXR;   // records a thread keeps in registers (2048 record places = 64 sub-chunks per tile); larger tiles re-read them per pass
static_assert(RES_MAXR >= 1 && RES_MAXR * 8 <= 64 && TILE_DIRECT == 128, "the register route reads the first 8 RES_MAXR <= 64 entries of the tile's direct table, the streaming route the rest");
// (RES_MAXR 4 / 5 / 6 / 7 / 8, same box: the resolve 108-110 / 108 / 105-106 / 104-105 / 102-103 us -- fewer registers buy no sixth
// workgroup per CU, 28 KB of LDS and the other ~80 registers cap it at five, and the sub-chunks beyond the registers are streamed per pass)

// what a thread needs of a tile before it can start, requested two tiles ahead
struct TilePre
{
  int64_t idx0;
  int nz;
  uint32_t fill; // sub-chunks (entries) of the tile (uniform)
  uint32_t cid;  // lane l of every wave: entry l of the tile
  uint32_t vs;   // four vstate bytes (both planes)
  uint32_t s0[4]; // new_map entries (HAS_S0)
};
// the result of a tile, written back one tile later (behind the next tile's wait for its records)
struct TilePost
{
  int64_t idx0;
  int nz;
  uint32_t tile;
  uint32_t vs;
  uint32_t touched; // bit j
  uint32_t value[4];
  uint32_t existing[4];
};

// One workgroup per touched tile, thread t owns the voxels 4t .. 4t+3 of the tile (one column, four consecutive z).
// HAS_S0: new_map is not (tau, 0) — the fold starts from the stored entry (a positive weight there freezes the voxel).
// FUSED: integrate the result straight into avg_map instead of writing new_map (new_map stays (tau, 0)).
//
// Per voxel, with the candidates in canonical order: the winner is the first positive-weight candidate p with
// |v_p| <= min |v_n| over the negative-weight candidates n BEFORE p (atomic_tsdf_min accepts iff the stored weight is
// <= 0 and |new| <= |stored|, cuda/util.h:70-102); if there is none, the negative candidate of smallest |value|
// (latest on ties); else the entry stays.  LDS phases per tile:
//   pass 1   kpos = earliest positive, kneg = smallest (latest) negative            (LDS atomicMin per record)
//   scan A   m = min |v_n| over the negatives before kpos with |v_n| < |v_kpos|      (only those can block it)
//   decide   no such negative -> kpos wins; no positive -> kneg; else kpos is blocked: later positives need |v| <= m
//   scan B / decide / scan A ...  the next eligible positive, until every voxel is decided (rare after the first round)
//
// Memory pipeline.  gfx950 retires vector memory operations in order behind ONE counter (loads and stores), and the
// counts here are data dependent, so every wait is a wait for everything outstanding.  The loop therefore has a single
// such point per tile — the arrival of the tile's records — and everything else is arranged around it: entry, voxel
// bytes and entry table of later tiles and the records of the next tile are all requested together at the END of an
// iteration, and the stores of a tile are issued right AFTER the next wait, so they drain under the LDS phases.
//
// A scan that ran out of sub-chunks (counters->abort) leaves no trace: the tiles' scratch is put back as always, nothing is
// written to the maps, and the host runs the scan again with a larger buffer.
template <bool HAS_S0, bool FUSED>
__global__ __launch_bounds__(256, WS_RESOLVE_WGS) void tile_resolve_kernel(ResolveArgs a)
{
  __shared__ unsigned long long kpos[TILE_VOXELS];
  __shared__ unsigned long long kneg[TILE_VOXELS];
  __shared__ unsigned long long klast[TILE_VOXELS]; // the positive candidate that was blocked last
  __shared__ uint32_t mstate[TILE_VOXELS];          // M_IDLE: decided; else min |value| of the blocking negatives (M_NONE: none)
  __shared__ uint16_t bound0[HAS_S0 ? TILE_VOXELS : 1]; // |stored value| + 1 (0: frozen)
  __shared__ uint32_t s_unres[2];
#ifdef WS_RESOLVE_TIMING
  const long long t_begin = wall_clock64();
#endif
  const uint32_t n_list = a.counters->n_listed; // the tiles with records
  const bool aborted = a.counters->abort != 0 || a.counters->range_seq == a.scan_seq;
  const int32_t weight_epsilon = a.tau / 10;
  const uint32_t reset = pack_entry(a.tau, 0);
  const int lane = threadIdx.x & 63;
  uint8_t *const vneg = a.vstate + vstate_plane_bytes(a.n_tiles);
  // thread t owns the voxels 4t .. 4t+3 of the tile: column t >> (ZB - 2), four consecutive z
  const int col = threadIdx.x >> (TILE_ZB - 2), lx = col >> TILE_YB, ly = col & ((1 << TILE_YB) - 1), z0 = (threadIdx.x & ((1 << (TILE_ZB - 2)) - 1)) * 4;
  const int l0 = threadIdx.x * 4;
  const uint32_t voff = vbrick((uint32_t)l0); // where the thread's four voxel bytes lie in the tile's kilobyte: one aligned word
  const uint32_t G = gridDim.x;
  uint32_t n_contested = 0;

  // all loads unconditional (clamped addresses, results masked)
  auto request = [&](const TileEntry &te, TilePre &p) {
    const int32_t sx = (te.tx << TILE_XB) + lx, sy = (te.ty << TILE_YB) + ly, sz = (te.tz << TILE_ZB) + z0;
    const bool col_ok = sx < a.map.size[0] && sy < a.map.size[1];
    int nz = a.map.size[2] - sz;
    p.nz = !col_ok ? 0 : (nz > 4 ? 4 : (nz < 0 ? 0 : nz));
    p.idx0 = p.nz ? storage_index(a.map, sx, sy, sz) : 0;
    p.fill = a.tile_nsub[te.tile];
    p.cid = a.tile_ent[(size_t)te.tile * TILE_DIRECT + (uint32_t)lane];
    // four voxels of a column in one access each (the arrays carry 16 bytes of slack behind the last voxel)
    const uint32_t keep = p.nz >= 4 ? 0xffffffffu : ((1u << (8 * p.nz)) - 1u);
    p.vs = 0;
    // both byte planes of the four voxels in one register: the second plane's mark becomes bit VOX_NEGFREE of the byte
    const size_t vb = ((size_t)te.tile << 10) + voff;
    if (!HAS_S0) p.vs = (*reinterpret_cast<const uint32_t *>(a.vstate + vb) | ((*reinterpret_cast<const uint32_t *>(vneg + vb) & 0x01010101u) << 3)) & keep;
    const u32x4 z4 = {reset, reset, reset, reset};
    u32x4 s4 = z4;
    if (HAS_S0) s4 = *reinterpret_cast<const u32x4_a4 *>(a.new_data + p.idx0);
    p.s0[0] = s4.x; p.s0[1] = s4.y; p.s0[2] = s4.z; p.s0[3] = s4.w;
  };
  // weight ramp of update_tsdf.cu:90-94; 64 * (tau + value) >= 0 is below 2^31
  auto weight_of = [&](int32_t value) -> int32_t {
    int32_t w = WEIGHT_RESOLUTION;
    if (value < -weight_epsilon) w = (int32_t)(__umulhi((uint32_t)(WEIGHT_RESOLUTION * (a.tau + value)), a.wM32) >> a.wS);
    return w;
  };
  auto init_lds = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      kpos[l0 + j] = KEY_INF;
      kneg[l0 + j] = KEY_INF;
      mstate[l0 + j] = M_NONE;
    }
  };
  // The records of a tile, in registers: thread t takes place t & 31 of the tile's sub-chunks t >> 5, (t >> 5) + 8, ... -- one
  // coalesced 256-byte read per half-wave and sub-chunk, all RES_MAXR of them in flight together.  Returns false (uniform
  // over the workgroup) when the tile has more than 8 * RES_MAXR sub-chunks: the waves then stream them from memory in every
  // pass.  The loads are UNCONDITIONAL (clamped address) and all issued before the first result is touched: a load under a
  // branch, or a use right behind it, makes the compiler wait for each of them in turn.
  unsigned long long rrec[RES_MAXR]; // REC_NONE: no record
  u32x4 ex_next = {0, 0, 0, 0}; // FUSED: the avg_map entries of the tile whose records are in flight
  auto fetch_records = [&](const TilePre &p) -> bool {
    if (FUSED) ex_next = *reinterpret_cast<const u32x4_a4 *>(a.avg_data + p.idx0);
    const uint32_t nsub = aborted ? 0u : p.fill;
    const bool in_regs = nsub != 0; // (a tile of more than 8 * RES_MAXR sub-chunks: the first 64 here, the rest streamed)
    const uint32_t pos = threadIdx.x & 31u;
#pragma unroll
    for (int k = 0; k < RES_MAXR; ++k)
    {
      const uint32_t j = (uint32_t)(8 * k) + (threadIdx.x >> 5);
      const uint32_t ent = (uint32_t)__shfl((int)p.cid, (int)j, 64);
      const bool ok = in_regs && j < nsub && pos <= (ent & 31u) && (ent >> SUB_BITS) < a.sub_cap;
      const unsigned long long v = a.recs[ok ? ((size_t)(ent >> SUB_BITS) << SUB_BITS) + pos : (size_t)threadIdx.x];
      rrec[k] = ok ? v : REC_NONE;
    }
    return in_regs;
  };
  auto write_back = [&](const TilePost &w) {
    const size_t vb = ((size_t)w.tile << 10) + voff;
    if (w.nz == 4 && !HAS_S0) // (a non-default new_map keeps the entries of its untouched voxels: voxel by voxel below)
    {
      // the thread's four voxels as ONE access per array (byte stores are a transaction each: 14 M of them per scan were
      // most of this kernel's write traffic)
      if (w.vs & 0x07070707u) *reinterpret_cast<uint32_t *>(a.vstate + vb) = 0;
      if (w.vs & 0x08080808u) *reinterpret_cast<uint32_t *>(vneg + vb) = 0;
      if (w.touched == 0 || aborted) return;
      u32x4 out;
      if (FUSED)
      {
        out.x = (w.touched & 1u) ? integrate_entry(w.existing[0], w.value[0], a.max_weight) : w.existing[0];
        out.y = (w.touched & 2u) ? integrate_entry(w.existing[1], w.value[1], a.max_weight) : w.existing[1];
        out.z = (w.touched & 4u) ? integrate_entry(w.existing[2], w.value[2], a.max_weight) : w.existing[2];
        out.w = (w.touched & 8u) ? integrate_entry(w.existing[3], w.value[3], a.max_weight) : w.existing[3];
        if (out.x != w.existing[0] || out.y != w.existing[1] || out.z != w.existing[2] || out.w != w.existing[3])
          *reinterpret_cast<u32x4_a4 *>(a.avg_data + w.idx0) = out;
      }
      else
      {
        // (the untouched voxels of a default new_map are (tau, 0), and that is what `value` holds for them)
        out.x = w.value[0]; out.y = w.value[1]; out.z = w.value[2]; out.w = w.value[3];
        *reinterpret_cast<u32x4_a4 *>(a.new_data + w.idx0) = out;
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      if (j >= w.nz) continue;
      if (!HAS_S0 && ((w.vs >> (8 * j)) & (0xffu & ~(uint32_t)VOX_NEGFREE))) a.vstate[vb + j] = 0;
      if (!HAS_S0 && ((w.vs >> (8 * j)) & VOX_NEGFREE)) vneg[vb + j] = 0;
      if (!(w.touched & (1u << j)) || aborted) continue;
      if (FUSED)
      {
        const uint32_t updated = integrate_entry(w.existing[j], w.value[j], a.max_weight);
        if (updated != w.existing[j]) a.avg_data[w.idx0 + j] = updated;
      }
      else
      {
        a.new_data[w.idx0 + j] = w.value[j];
      }
    }
  };
  // the tile's scratch goes back to zero for the next scan (no clean-up launch): its entry count (the table itself is only
  // ever read up to the count) and the values of its entries in the hash
  auto release_tile = [&](uint32_t tile, uint32_t nsub) {
    if (threadIdx.x == 8) a.tile_nsub[tile] = 0;
    // (the scan over the flag planes below owns the "listed" bytes and clears them; a scan into a non-default new_map has no
    // such pass -- ADVICE r4: the bytes of its listed tiles stayed set and hid those tiles from the NEXT scan's flag scan)
    if (HAS_S0 && threadIdx.x == 9) a.tile_dirty[tile_flag_plane_bytes(a.n_tiles) + tile] = 0;
    if (nsub > (uint32_t)TILE_DIRECT)
    {
      uint32_t *vals = reinterpret_cast<uint32_t *>(a.big_keys + (size_t)a.big_mask + 1);
      for (uint32_t j = (uint32_t)TILE_DIRECT + threadIdx.x; j < nsub; j += 256u)
      {
        const unsigned long long key = big_key(tile, j);
        uint32_t h = big_slot(key, a.big_mask);
        for (uint32_t probe = 0; probe <= a.big_mask; ++probe)
        {
          const unsigned long long cur = a.big_keys[h];
          if (cur == key)
          {
            // (the slot keeps its key: emptying it would cut the probe chains that run through it; a key of an earlier
            // scan with value 0 is "nothing" to the resolve and is overwritten by the tile's next entry j)
            vals[h] = 0;
            break;
          }
          if (cur == KEY_INF) break;
          h = (h + 1) & a.big_mask;
        }
      }
    }
  };

  // The per-scan scratch this scan has consumed goes back to zero here, for the next scan (no clean-up launch behind the
  // update); the host learns that the marches are over and whether the scan has to be repeated.
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    TsdfCounters *c = a.counters;
    c->last_chunks = c->chunk_cursor;
    c->last_need = c->ub_total & ((1ull << 48) - 1ull);
    c->ub_total = 0;
    __hip_atomic_store(a.status + 10, c->big_inserted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const uint32_t verdict = (c->abort != 0 ? 1u : 0u) | (c->range_seq == a.scan_seq ? 2u : 0u);
    __hip_atomic_store(a.status + 9, verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); // (bit 0: pool exhausted, bit 1: key range)
    __hip_atomic_store(a.status + 8, a.scan_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // The tiles with records: the scan's tile list (the marches appended every tile at its first reservation), dealt out
  // evenly: workgroup b takes the entries b, b + G, ...
  const uint32_t e0 = blockIdx.x, e_end = n_list, ES = G;
  uint32_t n_mine = 0; // tiles this workgroup has folded
  if (e0 < e_end)
  {
  const uint32_t last = e_end - 1;
  // pipeline: tile i is processed while the voxel bytes / entry table of tiles i+1 and i+2, the list entries up to i+3
  // and (from the middle of the iteration on) the records of tile i+1 are in flight
  TileEntry te_n2 = a.tile_list[min(e0 + 2 * ES, last)], te_n3 = te_n2;
  uint32_t tile_cur, tile_n1;
  TilePre p_cur, p_n1, p_n2;
  {
    const TileEntry t0 = a.tile_list[e0], t1 = a.tile_list[min(e0 + ES, last)];
    request(t0, p_cur);
    request(t1, p_n1);
    tile_cur = t0.tile;
    tile_n1 = t1.tile;
  }
  bool cached = fetch_records(p_cur), cached_next = false;
  u32x4 ex_cur = ex_next;
  auto issue_next = [&](uint32_t e) {
    te_n3 = a.tile_list[min(e + 3 * ES, last)];
    request(te_n2, p_n2);
    cached_next = fetch_records(p_n1);
  };
  TilePost post;
  post.nz = 0;
  post.idx0 = 0;
  post.tile = 0;
  post.vs = post.touched = 0;
  if (threadIdx.x == 0) s_unres[0] = s_unres[1] = 0;
  init_lds();
  __syncthreads();

  for (uint32_t e = e0; e < e_end; e += ES)
  {
    {
      // The five workgroups of a compute unit start together with the same amount of work, and the SIMDs serve the OLDEST ready
      // wave first: the workgroups finished one after the other (65 ... 115 us, a round-5 instrumented build: the spread is inside the
      // compute units, not between them, and has nothing to do with the tiles a workgroup got), the compute unit ran its last
      // 25 us with one or two workgroups.  Now the issue priority goes round: a workgroup changes its priority with every tile,
      // the five of a compute unit (b, b + 256, ... in dispatch order) start at different places of the cycle -- spread inside a
      // compute unit 9.7 -> 4.9 us, the launch 110 -> 104 us.  (Priority by progress -- a quarter of the tiles done, one level
      // down: 105; time slices of 2.56 us on the shared clock: 106.)
      const uint32_t prio = (n_mine + blockIdx.x / 256u) & 3u;
      if (prio == 3u) __builtin_amdgcn_s_setprio(3);
      else if (prio == 2u) __builtin_amdgcn_s_setprio(2);
      else if (prio == 1u) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    n_mine += 1;
    const TilePre p = p_cur;
    const uint32_t tile = tile_cur, nsub_real = p.fill, fill = (aborted || (WS_RESOLVE_KO & 4)) ? 0u : p.fill; // (an aborted scan: the entries may be anything)
    const int nz = p.nz;
    const int64_t idx0 = p.idx0;

    uint32_t entry[4] = {reset, reset, reset, reset};
    uint32_t touched = 0;
    uint8_t vs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) vs[j] = (uint8_t)(p.vs >> (8 * j)); // <- the wait of this iteration (with the records)
    write_back(post); // the previous tile's stores drain under this tile's LDS phases

    if (fill == 0)
    {
      issue_next(e);
      // free space only: (tau, +64) where an on-ray candidate landed, else (tau, -64) where only off-ray ones did
      if (!HAS_S0)
      {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (vs[j] & (VOX_TOUCHED | VOX_NEGFREE))
          {
            entry[j] = pack_entry(a.tau, (vs[j] & VOX_TOUCHED) ? WEIGHT_RESOLUTION : -WEIGHT_RESOLUTION);
            touched |= 1u << j;
          }
      }
      __syncthreads(); // (keeps the workgroup's iterations together: release_tile below relies on it)
    }
    else
    {
      if (HAS_S0)
      {
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
          const int32_t v0 = entry_value(p.s0[j]);
          bound0[l0 + j] = (uint16_t)((j < nz && entry_weight(p.s0[j]) <= 0) ? (v0 < 0 ? -v0 : v0) + 1 : 0);
        }
        __syncthreads();
      }
      bool from_regs = cached; // pass 1 and scan A; the rounds stream (the registers then hold the next tile's records)
      auto scan_records = [&](auto &&f) {
        if (from_regs)
        {
#pragma unroll
          for (int k = 0; k < RES_MAXR; ++k)
            if (rrec[k] != REC_NONE)
            {
              const int32_t value = rec_value(rrec[k]);
              const int32_t av = value < 0 ? -value : value;
              const int l = (int)rec_local(rrec[k]);
              if (HAS_S0 && av >= (int32_t)bound0[l]) continue; // rejected by the stored entry, now and for ever
              f((uint64_t)rrec[k], value, av, l);
            }
        }
        // what the registers do not hold: everything (the ordered rounds: the registers hold the next tile's records by then),
        // or the sub-chunks beyond the 64th of a heavy tile
        if (!from_regs || fill > (uint32_t)(8 * RES_MAXR))
        {
          for_each_record(a, tile, fill, p.cid, from_regs ? (uint32_t)(8 * RES_MAXR) : 0u, [&](uint64_t rec, int32_t value, int32_t av, int l) {
            if (HAS_S0 && av >= (int32_t)bound0[l]) return;
            f(rec, value, av, l);
          });
        }
      };
      // scan A: the negatives that come before the current positive candidate and can block it
      // (first: right behind pass 1 every voxel's mstate is still M_NONE -- nothing to look up there)
      auto scan_a = [&](auto first) {
        scan_records([&](uint64_t rec, int32_t value, int32_t av, int l) {
          if (!rec_negative(rec, a.fan_mask, a.fan_mid)) return;
          if (!decltype(first)::value)
          {
            const uint32_t m = mstate[l];
            if (m == M_IDLE || (uint32_t)av >= m) return;
          }
          const unsigned long long P = kpos[l];
          if (P == KEY_INF || rec > P) return;
          const int32_t vp = rec_value(P);
          if (av < (vp < 0 ? -vp : vp)) atomicMin(&mstate[l], (uint32_t)av);
        });
      };
      auto negative_entry = [&](unsigned long long N) {
        // no positive candidate is accepted: the negatives fold to the smallest |value|, latest on ties
        const int32_t an = neg_key_abs(N);
        const int32_t v = (N & 1ull) ? -an : an;
        return pack_entry(v, -weight_of(v));
      };

      // ---- pass 1: earliest positive, smallest negative per voxel
      scan_records([&](uint64_t rec, int32_t value, int32_t av, int l) {
        // (one LDS atomic with a selected address and key instead of two exec-mask regions per record)
        const bool neg = rec_negative(rec, a.fan_mask, a.fan_mid);
        const unsigned long long key = neg ? (unsigned long long)neg_key(rec, av, value) : (unsigned long long)rec;
#if WS_RESOLVE_KO & 2
        if (key == 0x12345ull) atomicMin(neg ? &kneg[l] : &kpos[l], key); // (never)
#else
        atomicMin(neg ? &kneg[l] : &kpos[l], key);
#endif
      });
      __syncthreads();
      // (round 6, measured and not kept: scan A only for tiles that hold off-ray records at all -- 105.9 us against 106.0:
      // nearly every tile of the benchmark scan does.  Knock-out builds, WS_RESOLVE_KO: scan A 14 us, the atomics of pass 1 16,
      // the rest of the fold 33, the kernel without any fold 50.)
      // (and: scan A only for the tiles that have a voxel whose smallest negative comes AFTER its earliest positive -- if it comes before,
      // it is itself the minimum scan A looks for -- decided per voxel behind pass 1, one more barrier: 29 % of the benchmark scan's
      // 19 535 tiles go without scan A then, 1.23 M of its voxels are contested, and the kernel takes 110.5 us against 102.3.)
#if !(WS_RESOLVE_KO & 1)
      scan_a(std::true_type{});
#endif
      __syncthreads();
      // this tile's records are not needed again (unless it needs ordered rounds, which stream): everything the next
      // iterations need is requested NOW and arrives under the decide phase, the barrier and the write-back
      from_regs = false;
      issue_next(e);

      // ---- decide
      uint32_t unres = 0; // bit j: voxel j is still open
#pragma unroll
      for (int j = 0; j < 4; ++j)
      {
        const unsigned long long P = kpos[l0 + j], N = kneg[l0 + j];
        const uint32_t m = mstate[l0 + j];
        bool open = false;
        if (j < nz && !(P == KEY_INF && N == KEY_INF))
        {
          touched |= 1u << j;
          if (P == KEY_INF)
          {
            entry[j] = negative_entry(N);
          }
          else
          {
            const int32_t vp = rec_value(P);
            const uint32_t ap = (uint32_t)(vp < 0 ? -vp : vp);
            if (N != KEY_INF && ap > (uint32_t)neg_key_abs(N)) n_contested += 1; // a negative candidate COULD have blocked it
            if (ap <= m)
            {
              entry[j] = pack_entry(vp, weight_of(vp));
            }
            else
            {
              // blocked: every later positive candidate needs |value| <= m (which stays in mstate)
              open = true;
              unres |= 1u << j;
              klast[l0 + j] = P;
              kpos[l0 + j] = KEY_INF;
            }
          }
        }
        else if (j < nz && !HAS_S0 && (vs[j] & (VOX_TOUCHED | VOX_NEGFREE)))
        {
          entry[j] = pack_entry(a.tau, (vs[j] & VOX_TOUCHED) ? WEIGHT_RESOLUTION : -WEIGHT_RESOLUTION);
          touched |= 1u << j;
        }
        if (!open)
        {
          // decided: ready for the next tile
          kpos[l0 + j] = KEY_INF;
          kneg[l0 + j] = KEY_INF;
          mstate[l0 + j] = M_NONE;
        }
      }
      if (unres) atomicAdd(&s_unres[0], 1u);
      __syncthreads();

      if (s_unres[0] != 0)
      {
        // ---- ordered rounds (some voxel of the tile had its earliest positive candidate blocked)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!(unres & (1u << j))) mstate[l0 + j] = M_IDLE;
        if (threadIdx.x == 0) s_unres[1] = 0;
        __syncthreads();
        int phase = 0;
        for (;;)
        {
          // B: the next positive candidate that can still be accepted
          scan_records([&](uint64_t rec, int32_t value, int32_t av, int l) {
            if (rec_negative(rec, a.fan_mask, a.fan_mid)) return;
            const uint32_t m = mstate[l];
            if (m == M_IDLE || (uint32_t)av > m) return;
            if (rec > klast[l]) atomicMin(&kpos[l], (unsigned long long)rec);
          });
          __syncthreads();
#pragma unroll
          for (int j = 0; j < 4; ++j)
          {
            if (!(unres & (1u << j))) continue;
            if (kpos[l0 + j] == KEY_INF)
            {
              entry[j] = negative_entry(kneg[l0 + j]);
              unres &= ~(1u << j);
              mstate[l0 + j] = M_IDLE;
            }
            else
            {
              mstate[l0 + j] = M_NONE;
            }
          }
          if (unres) atomicAdd(&s_unres[phase ^ 1], 1u);
          __syncthreads();
          if (threadIdx.x == 0) s_unres[phase] = 0;
          phase ^= 1;
          if (s_unres[phase] == 0) break;
          scan_a(std::false_type{});
          __syncthreads();
#pragma unroll
          for (int j = 0; j < 4; ++j)
          {
            if (!(unres & (1u << j))) continue;
            const unsigned long long P = kpos[l0 + j];
            const int32_t vp = rec_value(P);
            const uint32_t ap = (uint32_t)(vp < 0 ? -vp : vp);
            if (ap <= mstate[l0 + j])
            {
              entry[j] = pack_entry(vp, weight_of(vp));
              unres &= ~(1u << j);
              mstate[l0 + j] = M_IDLE;
            }
            else
            {
              klast[l0 + j] = P;
              kpos[l0 + j] = KEY_INF;
            }
          }
          if (unres) atomicAdd(&s_unres[phase ^ 1], 1u);
          __syncthreads();
          if (threadIdx.x == 0) s_unres[phase] = 0;
          phase ^= 1;
          if (s_unres[phase] == 0) break;
        }
        __syncthreads();
        if (threadIdx.x == 0) s_unres[0] = s_unres[1] = 0;
        init_lds();
        __syncthreads();
      }
    }

    // Nobody reads the tile's tables again: every thread's prefetch of them was consumed before the last barrier of the
    // PREVIOUS iteration, the passes that stream the sub-chunks from memory ended before the last barrier of this one.
    release_tile(tile, nsub_real);

    // ---- this tile's result waits in registers until the next iteration's loads have arrived
    post.idx0 = idx0;
    post.nz = nz;
    post.tile = tile;
    post.vs = p.vs;
    post.touched = touched;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      post.value[j] = entry[j];
    }
    post.existing[0] = ex_cur.x; post.existing[1] = ex_cur.y; post.existing[2] = ex_cur.z; post.existing[3] = ex_cur.w;
    tile_cur = tile_n1;
    p_cur = p_n1;
    cached = cached_next;
    ex_cur = ex_next;
    tile_n1 = te_n2.tile;
    p_n1 = p_n2;
    te_n2 = te_n3;
  }
  write_back(post);
  } // listed tiles

  // ---- Tiles that are NOT on the list: no records, only marks of the free pass or of off-ray +tau candidates in the byte
  // planes -- (tau, +64) / (tau, -64) where a mark is, nothing to fold.  They are found by scanning the per-tile flag planes
  // (a byte per tile; the marches only ever STORE there: no atomic, no waiting in their loops), 16 tiles per thread and step,
  // granule g of workgroup b = b + G k so that a cluster of such tiles spreads over the grid.  The scan owns both planes
  // (it clears what it finds); the listed tiles above never look at them.
  if (!HAS_S0)
  {
    uint32_t *found = reinterpret_cast<uint32_t *>(kpos); // 2048 tile ids (the fold above is over)
    const int64_t n_gran = (a.n_tiles + 15) >> 4;
    uint8_t *const flag_mark = a.tile_dirty, *const flag_listed = a.tile_dirty + tile_flag_plane_bytes(a.n_tiles);
    __syncthreads();
    if (threadIdx.x == 0) s_unres[0] = 0;
    __syncthreads();
    for (int64_t k0 = 0; (int64_t)blockIdx.x + (int64_t)G * k0 < n_gran; k0 += 128)
    {
      const int64_t g = (int64_t)blockIdx.x + (int64_t)G * (k0 + threadIdx.x);
      if (threadIdx.x < 128 && g < n_gran)
      {
        const u32x4 d = *reinterpret_cast<const u32x4 *>(flag_mark + 16 * g), h = *reinterpret_cast<const u32x4 *>(flag_listed + 16 * g);
        const uint32_t dw[4] = {d.x, d.y, d.z, d.w}, hw[4] = {h.x, h.y, h.z, h.w};
        const u32x4 zero = {0, 0, 0, 0};
        if (d.x | d.y | d.z | d.w) *reinterpret_cast<u32x4 *>(flag_mark + 16 * g) = zero;
        if (h.x | h.y | h.z | h.w) *reinterpret_cast<u32x4 *>(flag_listed + 16 * g) = zero;
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
          const uint32_t dj = (dw[j >> 2] >> (8 * (j & 3))) & 0xffu, hj = (hw[j >> 2] >> (8 * (j & 3))) & 0xffu;
          if (dj != 0 && hj == 0 && 16 * g + j < a.n_tiles) found[atomicAdd(&s_unres[0], 1u)] = (uint32_t)(16 * g + j);
        }
      }
      __syncthreads();
      const uint32_t n_found = s_unres[0];
      if (n_found && threadIdx.x == 0) atomicAdd(&a.counters->last_unlisted, n_found);
      for (uint32_t i = 0; i < n_found; ++i)
      {
        const uint32_t tile = found[i];
        const int32_t tz = (int32_t)(tile % (uint32_t)a.ntz);
        const uint32_t colt = tile / (uint32_t)a.ntz;
        const int32_t ty = (int32_t)(colt % (uint32_t)a.nty), tx = (int32_t)(colt / (uint32_t)a.nty);
        const int32_t sx = (tx << TILE_XB) + lx, sy = (ty << TILE_YB) + ly, sz = (tz << TILE_ZB) + z0;
        const bool col_ok = sx < a.map.size[0] && sy < a.map.size[1];
        int nz = a.map.size[2] - sz;
        nz = !col_ok ? 0 : (nz > 4 ? 4 : (nz < 0 ? 0 : nz));
        const int64_t idx0 = nz ? storage_index(a.map, sx, sy, sz) : 0;
        const uint32_t keep = nz >= 4 ? 0xffffffffu : ((1u << (8 * nz)) - 1u);
        const size_t vb = ((size_t)tile << 10) + voff;
        const uint32_t vs4 = (*reinterpret_cast<const uint32_t *>(a.vstate + vb) | ((*reinterpret_cast<const uint32_t *>(vneg + vb) & 0x01010101u) << 3)) & keep;
        u32x4 ex = {0, 0, 0, 0};
        if (FUSED) ex = *reinterpret_cast<const u32x4_a4 *>(a.avg_data + idx0);
        TilePost w;
        w.idx0 = idx0;
        w.nz = nz;
        w.tile = tile;
        w.vs = vs4;
        w.touched = 0;
        w.existing[0] = ex.x; w.existing[1] = ex.y; w.existing[2] = ex.z; w.existing[3] = ex.w;
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
          const uint32_t b = (vs4 >> (8 * j)) & 0xffu;
          w.value[j] = (b & (VOX_TOUCHED | VOX_NEGFREE)) ? pack_entry(a.tau, (b & VOX_TOUCHED) ? WEIGHT_RESOLUTION : -WEIGHT_RESOLUTION) : reset;
          if (b & (VOX_TOUCHED | VOX_NEGFREE)) w.touched |= 1u << j;
        }
        write_back(w);
        if (!FUSED && !aborted && threadIdx.x == 0)
        {
          TileEntry e;
          e.tile = tile;
          e.tx = tx; e.ty = ty; e.tz = tz;
          // behind the marches' entries, through a counter of its own: n_listed is what every workgroup of this launch read on
          // entry (a workgroup that starts late must not take an appended tile for a listed one)
          a.tile_list[n_list + atomicAdd(&a.counters->n_appended, 1u)] = e;
        }
      }
      __syncthreads();
      if (threadIdx.x == 0) s_unres[0] = 0;
      __syncthreads();
    }
  }

  // statistics: one slot per workgroup, no shared counter
  for (int d = 32; d > 0; d >>= 1) n_contested += __shfl_down(n_contested, d, 64);
  __shared__ uint32_t s_stat[4];
  if ((threadIdx.x & 63) == 0) s_stat[threadIdx.x >> 6] = n_contested;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    a.resolve_stats[2 * blockIdx.x + 0] = s_stat[0] + s_stat[1] + s_stat[2] + s_stat[3];
    a.resolve_stats[2 * blockIdx.x + 1] = n_mine;
#ifdef WS_RESOLVE_TIMING
    // (instead of the statistics: 10 ns ticks this workgroup was busy, and when it started)
    a.resolve_stats[2 * blockIdx.x + 0] = (uint32_t)(wall_clock64() - t_begin);
    a.resolve_stats[2 * blockIdx.x + 1] = (uint32_t)t_begin;
#endif
  }
}

// the resolve's arguments for the scatter whose marches ran with `sa`
static ResolveArgs make_resolve_args(ws_map *m, const ScatterArgs &sa)
{
  ResolveArgs ra;
  ra.tile_list = m->tile_list.as<TileEntry>();
  ra.tile_nsub = m->tile_nsub.as<uint32_t>();
  ra.tile_ent = m->tile_ent.as<uint32_t>();
  ra.sub_cap = m->sub_cap;
  ra.tile_dirty = m->tile_dirty.as<uint8_t>();
  ra.recs = m->rec.as<unsigned long long>();
  ra.big_keys = m->big_keys.as<unsigned long long>();
  ra.big_mask = m->big_slots - 1;
  ra.scan_seq = sa.scan_seq;
  ra.fan_mask = (1u << (sa.rec_fmt >> 8)) - 1u;
  ra.fan_mid = rec_fan_mid((int32_t)(sa.rec_fmt >> 8));
  ra.new_data = m->data[WS_MAP_NEW].as<uint32_t>();
  ra.avg_data = m->data[WS_MAP_AVG].as<uint32_t>();
  ra.vstate = m->vstate.as<uint8_t>();
  ra.map = m->par[WS_MAP_NEW];
  ra.nty = m->nty;
  ra.ntz = m->ntz;
  ra.tau = m->tau;
  ra.max_weight = m->max_weight;
  {
    const FastDiv wd = make_fastdiv(m->tau - m->tau / 10);
    ra.wM32 = (uint32_t)wd.M;
    ra.wS = wd.k - 32;
  }
  ra.resolve_stats = m->block_stats.as<uint32_t>() + 2 * WS_TAIL_STATS;
  ra.counters = m->counters.as<TsdfCounters>();
  ra.status = m->status.dev_as<uint32_t>();
  ra.n_tiles = m->n_tiles;
  return ra;
}
void launch_tile_resolve(ws_map *m, const ScatterArgs &sa, bool s0, bool fuse, hipStream_t s)
{
  const ResolveArgs ra = make_resolve_args(m, sa);
  const dim3 block(256);
  m->resolve_blocks = RESOLVE_GRID;
  if (s0)
    hipLaunchKernelGGL((tile_resolve_kernel<true, false>), dim3(RESOLVE_GRID), block, 0, s, ra);
  else if (fuse)
    hipLaunchKernelGGL((tile_resolve_kernel<false, true>), dim3(RESOLVE_GRID), block, 0, s, ra);
  else
    hipLaunchKernelGGL((tile_resolve_kernel<false, false>), dim3(RESOLVE_GRID), block, 0, s, ra);
}
} // namespace ws
