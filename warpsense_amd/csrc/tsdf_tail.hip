// tsdf_tail.hip — the tail march of the TSDF scatter (gfx950): ray tails -> records, straight into sub-chunks of their tiles.
// (Survey: tsdf_update.hip.)
#include "tsdf_pool.h"

namespace ws
{
#ifndef WS_TAIL_KO
#define WS_TAIL_KO 0 // knock-out builds for timing (results wrong): 1 no voxel-byte stores, 2 no record store, 4 no table / record at all, 8 no rounds, 16 no publishing at the end
#endif
#ifndef WS_TAIL_WGS
#define WS_TAIL_WGS 5 // workgroups per CU the register budget is set for (six: 80 VGPRs, 16 of them spilled, 234 instead of 187 us)
#endif
constexpr int TAIL_SPLIT = WS_TAIL_SPLIT, TAIL_WAVES = WS_TAIL_WAVES; // workgroups that share the tails of one group of 64 rays (TAIL_WAVES parts each)
constexpr int TAIL_QCAP = 128; // queue entries per wave of the compacting walk (one sample phase adds at most 64)
constexpr uint32_t HT_EMPTY = 0xffffffffu;

typedef uint32_t __attribute__((aligned(1))) u32_a1; // four consecutive vstate bytes

// What a wave of the tail march keeps in LDS about the records it has made since it last published (wave_flush): nothing in
// here is shared with another wave -- no barrier, no waiting; LDS operations of one wave are performed in order.
//   key / cnt     the tiles of those records (open addressing) and how many each has: the counter's old value IS the record's
//                 place -- sub-chunk rank >> 5 of the wave's sub-chunks for that tile, position rank & 31
//   sub_of        the (local number of the) sub-chunks rank >> 5 = ..., modulo 4: one round of puts -- at most 64 records --
//                 spans three of a tile's sub-chunks at most
//   owner         local sub-chunk -> (slot, rank >> 5): what the flush publishes
//   blk           local sub-chunk l lives in pool sub-chunk blk[(l >> 5) & 7] + (l & 31): the wave's ids come in runs of 32
// Local numbers count up for the life of the wave; [flushed, n_local) are the ones not yet published, [n_local, covered) have
// an id waiting.  All of it modulo 256: flushed, rounded down to 32, and covered are never more than 256 apart.
constexpr int WT_BITS = 8, WT_SLOTS = 1 << WT_BITS;
constexpr uint32_t WT_SLOT_LIMIT = 224; // tiles in the table before the wave publishes and starts over
constexpr uint32_t WT_RING = 256;
constexpr uint32_t WT_LOCAL_LIMIT = 160; // sub-chunks in flight before it does
struct WaveTab
{
  uint32_t key[WT_SLOTS];
  uint32_t cnt[WT_SLOTS]; // (wave_flush: | first entry number << 13)
  uint8_t sub_of[WT_SLOTS][4];
  uint16_t owner[256];
  uint32_t blk[8];
  uint32_t n_local, n_slots, flushed, covered;
  uint32_t n_rec, n_groups; // statistics: records (general walk), (flush, tile) groups
};

__device__ __forceinline__ int wt_insert(WaveTab &wt, uint32_t tile, bool &fresh)
{
  uint32_t h = (tile * 0x9E3779B1u) >> (32 - WT_BITS);
  for (int p = 0; p < WT_SLOTS; ++p)
  {
    const uint32_t cur = wt.key[h];
    if (cur == tile) return (int)h;
    if (cur == HT_EMPTY)
    {
      const uint32_t old = atomicCAS(&wt.key[h], HT_EMPTY, tile);
      if (old == HT_EMPTY)
      {
        atomicAdd(&wt.n_slots, 1u);
        fresh = true;
      }
      if (old == HT_EMPTY || old == tile) return (int)h;
    }
    h = (h + 1) & (WT_SLOTS - 1);
  }
  return -1; // (never: wave_room keeps 32 slots free)
}

// The wave publishes the sub-chunks it has filled since the last time and empties its table.  Any set of lanes may call it
// (the general walk does, with whoever is there).  ONE memory round trip: a tile's entries are reserved with one atomic per
// (wave, tile) -- four tiles per lane travel together -- and written behind it; a tile that had no entries yet goes on the
// scan's tile list (one request to the list's counter per flush).
template <bool LAST = false> // LAST: the wave is through (its table is not used again: not emptied)
__device__ __forceinline__ void wave_flush(const ScatterArgs &a, WaveTab &wt)
{
  const unsigned long long act = __ballot(1);
  const int lane = threadIdx.x & 63;
  const uint32_t na = (uint32_t)__popcll(act), lr = (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
  const int leader = __ffsll((long long)act) - 1;
  const uint32_t n_local = wt.n_local, flushed = wt.flushed;
  if (n_local != flushed)
  {
    for (uint32_t s0 = 0; s0 < (uint32_t)WT_SLOTS; s0 += 4u * na)
    {
      uint32_t c[4], tile[4], j0[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
      {
        const uint32_t s = s0 + lr + (uint32_t)u * na;
        c[u] = s < (uint32_t)WT_SLOTS ? wt.cnt[s] : 0u;
        tile[u] = s < (uint32_t)WT_SLOTS ? wt.key[s] : 0u;
        j0[u] = 0;
        if (c[u]) j0[u] = __hip_atomic_fetch_add(&a.tile_nsub[tile[u]], (c[u] + (uint32_t)SUB_RECS - 1u) >> SUB_BITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      uint32_t my_first = 0, n_first = 0, n_used = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u)
      {
        const uint32_t s = s0 + lr + (uint32_t)u * na;
        const bool first = c[u] != 0 && j0[u] == 0;
        const unsigned long long fm = __ballot(first);
        if (first) my_first |= (((n_first + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull))) & 0x7fu) | 0x80u) << (8 * u);
        n_first += (uint32_t)__popcll(fm);
        n_used += (uint32_t)__popcll(__ballot(c[u] != 0));
        if (c[u])
        {
          if (j0[u] >= (1u << 19) - 256u) raise_error(a.counters, a.status, ERR_INTERNAL); // (half a million entries of one tile: never)
          wt.cnt[s] = c[u] | (j0[u] << 13);
        }
      }
      // (a lane's place among the firsts travels in seven bits: a flush of more than 127 new tiles takes the list places one by one)
      if (n_first)
      {
        if (n_first < 128u)
        {
          uint32_t lb = 0;
          if (lane == leader) lb = __hip_atomic_fetch_add(&a.counters->n_listed, n_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          lb = (uint32_t)__builtin_amdgcn_readlane((int)lb, leader);
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (my_first & (0x80u << (8 * u))) list_tile(a, lb + ((my_first >> (8 * u)) & 0x7fu), tile[u]);
        }
        else
        {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (my_first & (0x80u << (8 * u)))
              list_tile(a, __hip_atomic_fetch_add(&a.counters->n_listed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), tile[u]);
        }
      }
      if (lane == leader) wt.n_groups += n_used;
    }
    asm volatile("" ::: "memory");
    // the sub-chunks: entry number = the tile's reservation + the sub-chunk's number among the wave's for that tile
    const uint32_t nl = n_local - flushed;
    for (uint32_t q = lr; q < nl; q += na)
    {
      const uint32_t gl = (flushed + q) & (WT_RING - 1u);
      const uint32_t o = wt.owner[gl];
      const uint32_t s = o & 255u, sub = o >> 8;
      const uint32_t cj = wt.cnt[s];
      const uint32_t c = cj & 8191u, j0 = cj >> 13;
      const uint32_t ns = (c + (uint32_t)SUB_RECS - 1u) >> SUB_BITS;
      const uint32_t fill = sub + 1u == ns ? c - (sub << SUB_BITS) : (uint32_t)SUB_RECS;
      const uint32_t base = wt.blk[(gl >> 5) & (WT_RING / 32u - 1u)];
      if (sub < ns && base != SUB_LOST) entry_publish(a, wt.key[s], j0 + sub, make_entry(base + (gl & 31u), fill)); // (sub >= ns: the unused rest of a run)
    }
    asm volatile("" ::: "memory");
  }
  if (LAST) return;
  for (uint32_t s = lr; s < (uint32_t)WT_SLOTS; s += na)
  {
    wt.key[s] = HT_EMPTY;
    wt.cnt[s] = 0;
  }
  if (lane == leader)
  {
    wt.flushed = n_local;
    wt.n_slots = 0;
  }
  asm volatile("" ::: "memory");
}

// Room for `n_put` more records (n_put <= 64), whatever tiles they fall into: each can open one sub-chunk and one table slot
// at most.  Publishes and / or asks the pool for 32 more ids when it must; returns how many records the wave can put before
// it has to ask again (>= 64).  Uniform over the calling lanes.
__device__ __forceinline__ uint32_t wave_room(const ScatterArgs &a, WaveTab &wt)
{
  const unsigned long long act = __ballot(1);
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)act) - 1;
  uint32_t nl = wt.n_local, ns = wt.n_slots, fl = wt.flushed, cov = wt.covered;
  constexpr uint32_t PER_PUT = 1u; // local numbers (sub-chunks) a put can open
  constexpr uint32_t NEED = 64u * PER_PUT;             // ... a round of 64 puts
  if (nl - fl + NEED > WT_LOCAL_LIMIT || ns + 64u > WT_SLOT_LIMIT || (cov - nl < NEED && cov + NEED - (fl & ~31u) > WT_RING))
  {
    wave_flush(a, wt);
    fl = nl;
    ns = 0;
  }
  while (cov - nl < NEED)
  {
    // (flushed above if the ring of blocks had no place for more)
    uint32_t b = 0;
    if (lane == leader)
    {
      b = pool_grab(a, SUB_REFILL);
      for (uint32_t i = 0; i < SUB_REFILL; i += 32u) wt.blk[((cov + i) >> 5) & (WT_RING / 32u - 1u)] = b == SUB_LOST ? SUB_LOST : b + i;
      wt.covered = cov + SUB_REFILL;
    }
    cov += SUB_REFILL;
  }
  asm volatile("" ::: "memory");
  const uint32_t r0 = (WT_LOCAL_LIMIT - (nl - fl)) / PER_PUT, r1 = WT_SLOT_LIMIT - ns, r2 = (cov - nl) / PER_PUT;
  return min(r0, min(r1, r2));
}

// one record of the wave: its tile's slot, its rank there, the sub-chunk (opened by the record of rank 0 mod 32), its place
// Returns bit 0: the record opened a sub-chunk, bit 1: its tile is new in the table (what the caller's room shrinks by).
template <bool SMALL>
__device__ __forceinline__ uint32_t wave_put(const ScatterArgs &a, WaveTab &wt, uint32_t tile, unsigned long long rec)
{
  bool fresh = false;
  const int s = wt_insert(wt, tile, fresh);
  if (s < 0)
  {
    raise_error(a.counters, a.status, ERR_INTERNAL);
    return 0;
  }
  // (the lanes of a wave mostly hit ONE counter, and the LDS takes such atomics one lane at a time: the old value is used for
  // everything -- no second atomic on the word)
  const uint32_t rank = atomicAdd(&wt.cnt[s], 1u);
  const uint32_t sub = rank >> SUB_BITS, pos = rank & (uint32_t)(SUB_RECS - 1);
  if (pos == 0)
  {
    const uint32_t g = atomicAdd(&wt.n_local, 1u);
    wt.sub_of[s][sub & 3u] = (uint8_t)g;
    wt.owner[g & 255u] = (uint16_t)((uint32_t)s | (sub << 8));
  }
  asm volatile("" ::: "memory");
  const uint32_t gl = wt.sub_of[s][sub & 3u];
  const uint32_t base = wt.blk[(gl >> 5) & 7u];
#if WS_TAIL_KO & 2
  if (base != SUB_LOST && rec == 0x12345ull) *rec_ptr<SMALL>(a.rec, base + (gl & 31u), pos) = rec; // (never)
#else
  if (base != SUB_LOST) *rec_ptr<SMALL>(a.rec, base + (gl & 31u), pos) = rec;
#endif
  return (pos == 0 ? 1u : 0u) | (fresh ? 2u : 0u);
}

// one work item: 64 direction-sorted rays x four of the 4 * TAIL_SPLIT parts of their tails (one part per wave): the scatter
// targets of a wave fall into the same vertical slab of space, i.e. into few tiles.  Every wave is on its own: its records go
// straight from the march into sub-chunks of their tiles (wave_put) and are published when it is through (wave_flush).
// (Round 4 measured two other shapes first: the records through a slice of a raw buffer in HBM and a copy by the workgroup
// into 2 KB chunks per tile -- 226-233 us, 66 of them the copy; and staged in LDS, flushed whenever the area filled up --
// 243-258 us, it costs two workgroups per CU of occupancy.)
template <bool SMALL>
__device__ __forceinline__ void tail_item(const ScatterArgs &a, const uint32_t item)
{
  __shared__ WaveTab s_tab[TAIL_WAVES];
  __shared__ u32x4 s_queue[TAIL_WAVES * TAIL_QCAP];
  __shared__ uint32_t s_stat[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  WaveTab &wt = s_tab[wave];
#ifdef WS_TAIL_TIMING
  const long long t_begin = wall_clock64();
#endif
  const uint32_t n_sorted = a.az_off[AZ_BINS];
  const uint32_t slot = (item / (uint32_t)TAIL_SPLIT) * 64u + (uint32_t)lane;
  const int part0 = (int)(item % (uint32_t)TAIL_SPLIT) * TAIL_WAVES; // this workgroup's parts of the tails
  const bool has_ray = slot < n_sorted;
  uint32_t ix = 0;
  RaySetup r;
  r.steps = 0;
  r.kfirst = 0;
  r.ub = 0;
  r.pad = 0;
  if (has_ray)
  {
    ix = a.ray_order[slot];
    r = a.rays[ix];
  }
  // ---- phase 0: the work item's block of sub-chunk ids (fixed: no request to anybody), every wave's table
  const uint32_t s_block = pool_holds_static(a) ? item * SUB_WG_BLOCK : SUB_LOST;
  if (threadIdx.x == 0)
  {
    if (s_block == SUB_LOST) raise_abort(a);
    s_stat[0] = s_stat[1] = 0;
    a.tail_stats[item] = 0;
    a.tail_stats[WS_TAIL_STATS + item] = 0;
  }
  for (int i = lane; i < WT_SLOTS; i += 64)
  {
    wt.key[i] = HT_EMPTY;
    wt.cnt[i] = 0;
  }
  if (lane == 0)
  {
    wt.n_local = wt.flushed = wt.n_slots = 0;
    wt.covered = SUB_WAVE_FIRST;
    wt.n_rec = wt.n_groups = 0;
  }
  __syncthreads();
  if (s_block == SUB_LOST) return; // (the scan is aborted: the host repeats it with a larger pool)
  if (lane < (int)(SUB_WAVE_FIRST / 32u)) wt.blk[lane] = s_block + (uint32_t)wave * SUB_WAVE_FIRST + (uint32_t)lane * 32u;
  int32_t k0 = 0, k1 = 0;
  if (has_ray && r.steps > 0 && r.kfirst < r.steps)
  {
    const int32_t kbeg = r.kfirst, kend = r.steps;
    const int32_t ch = (kend - kbeg + TAIL_WAVES * TAIL_SPLIT - 1) / (TAIL_WAVES * TAIL_SPLIT);
    k0 = min(kbeg + (part0 + wave) * ch, kend);
    k1 = min(k0 + ch, kend);
  }
  const bool work = k0 < k1;
  uint32_t n_written = 0; // records this wave has made (uniform; the general walk counts in LDS)

  // ---- phase 1: march, one record per scatter target
  const MarchFrame f = make_march_frame(a.scanner_pos, a.res, a.tau, a.map);
  const bool mark = !a.all_keyed;
  uint8_t *const vneg = a.vstate + vstate_plane_bytes((int64_t)a.ntx * a.nty * a.ntz);
  // a record (sx, sy, sz: storage coordinates of its voxel); returns the voxel's tile
  auto put_record = [&](uint32_t rix, int32_t k, int32_t fan_minus_mid, int32_t value, int32_t sx, int32_t sy, int32_t sz, uint32_t &used) -> uint32_t {
    // the free-space pass must know that this voxel takes part in the key order
    // (as a non-temporal store -- the marks push the half-filled sub-chunk lines out of the L2: 380 MB of writes for 98 MB of
    // records -- the kernel takes 462 instead of 183 us)
    const uint32_t tile = tile_of(a.nty, a.ntz, sx, sy, sz), vox = vox_of(sx, sy, sz);
    if (mark) *vox_ptr<SMALL>(a.vstate, tile, vox) = VOX_KEYED;
    used = wave_put<SMALL>(a, wt, tile, make_rec(rix, k, fan_minus_mid, value, local_of(sx, sy, sz), REC_S(a), REC_F(a)));
    return tile;
  };
  // an off-ray candidate of value +tau: (tau, -64) whoever makes it, never ordered (see ray_setup_block) -> a mark in the second plane
  auto mark_negative = [&](int32_t sx, int32_t sy, int32_t sz, uint32_t listed_tile) {
    const uint32_t tile = tile_of(a.nty, a.ntz, sx, sy, sz);
    *vox_ptr<SMALL>(vneg, tile, vox_of(sx, sy, sz)) = 1;
    // (the tile of the sample's on-ray record is on the list through that record -- nearly always this tile too; any other gets
    // the byte the resolve scans for.  A blind store: a load here would be a wait for everything the wave has in flight.)
    if (tile != listed_tile) a.tile_dirty[tile] = 1;
  };

  const bool general = !__all(!work || ((r.pad & RAY_SIMPLE) && r.distance >= 2)); // (>= 2: the 32-bit multiplier of ws_dda.h)
  if (general)
  {
    // a ray of this wave wraps in int32 or leaves the window: the general walk with all its tests, record by record.  (The
    // literal form with its divisions for every ray of such a wave: exact for all of them, and without the carried-remainder
    // walk's state the kernel fits 80 vector registers -- six workgroups per CU -- without a spill; such waves are rare.)
    if (work)
      march_steps_direct(f, r, k0, k1, [&](int32_t kk, int32_t step, int32_t vx, int32_t vy, int32_t vz, int32_t value, bool positive) {
        const int32_t sx = ring_fast(vx, f.ringK[0], a.map.size[0]), sy = ring_fast(vy, f.ringK[1], a.map.size[1]),
                      sz = ring_fast(vz, f.ringK[2], a.map.size[2]);
        if (mark && !positive && value == a.tau)
        {
          mark_negative(sx, sy, sz, 0xffffffffu);
          return;
        }
        // fan step - mid: update_tsdf.cu:103-104 (`positive` == the on-ray step)
        const int32_t delta_z = wmul(DZ_PER_DISTANCE, 1 + kk * f.half) / MATRIX_RESOLUTION;
        // (the lanes reach this point in varying company: room for whoever is here, counted in LDS)
        (void)wave_room(a, wt);
        atomicAdd(&wt.n_rec, 1u);
        uint32_t used = 0;
        put_record(ix, kk, step - delta_z / f.res, value, sx, sy, sz, used);
      });
  }
  else if (__any(work))
  {
    // compacting walk (ws_march.h): the sample phase queues (position, step, ray) of every sample that enters a new
    // voxel column; the emit phase pops 64 of them and does update_tsdf.cu:81-125 with every lane busy
    u32x4 *queue = s_queue + wave * TAIL_QCAP;
    uint32_t qhead = 0, qtail = 0;
    uint32_t cap_left = 0; // records the wave may put before it looks at its bookkeeping again (uniform)
    const int32_t res = f.res, half = f.half, tau = f.tau, dist = r.distance;
    // the scan point (update_tsdf.cu:57), shifted by divB - half: what the biased voxel index of div_res_b is subtracted from
    const int32_t hshift = (int32_t)f.divB - half;
    const int32_t hitbx = f.posx + r.dx + hshift, hitby = f.posy + r.dy + hshift, hitbz = f.posz + r.dz + hshift;
    AxisRun ix0, iy0, iz0;
    ix0.r = ix0.ar = ix0.aq = ix0.q = ix0.spos = ix0.sm = 0;
    ix0.gap = 0x3fffffff;
    iy0 = ix0;
    iz0 = ix0;
    int32_t k = k0; // the next sample of this lane
    if (work)
    {
      const int32_t kinit = k0 > 0 ? k0 - 1 : 0;
      run_init(ix0, f, r, r.dx, f.posx, kinit, true);
      run_init(iy0, f, r, r.dy, f.posy, kinit, true);
      run_init(iz0, f, r, r.dz, f.posz, kinit, false);
    }
    // the branch-free sample step of ws_march.h (lanes that are through keep stepping, masked)
    AxisFast wx = fast_from(ix0, work ? dist : 1), wy = fast_from(iy0, work ? dist : 1), wz = fast_from(iz0, work ? dist : 1);
    auto push = [&](unsigned long long mask /* ballot of cand */, bool cand, bool cx, bool cy) {
      if (mask == 0) return;
      if (cand)
      {
        u32x4 e;
        e.x = (uint32_t)fast_proj(wx, cx, res);
        e.y = (uint32_t)fast_proj(wy, cy, res);
        e.z = (uint32_t)fast_proj(wz, false, res);
        e.w = (uint32_t)k | ((uint32_t)lane << 16);
        const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        queue[(qtail + rank) & (TAIL_QCAP - 1)] = e;
      }
      qtail += (uint32_t)__popcll(mask);
    };
    {
      // the sample k == 0 is compared with the voxel column (0, 0) (update_tsdf.cu:65,71) and is where the walk starts: out
      // of the loop, so that every iteration is "step, then test"
      bool first = false;
      if (work && k0 == 0) first = div_res(fast_proj(wx, false, res), f) != 0 || div_res(fast_proj(wy, false, res), f) != 0;
      push(__ballot(first), first, false, false);
      if (work && k0 == 0) k = 1;
    }
    int32_t todo = work ? k1 - k : 0;
    for (int d = 32; d > 0; d >>= 1) todo = max(todo, __shfl_xor(todo, d, 64));
    const int32_t n_iter = __builtin_amdgcn_readfirstlane(todo);
    // emit phase: up to 64 queued samples, one per lane
    auto emit_batch = [&]() {
      const uint32_t cnt = qtail - qhead;
      const uint32_t n = cnt < 64 ? cnt : 64;
      u32x4 e = {0, 0, 0, 0};
      const bool has = (uint32_t)lane < n;
      if (has) e = queue[(qhead + (uint32_t)lane) & (TAIL_QCAP - 1)];
      qhead += n;
      // constants of the ray the sample belongs to (a lane of this wave)
      const int src = (int)(e.w >> 16);
      const int32_t s_hitx = __shfl(hitbx, src, 64), s_hity = __shfl(hitby, src, 64), s_hitz = __shfl(hitbz, src, 64);
      const int32_t s_ivx = __shfl(r.ivx, src, 64), s_ivy = __shfl(r.ivy, src, 64), s_ivz = __shfl(r.ivz, src, 64);
      const int32_t s_dist = __shfl(r.distance, src, 64);
      const uint32_t s_ix = (uint32_t)__shfl((int)ix, src, 64);
      const int32_t ek = (int32_t)(e.w & 0xffffu);
      const int32_t projx = (int32_t)e.x, projy = (int32_t)e.y, projz = (int32_t)e.z;
      const int32_t len = 1 + ek * half;
      // update_tsdf.cu:81-98 (no int32 wrap for a RAY_SIMPLE ray: 24-bit multiplies are exact).  The voxel's index comes biased by
      // divBq (div_res_b): centre = (q - divBq) res + half, and the hit point was shifted by divB - half once per ray
      const int32_t ddx = s_hitx - (int32_t)__umul24(div_res_b(projx, f), (uint32_t)res), ddy = s_hity - (int32_t)__umul24(div_res_b(projy, f), (uint32_t)res),
                    ddz = s_hitz - (int32_t)__umul24(div_res_b(projz, f), (uint32_t)res);
      int32_t value = (int32_t)sqrtf((float)(__mul24(ddx, ddx) + __mul24(ddy, ddy) + __mul24(ddz, ddz)));
      value = value < tau ? value : tau;
      if (len > s_dist) value = -value;
      // update_tsdf.cu:101-105
      const int32_t delta_z = (DZ_PER_DISTANCE * len) >> 15; // len > 0
      int32_t iter_steps = 0, mid = 0;
      if (has && !tsdf_weight_is_zero(value, tau, f.weight_epsilon))
      {
        iter_steps = 1;
        if (delta_z * 2 >= res)
        {
          iter_steps = (int32_t)(__umulhi((uint32_t)(delta_z * 2), f.rM32) >> f.rS) + 1;
          mid = (int32_t)(__umulhi((uint32_t)delta_z, f.rM32) >> f.rS);
        }
      }
      if (!__any(iter_steps > 0)) return;
      // the off-ray targets of a sample of value +tau are marks, not records
      const bool blind = mark && value == tau;
      const unsigned long long m_blind = mark ? __ballot(value == tau) : 0ull;
      // The fan (update_tsdf.cu:107-112): target j = (lowest + trunc(j res iv / 32768)) / res.  The products grow by res * iv
      // from one fan step to the next and their sign is iv's: `acc` carries j res iv + (iv < 0 ? 32767 : 0), the truncating
      // division by 32768 is its arithmetic shift -- one add and one shift per axis and round instead of multiply, sign, mask,
      // add, shift (round 6; the three multiply-shift divisions by res and the ring buffer: div_res_b / ring_b, ws_march.h)
      const int32_t bx = iv_bias(s_ivx), by = iv_bias(s_ivy), bz = iv_bias(s_ivz);
      const int32_t lowx = projx - trunc15_biased(delta_z, s_ivx, bx), lowy = projy - trunc15_biased(delta_z, s_ivy, by),
                    lowz = projz - trunc15_biased(delta_z, s_ivz, bz);
      const int32_t incx = __mul24(res, s_ivx), incy = __mul24(res, s_ivy), incz = __mul24(res, s_ivz);
      int32_t accx = bx, accy = by, accz = bz;
      // the parts of the record that belong to the sample (make_rec, ws_internal.h): u = step << F | fan, fan = round - mid + MID
      const int32_t recS = REC_S(a), recF = REC_F(a);
      const uint32_t rec_hi0 = s_ix << (recS + recF - 6), rec_lo0 = ((uint32_t)value & 0xffffu) << REC_VALUE_SHIFT;
      const uint32_t rec_u0 = ((uint32_t)ek << recF) + rec_fan_mid(recF) - (uint32_t)mid;
      // Rounds of at most one target per lane, fan step by fan step (update_tsdf.cu:107-125) IN THE FAN'S OWN ORDER: round j is
      // fan step j of every sample whose fan has more than j steps -- the on-ray target (always a record) where j == mid, an
      // off-ray one (a record, or a mark for a sample of value +tau) elsewhere.  The samples of a batch come from rays that
      // end in the same cell, i.e. of nearly the same length, and the fan's width depends on the length alone: the rounds run
      // 92 % full (tools/lane_model.py).  (Until round 5 the on-ray targets had a round of their own in front and every lane
      // sat out the round j == mid: 381 k rounds of 59 % instead of 244 k for the benchmark scan's 14.4 M targets.)  In front
      // of every round the wave makes sure its bookkeeping has room for the records of the round (a scalar compare, nearly always).
      uint32_t mid_tile = 0xffffffffu; // the tile of the sample's on-ray record, once that is made (it is on the list through it)
#if WS_TAIL_KO & 8
      if ((rec_hi0 ^ rec_u0 ^ (uint32_t)lowx ^ (uint32_t)lowy ^ (uint32_t)lowz ^ (uint32_t)incx ^ (uint32_t)incy ^ (uint32_t)incz ^ m_blind) == 0x12345u)
#endif
      for (int32_t round = 0;; ++round)
      {
        // (the loop bound as a ballot per round: a maximum over the lanes by shuffles is six trips through the LDS pipe per emit phase)
        const unsigned long long m_on = __ballot(round < iter_steps);
        if (m_on == 0) break;
        const bool on = round < iter_steps;
        const bool onray = round == mid;
        const bool puts = on && (onray || !blind);
        const uint32_t n_put = (uint32_t)__popcll(m_on & (__ballot(onray) | ~m_blind)); // ballot(puts), from scalar masks
        if (n_put)
        {
          // (every record of the round could open a sub-chunk and bring a new tile: room for that, then count what they did)
          if (cap_left < n_put) cap_left = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_room(a, wt));
          n_written += n_put;
        }
        // the target's storage coordinates (all lanes: the fan's state moves on in every round)
        const int32_t sx = ring_b(div_res_b(lowx + (accx >> 15), f), f.ringB[0], a.map.size[0]),
                      sy = ring_b(div_res_b(lowy + (accy >> 15), f), f.ringB[1], a.map.size[1]),
                      sz = ring_b(div_res_b(lowz + (accz >> 15), f), f.ringB[2], a.map.size[2]);
        accx += incx;
        accy += incy;
        accz += incz;
        uint32_t used = 0;
        if (on)
        {
          const uint32_t tile = tile_of(a.nty, a.ntz, sx, sy, sz), vox = vox_of(sx, sy, sz);
          if (!puts)
          {
            // an off-ray candidate of value +tau: a mark in the second plane (mark_negative)
#if !(WS_TAIL_KO & 1)
            *vox_ptr<SMALL>(vneg, tile, vox) = 1;
            if (tile != mid_tile) a.tile_dirty[tile] = 1;
#endif
          }
          else
          {
#if !(WS_TAIL_KO & 1)
            if (mark) *vox_ptr<SMALL>(a.vstate, tile, vox) = VOX_KEYED;
#endif
            const uint32_t u = rec_u0 + (uint32_t)round;
            const uint32_t hi = rec_hi0 | (u >> 6), lo = (u << REC_T_SHIFT) | rec_lo0 | local_of(sx, sy, sz);
#if WS_TAIL_KO & 4
            if ((hi ^ lo ^ tile) == 0x12345u) used = wave_put<SMALL>(a, wt, tile, ((unsigned long long)hi << 32) | lo); // (never: keeps the arithmetic alive)
#else
            used = wave_put<SMALL>(a, wt, tile, ((unsigned long long)hi << 32) | lo);
#endif
            if (onray) mid_tile = tile;
          }
        }
        if (n_put)
        {
          const uint32_t n_open = (uint32_t)__popcll(__ballot(used & 1u)), n_new = (uint32_t)__popcll(__ballot(used & 2u));
          cap_left -= n_open > n_new ? n_open : n_new;
        }
      }
    };
    for (int32_t it = 0; it < n_iter; ++it)
    {
      // ---- sample phase
      const bool cx = fast_step(wx, res), cy = fast_step(wy, res);
      fast_step_z(wz);
      // (ballots of the simple conditions, combined as scalars: the ballot of a conjunction costs two vector instructions more)
      push((__ballot(cx) | __ballot(cy)) & __ballot(k < k1), (cx || cy) && k < k1, cx, cy);
      k += 1;
      // ---- emit phase: 64 queued samples, one per lane
      if (qtail - qhead >= 64) emit_batch();
    }
    while (qtail != qhead) emit_batch();
  }
#ifdef WS_TAIL_TIMING
  const long long t_mid = wall_clock64();
#endif
  // ---- phase 2: the wave publishes what it has filled
#if !(WS_TAIL_KO & 16)
  wave_flush<true>(a, wt);
#endif
  if (lane == 0)
  {
    atomicAdd(&s_stat[0], n_written + wt.n_rec);
    atomicAdd(&s_stat[1], wt.n_groups);
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    a.tail_stats[item] = s_stat[0];
    a.tail_stats[WS_TAIL_STATS + item] = s_stat[1];
  }
#ifdef WS_TAIL_TIMING
  // (instead of the statistics: 10 ns ticks of the march and of the flush of this item, and when it started)
  if (threadIdx.x == 0)
  {
    a.tail_stats[item] = (uint32_t)(t_mid - t_begin);
    a.tail_stats[WS_TAIL_STATS + item] = (uint32_t)(wall_clock64() - t_mid);
    a.tail_stats[2 * WS_TAIL_STATS + 8192 + item] = (uint32_t)t_begin;
  }
#endif
}

template <bool SMALL> // SMALL: 32-bit offsets into the voxel bytes and the record pool (vox_ptr)
__global__ __launch_bounds__(64 * WS_TAIL_WAVES, WS_TAIL_WGS * 4 / WS_TAIL_WAVES) void march_tail_kernel(ScatterArgs a)
{
  // the direction histogram has been consumed by the sort blocks of this scan: zero for the next one (no clean-up launch)
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < (uint32_t)(AZ_BINS + 1); i += gridDim.x * blockDim.x) a.az_hist[i] = 0;
  const uint32_t n_items = ((a.n + 63u) / 64u) * (uint32_t)TAIL_SPLIT;
  // (No look at counters->abort here, although a scan that the set-up pass has aborted for a ray beyond the key range could leave at
  // once: the word shares its cache line with the pool's cursor, which other workgroups of THIS launch hit with atomics -- every
  // workgroup starting with a load of it took the kernel from 135 to 210 us.  Such a scan marches in vain and is repeated in pieces.)
  if (blockIdx.x < n_items) tail_item<SMALL>(a, blockIdx.x);
}

void launch_march_tail(ws_map *m, const ScatterArgs &sa, bool small, hipStream_t s)
{
  const dim3 grid_tail((unsigned)(((size_t)sa.n + 63) / 64) * TAIL_SPLIT);
  m->tail_blocks = grid_tail.x;
  if (small)
    hipLaunchKernelGGL(march_tail_kernel<true>, grid_tail, dim3(64 * TAIL_WAVES), 0, s, sa);
  else
    hipLaunchKernelGGL(march_tail_kernel<false>, grid_tail, dim3(64 * TAIL_WAVES), 0, s, sa);
}
} // namespace ws
