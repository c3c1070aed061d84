// tsdf_pool.h — the record pool and the tile lists of the TSDF scatter (gfx950) as the marches write them, second layer: sub-chunk
// ids out of the pool, a tile's entries (table, then hash), the scan's tile list, the abort flag.  Used by the tail march and the
// free pass; the resolve reads what they wrote and needs none of this.
#pragma once

#include "tsdf_scatter.h"

namespace ws
{
// the scan in flight ran out of sub-chunks: from here on nothing of it may reach the maps -- the resolve only puts the scratch
// back and the host repeats the scan with a larger pool (launch_tsdf_scatter)
__device__ __forceinline__ void raise_abort(const ScatterArgs &a)
{
  __hip_atomic_fetch_or(&a.counters->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (pool exhausted only; a ray beyond the key range goes to range_seq, ray_setup_block)
}

// The pool, bottom to top: [one block of SUB_WG_BLOCK ids per work item of the tail march | what its waves ask for on top of
// that (chunk_cursor, upwards) ... (free_cursor, downwards) what the waves of the free pass ask for on top of | FREE_WAVE_FIRST
// ids per wave of the free pass].  The fixed parts cost no request at all: a returning atomic on ONE address takes ~40 ns
// under load (measured: 25 000 of them, one per free-space record, made the free pass 1.16 ms instead of 0.12), so the
// shared counters are for the exceptions.
constexpr uint32_t FREE_WAVE_FIRST = WS_FREE_FIRST; // (subs_needed() counts them)
__device__ __forceinline__ uint32_t tail_static_subs(const ScatterArgs &a) { return ((a.n + 63u) / 64u) * (uint32_t)WS_TAIL_SPLIT * SUB_WG_BLOCK; }
__device__ __forceinline__ uint32_t free_static_subs(const ScatterArgs &a) { return ((a.n + 63u) / 64u) * 4u * FREE_WAVE_FIRST; }
__device__ __forceinline__ bool pool_holds_static(const ScatterArgs &a)
{
  return (unsigned long long)tail_static_subs(a) + free_static_subs(a) <= (unsigned long long)a.sub_cap;
}
// n more consecutive sub-chunk ids for a wave of the tail march, or SUB_LOST
__device__ __forceinline__ uint32_t pool_grab(const ScatterArgs &a, uint32_t n)
{
  const uint32_t b = __hip_atomic_fetch_add(&a.counters->chunk_cursor, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long lo = (unsigned long long)tail_static_subs(a) + b;
  if (pool_holds_static(a) && lo + n <= (unsigned long long)a.sub_cap - free_static_subs(a)) return (uint32_t)lo;
  raise_abort(a);
  return SUB_LOST;
}
// ... for the free pass (the next launch: chunk_cursor is final), from the top down
__device__ __forceinline__ uint32_t free_grab(const ScatterArgs &a, uint32_t n)
{
  const unsigned long long lo = (unsigned long long)tail_static_subs(a) + a.counters->chunk_cursor;
  const uint32_t d = __hip_atomic_fetch_add(&a.counters->free_cursor, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long top = (unsigned long long)a.sub_cap - free_static_subs(a);
  if (pool_holds_static(a) && lo + d + n <= top) return (uint32_t)(top - d - n);
  raise_abort(a);
  return SUB_LOST;
}

// entry number j of `tile`: into the tile's table, or -- beyond TILE_DIRECT -- into the hash (value: entry + 1)
__device__ __forceinline__ void entry_publish(const ScatterArgs &a, uint32_t tile, uint32_t j, uint32_t ent)
{
  if (j < (uint32_t)TILE_DIRECT)
  {
    a.tile_ent[(size_t)tile * TILE_DIRECT + j] = ent;
    return;
  }
  const unsigned long long key = big_key(tile, j);
  uint32_t *vals = reinterpret_cast<uint32_t *>(a.big_keys + (size_t)a.big_mask + 1);
  uint32_t h = big_slot(key, a.big_mask);
  for (uint32_t probe = 0; probe <= a.big_mask; ++probe)
  {
    const unsigned long long old = atomicCAS(&a.big_keys[h], KEY_INF, key);
    if (old == KEY_INF || old == key)
    {
      // (a key stays in the table when its tile is released -- only the value goes back to 0 -- so that the probe chains
      // through it stay whole; the host empties the whole table before it fills up)
      if (old == KEY_INF) atomicAdd(&a.counters->big_inserted, 1u);
      vals[h] = ent + 1u;
      return;
    }
    h = (h + 1) & a.big_mask;
  }
  raise_error(a.counters, a.status, ERR_INTERNAL); // (the table has two slots per sub-chunk of the pool)
}
// the tile got its first entries: place `at` of the scan's tile list, and the flag byte that keeps the resolve's scan for
// tiles WITHOUT records away from it
__device__ __forceinline__ void list_tile(const ScatterArgs &a, uint32_t at, uint32_t tile)
{
  // tile -> (tx, ty, tz) by multiply-shift (constants behind the fan table, ws_map_create): exact for tile ids below 2^31
  const uint32_t Mz = (uint32_t)a.fan_steps[256], My = (uint32_t)a.fan_steps[258];
  const int32_t sz = a.fan_steps[257], sy = a.fan_steps[259];
  const uint32_t col = sz >= 0 ? __umulhi(tile, Mz) >> sz : tile;
  const uint32_t tx = sy >= 0 ? __umulhi(col, My) >> sy : col;
  TileEntry e;
  e.tile = tile;
  e.tz = (int32_t)(tile - col * (uint32_t)a.ntz);
  e.ty = (int32_t)(col - tx * (uint32_t)a.nty);
  e.tx = (int32_t)tx;
  a.tile_list[at] = e;
  a.tile_dirty[tile_flag_plane_bytes((int64_t)a.ntx * a.nty * a.ntz) + tile] = 1;
}
__device__ __forceinline__ uint32_t make_entry(uint32_t id, uint32_t fill) { return (id << SUB_BITS) | (fill - 1u); }

// one record in a sub-chunk of its own (a free-space candidate on a keyed voxel: 25 000 of the benchmark scan's 21 million)
__device__ __forceinline__ void append_single(const ScatterArgs &a, uint32_t tile, uint32_t id, unsigned long long rec)
{
  if (id == SUB_LOST) return;
  a.rec[(size_t)id << SUB_BITS] = rec;
  const uint32_t j = __hip_atomic_fetch_add(&a.tile_nsub[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  entry_publish(a, tile, j, make_entry(id, 1u));
  if (j == 0) list_tile(a, __hip_atomic_fetch_add(&a.counters->n_listed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), tile);
}
} // namespace ws
