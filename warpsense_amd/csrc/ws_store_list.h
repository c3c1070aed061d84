// ws_store_list.h — the chunk list of a store call, on the host.  A call on the chunk store LISTS the written chunks it works on:
// {cx, cy, cz, slot} each, ascending (cx, cy, cz) like the directory (store_list, api_store_query.hip).  Everything a call derives
// from its list alone is here, once: the chunks of a box, the limit of a list, the word-space tables, the live box, the z range and
// the list positions of neighbours.  Pure host functions over the list and plain integers: no HIP call, no ws_store, no lock
// (tests/cpp/store_list_units.hip restates each by brute force).
#pragma once

#include <algorithm>
#include <array>
#include <cstring>
#include <vector>

#include "ws_internal.h"

namespace ws
{
using StoreKey = std::array<int32_t, 3>;

// A call lists fewer than 2^19 chunks.  The 4096 words of each listed chunk are numbered in one word space (ws_store_words.h) that
// must stay below 2^31, and the lookup of the listed chunks has store_ray_table_slots(n) <= 2^20 places of 16 bytes, whose count
// and bytes fit the uint32_t the kernels carry them in.  Every entry point refuses a longer list in its own words.
constexpr size_t STORE_LIST_LIMIT = (size_t)1 << 19;

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

// The word-space tables of the n listed chunks (n < STORE_LIST_LIMIT) at `grp`, store_word_table_bytes(n): per chunk the four counts
// {B, N, P, n} that place its 4096 words in world order (ws_store_words.h), then its key and slot.  An empty list writes nothing.
inline void store_word_tables(const std::vector<StoreRaySlot> &listed, uint32_t *grp)
{
  const size_t n = listed.size();
  if (n) std::memcpy(grp + 4 * n, listed.data(), n * sizeof(StoreRaySlot)); // {cx, cy, cz, slot} per chunk
  for (size_t b = 0; b < n;) // the chunks of one cx: [b, e)
  {
    size_t e = b;
    while (e < n && listed[e].cx == listed[b].cx) ++e;
    for (size_t p = b; p < e;) // the chunks of one (cx, cy): [p, q)
    {
      size_t q = p;
      while (q < e && listed[q].cy == listed[p].cy) ++q;
      for (size_t i = p; i < q; ++i)
        grp[4 * i + 0] = (uint32_t)b, grp[4 * i + 1] = (uint32_t)(e - b), grp[4 * i + 2] = (uint32_t)(p - b), grp[4 * i + 3] = (uint32_t)(q - p);
      p = q;
    }
    b = e;
  }
}

// The live box of a call over the box [lo, hi]: the bounding box of the listed chunks (keys are floor(int32 / 64): 64 k + 63 fits, summed
// in that order: 64 k + 64 does not at the last key), cut to the box.  Nothing listed leaves INT32_MAX / INT32_MIN cut to the box: blo > bhi.
inline void store_live_box(const std::vector<StoreRaySlot> &listed, const int32_t lo[3], const int32_t hi[3], int32_t blo[3], int32_t bhi[3])
{
  for (int k = 0; k < 3; ++k) blo[k] = INT32_MAX, bhi[k] = INT32_MIN;
  for (const StoreRaySlot &e : listed)
  {
    const int32_t key[3] = {e.cx, e.cy, e.cz};
    for (int k = 0; k < 3; ++k) blo[k] = std::min(blo[k], key[k] * STORE_CS), bhi[k] = std::max(bhi[k], key[k] * STORE_CS + (STORE_CS - 1));
  }
  for (int k = 0; k < 3; ++k) blo[k] = std::max(blo[k], lo[k]), bhi[k] = std::min(bhi[k], hi[k]);
}

// The z range the listed chunks cover inside [lo_z, hi_z]; nothing listed: 1, 0
inline void store_z_range(const std::vector<StoreRaySlot> &listed, int32_t lo_z, int32_t hi_z, int32_t *zlo, int32_t *zhi)
{
  *zlo = 1, *zhi = 0;
  if (listed.empty()) return;
  *zlo = INT32_MAX, *zhi = INT32_MIN;
  for (const StoreRaySlot &e : listed) *zlo = std::min(*zlo, e.cz * STORE_CS), *zhi = std::max(*zhi, e.cz * STORE_CS + (STORE_CS - 1));
  *zlo = std::max(*zlo, lo_z), *zhi = std::min(*zhi, hi_z);
}

// The list positions of every listed chunk's neighbours at the n_off key offsets `off`, into nb[n_off * i + d]: 0xffffffffu where
// the list has no such chunk.  (Keys are floor(int32 / 64): a step of one cannot overflow.)  O(n n_off log n).
inline void store_neighbour_positions(const std::vector<StoreRaySlot> &listed, const int32_t (*off)[3], int n_off, uint32_t *nb)
{
  const auto before = [](const StoreRaySlot &e, const StoreKey &k) { return StoreKey{e.cx, e.cy, e.cz} < k; };
  for (size_t i = 0; i < listed.size(); ++i)
    for (int d = 0; d < n_off; ++d)
    {
      const StoreKey k = {listed[i].cx + off[d][0], listed[i].cy + off[d][1], listed[i].cz + off[d][2]};
      const auto it = std::lower_bound(listed.begin(), listed.end(), k, before);
      const bool found = it != listed.end() && it->cx == k[0] && it->cy == k[1] && it->cz == k[2];
      nb[(size_t)n_off * i + d] = found ? (uint32_t)(it - listed.begin()) : 0xffffffffu;
    }
}
} // namespace ws
