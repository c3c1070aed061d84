// ws_store_words.h — the sparse, world-ordered word space of the chunk store, shared by its mesh (store_mesh.hip, whose head derives
// the index) and its surface cloud (store_surface.hip).  A word is one (x, y) column of one listed chunk, 64 voxels; its index
//
//     t = 4096 B + lx 64 N + 64 P + ly n + r
//
// ascends like world (x, y, cz).  The host writes, per listed chunk, {B, N, P, n} and {cx, cy, cz, slot} (store_word_tables,
// ws_store_list.h; store_word_table_bytes, ws_internal.h); the way back from t to the chunk and the column needs two table reads and no search.
#pragma once

#include "ws_device.h"

namespace ws
{
constexpr uint32_t SM_NONE = 0xffffffffu;

struct StoreWords
{
  uint32_t n_chunks, n_words; // listed chunks; 4096 words each (n_words < 2^31)
  const su32x4 *grp;          // [n_chunks] B, N, P, n
  const mi32x4 *key;          // [n_chunks] cx, cy, cz, slot
  uint32_t *const *segs;      // base pointers of the store's segments
  uint32_t seg_shift;
};

// the two tables of `n_chunks` listed chunks at `tab` (device memory) and the store's segments
inline void store_words_bind(StoreWords &a, const ws_store *st, const char *tab, uint32_t n_chunks)
{
  a.n_chunks = n_chunks;
  a.n_words = n_chunks * 4096u;
  a.grp = reinterpret_cast<const su32x4 *>(tab);
  a.key = reinterpret_cast<const mi32x4 *>(tab + (size_t)n_chunks * 16);
  a.segs = st->seg_tab.as<uint32_t *>();
  a.seg_shift = st->seg_shift;
}

__device__ __forceinline__ uint32_t sm_word(const su32x4 g, uint32_t i, uint32_t lx, uint32_t ly)
{
  return 4096u * g.x + lx * 64u * g.y + 64u * g.z + ly * g.w + (i - g.x - g.z);
}
__device__ __forceinline__ const uint32_t *sm_chunk(const StoreWords &a, uint32_t i)
{
  const uint32_t slot = (uint32_t)a.key[i].w;
  return a.segs[slot >> a.seg_shift] + (size_t)(slot & ((1u << a.seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
}

// a word of the sparse space: its chunk (list position), its column in the chunk
struct StoreWord
{
  uint32_t i, lx, ly;
  su32x4 g;
  __device__ __forceinline__ void find(const StoreWords &a, uint32_t t)
  {
    const su32x4 gx = a.grp[t >> 12];      // a chunk of the word's cx
    const uint32_t u = t - 4096u * gx.x;
    lx = u / (64u * gx.y);
    const uint32_t v = u - lx * 64u * gx.y;
    g = a.grp[gx.x + (v >> 6)];            // a chunk of the word's (cx, cy)
    const uint32_t w = v - 64u * g.z;
    ly = w / g.w;
    i = g.x + g.z + (w - ly * g.w);
  }
  // index of the word at column (lx + dx, ly + dy) of the chunk dz above, dx, dy, dz in {-1, 0, 1}; SM_NONE: no such word (a zero
  // word).  `a` carries the neighbour entries of the listed chunks as well (nb: [n_chunks][27], store_mesh.hip)
  template <typename Args> __device__ __forceinline__ uint32_t at(const Args &a, int dx, int dy, int dz) const
  {
    const int nx = (int)lx + dx, ny = (int)ly + dy;
    const int cx = nx >> 6, cy = ny >> 6; // -1, 0, 1
    if (cx == 0 && cy == 0 && dz == 0) return sm_word(g, i, (uint32_t)nx, (uint32_t)ny);
    const uint32_t j = a.nb[(size_t)i * 27u + (uint32_t)((cx + 1) * 9 + (cy + 1) * 3 + (dz + 1))];
    if (j == SM_NONE) return SM_NONE;
    return sm_word(a.grp[j], j, (uint32_t)(nx & 63), (uint32_t)(ny & 63));
  }
};

} // namespace ws
