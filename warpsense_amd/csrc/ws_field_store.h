// ws_field_store.h — the chunks of the store as the FIELD of ws_raycast.h: the chunk lookup, the loads inside and across chunks, and
// what the march may pass over.  Shared by the ray cast (store_raycast.hip) and the point sample (store_sample.hip) of the store.
#pragma once

#include "ws_raycast.h"

namespace ws
{
struct StoreRayArgs
{
  RayCommon c;
  int32_t lo[3], hi[3];   // the box, inclusive world voxels
  int32_t blo[3], bhi[3]; // the live box
  uint32_t n_chunks;      // 0: nothing is valid anywhere
  const StoreRaySlot *table;
  uint32_t mask;          // table places - 1
  uint32_t *const *segs;  // base pointers of the store's segments
  uint32_t seg_shift;
};

struct StoreField
{
#ifdef WS_STORE_RAY_NO_JUMP
  static constexpr bool JUMPS = false;
#else
  static constexpr bool JUMPS = true;
#endif
  const StoreRayArgs &a;
  int32_t ck[3];           // the chunk key of the last base voxel looked up ...
  const uint32_t *cp;      // ... and its words, nullptr if absent
  bool outside;            // the last load's base voxel was outside the live cell range (else an invalid cell's base chunk decides)
  __device__ __forceinline__ explicit StoreField(const StoreRayArgs &args) : a(args), ck{INT32_MIN, INT32_MIN, INT32_MIN}, cp(nullptr), outside(false) {}

  __device__ __forceinline__ const uint32_t *lookup(int32_t cx, int32_t cy, int32_t cz) const
  {
    const uint32_t slot = store_ray_find(a.table, a.mask, cx, cy, cz);
    if (slot == STORE_ABSENT) return nullptr;
    return a.segs[slot >> a.seg_shift] + (size_t)(slot & ((1u << a.seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
  }
  __device__ __forceinline__ const uint32_t *chunk(int32_t cx, int32_t cy, int32_t cz) const
  {
    return cx == ck[0] && cy == ck[1] && cz == ck[2] ? cp : lookup(cx, cy, cz);
  }
  // past the live box on an axis the ray moves away on (or stands still beside it): every later cell has a corner outside it
  __device__ __forceinline__ bool gone(const int32_t b[3], const int32_t sgn[3]) const
  {
    bool g = false;
#pragma unroll
    for (int x = 0; x < 3; ++x) g = g || (sgn[x] >= 0 && b[x] >= a.bhi[x]) || (sgn[x] <= 0 && b[x] < a.blo[x]);
    return g;
  }
  // the raw entries of the 8 corners of the cell with base voxel b, index cx * 4 + cy * 2 + cz; false if a corner is outside the live
  // box or in an absent chunk (raw is then not to be read)
  __device__ __forceinline__ bool gather(const int32_t b[3], uint32_t raw[8])
  {
    outside = b[0] < a.blo[0] || b[0] >= a.bhi[0] || b[1] < a.blo[1] || b[1] >= a.bhi[1] || b[2] < a.blo[2] || b[2] >= a.bhi[2];
    if (outside) return false;
    const int32_t cx = b[0] >> 6, cy = b[1] >> 6, cz = b[2] >> 6;
    if (cx != ck[0] || cy != ck[1] || cz != ck[2])
    {
      cp = lookup(cx, cy, cz);
      ck[0] = cx, ck[1] = cy, ck[2] = cz;
    }
    if (!cp) return false;
    const uint32_t lx = (uint32_t)b[0] & 63u, ly = (uint32_t)b[1] & 63u, lz = (uint32_t)b[2] & 63u;
    if (lx != 63u && ly != 63u && lz != 63u) // the cell lies in one chunk
    {
      const uint32_t *p = cp + (lx * (uint32_t)(STORE_CS * STORE_CS) + ly * (uint32_t)STORE_CS + lz);
#pragma unroll
      for (int j = 0; j < 4; ++j)
      {
        const ru32x2_a4 v = *reinterpret_cast<const ru32x2_a4 *>(p + ((j & 2) ? STORE_CS * STORE_CS : 0) + ((j & 1) ? STORE_CS : 0));
        raw[2 * j] = v.x;
        raw[2 * j + 1] = v.y;
      }
    }
    else
    {
      for (int j = 0; j < 4; ++j) // (not unrolled: one cell in 64 per axis comes here, up to two lookups per column)
      {
        const uint32_t xi = lx + (uint32_t)(j >> 1), yi = ly + (uint32_t)(j & 1);
        const int32_t kx = cx + (int32_t)(xi >> 6), ky = cy + (int32_t)(yi >> 6);
        const uint32_t off = (xi & 63u) * (uint32_t)(STORE_CS * STORE_CS) + (yi & 63u) * (uint32_t)STORE_CS;
        const uint32_t *p0 = chunk(kx, ky, cz);
        if (!p0) return false;
        if (lz != 63u)
        {
          const ru32x2_a4 v = *reinterpret_cast<const ru32x2_a4 *>(p0 + off + lz);
          raw[2 * j] = v.x;
          raw[2 * j + 1] = v.y;
        }
        else
        {
          const uint32_t *p1 = lookup(kx, ky, cz + 1);
          if (!p1) return false;
          raw[2 * j] = p0[off + 63u];
          raw[2 * j + 1] = p1[off];
        }
      }
    }
    return true;
  }
  __device__ __forceinline__ void load(const int32_t b[3], bool any_weight, RayCell &c)
  {
    uint32_t raw[8];
    c.valid = false;
    if (gather(b, raw)) ray_cell_fill(raw, any_weight, c);
  }
  // voxel v lies in the box, and the call lists chunks at all: entry(v) may be asked for
  __device__ __forceinline__ bool holds(const int32_t v[3]) const
  {
    bool ok = a.n_chunks != 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && v[k] >= a.lo[k] && v[k] <= a.hi[k];
    return ok;
  }
  // After load(b) at sample k left an invalid cell: the first k' > k whose cell can be valid, k + 1 if this field knows nothing.
  // Outside the live cell range [blo, bhi - 1]: all the axes b is outside on must have come in (gone() has seen to it that the ray
  // moves towards the range on each of them).  In an absent chunk: any axis must have left the chunk.
  __device__ __forceinline__ uint32_t resume(const RayWalk &w, const RayCommon &rc, const int32_t b[3], uint32_t k) const
  {
    uint32_t kn;
    if (outside)
    {
      kn = 0u;
#pragma unroll
      for (int x = 0; x < 3; ++x)
      {
        if (b[x] < a.blo[x]) kn = max(kn, w.first_voxel(rc, x, a.blo[x]));
        if (b[x] >= a.bhi[x]) kn = max(kn, w.first_voxel(rc, x, (int64_t)a.bhi[x] - 1));
      }
    }
    else if (!cp)
    {
      kn = 0xffffffffu;
#pragma unroll
      for (int x = 0; x < 3; ++x)
        if (w.sgn[x] != 0) kn = min(kn, w.first_voxel(rc, x, (int64_t)ck[x] * STORE_CS + (w.sgn[x] > 0 ? STORE_CS : -1))); // (up to 2^31)
    }
    else
      return k + 1u; // an unobserved corner, or a missing neighbour chunk: the next cell decides for itself
    return max(kn, k + 1u);
  }
  // the six neighbours lie in the box: c - 1 and c + 1 do on every axis
  __device__ __forceinline__ bool grad_inside(const int32_t c[3]) const
  {
    bool ok = a.n_chunks != 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && c[k] > a.lo[k] && c[k] < a.hi[k];
    return ok;
  }
  __device__ __forceinline__ bool entry(const int32_t v[3], uint32_t &raw) const
  {
    const uint32_t *p = lookup(v[0] >> 6, v[1] >> 6, v[2] >> 6);
    if (!p) return false;
    raw = p[((uint32_t)v[0] & 63u) * (uint32_t)(STORE_CS * STORE_CS) + ((uint32_t)v[1] & 63u) * (uint32_t)STORE_CS + ((uint32_t)v[2] & 63u)];
    return true;
  }
};

} // namespace ws
