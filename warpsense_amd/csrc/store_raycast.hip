// store_raycast.hip — the ray cast of the chunk store (ws_store_raycast, include/warpsense_hip.h): the march of ws_raycast.h over the
// 64^3 chunks of the global map in device memory, wherever they lie.  The rules of a sample, a crossing, a record and the gradient are
// those of ws_raycast.h; what is new is the SPARSE field:
//
//   store_raycast_kernel        one lane per ray: the march, the crossing, the record
//   store_raycast_grad_kernel   one lane per ray: six voxels around the hit, six lookups
//
// A voxel is valid only if it lies in the box and in a present chunk.  The call lists the present chunks the box overlaps (the
// host's directory walk, before anything is launched), so "present" is "in the call's table" for every voxel of the box.  The LIVE
// box is the bounding box of the listed chunks cut to the box: a cell with a corner outside it is invalid, and inside it all 8
// corners lie in the box, so only the chunks decide.
//
// Chunk lookup: an open-addressing table key -> slot (ws_internal.h), one 16-byte load per probe.  A lane keeps the chunk of its
// base voxel (key and pointer) and looks a chunk up again only when the base voxel's chunk changes, or for the corners of a cell
// that straddles a chunk face (one cell in 64 per axis).  In a chunk z is fastest and a column is 64 aligned words: a z pair is one
// 8-byte load unless lz == 63.  Offsets into a chunk are below 2^18 and are added to a 64-bit pointer.
//
// What the march does not do, beyond ws_raycast.h:
//   * walk through nothing.  A cell's corner (0,0,0) is its base voxel: a sample whose base voxel lies in an absent chunk, or
//     outside the live box, has an invalid cell.  Each axis of p_k is monotone in k, so the next sample that can be valid is the
//     first one whose base voxel has left that chunk (the earliest exit over the axes) or has entered the live box (the latest
//     entry over the axes it is outside on).  RayWalk::first_voxel gives that sample exactly, in 64-bit arithmetic; the march
//     re-seeds quotient and remainder there.  -DWS_STORE_RAY_NO_JUMP turns this off, and only this.
//   * go on when nothing can follow: the ray ends once its base voxel has passed the live box on an axis it moves away on.
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
  __device__ __forceinline__ void load(const int32_t b[3], bool any_weight, RayCell &c)
  {
    c.valid = false;
    outside = b[0] < a.blo[0] || b[0] >= a.bhi[0] || b[1] < a.blo[1] || b[1] >= a.bhi[1] || b[2] < a.blo[2] || b[2] >= a.bhi[2];
    if (outside) return;
    const int32_t cx = b[0] >> 6, cy = b[1] >> 6, cz = b[2] >> 6;
    if (cx != ck[0] || cy != ck[1] || cz != ck[2])
    {
      cp = lookup(cx, cy, cz);
      ck[0] = cx, ck[1] = cy, ck[2] = cz;
    }
    if (!cp) return;
    const uint32_t lx = (uint32_t)b[0] & 63u, ly = (uint32_t)b[1] & 63u, lz = (uint32_t)b[2] & 63u;
    uint32_t raw[8];
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
        if (!p0) return;
        if (lz != 63u)
        {
          const ru32x2_a4 v = *reinterpret_cast<const ru32x2_a4 *>(p0 + off + lz);
          raw[2 * j] = v.x;
          raw[2 * j + 1] = v.y;
        }
        else
        {
          const uint32_t *p1 = lookup(kx, ky, cz + 1);
          if (!p1) return;
          raw[2 * j] = p0[off + 63u];
          raw[2 * j + 1] = p1[off];
        }
      }
    }
    ray_cell_fill(raw, any_weight, c);
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

__global__ __launch_bounds__(64) void store_raycast_kernel(StoreRayArgs a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  ri32x4 out = {0, 0, 0, -1};
  if (i < a.c.n) // (n <= the capacity of the record buffer: ws_store_raycast grows it first)
  {
    if (a.n_chunks != 0u)
    {
      StoreField fld(a);
      out = ray_march(a.c, fld, i);
    }
    a.c.rec[i] = out;
  }
  ray_count_hits(out, a.c.hits);
}

__global__ __launch_bounds__(64) void store_raycast_grad_kernel(StoreRayArgs a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.c.n) return;
  ray_gradient(a.c, StoreField(a), i);
}

// the table's upload, then the launch sequence
int launch_store_raycast(ws_store *st, ws_store::Ray &q, const StoreRayCall &c, const int32_t origin[3], const int32_t *dirs_dev, size_t n, int32_t max_range, uint32_t flags)
{
  StoreRayArgs a;
  a.c = ray_common(q, origin, dirs_dev, n, c.res, max_range, flags);
  for (int k = 0; k < 3; ++k) a.lo[k] = c.lo[k], a.hi[k] = c.hi[k], a.blo[k] = c.blo[k], a.bhi[k] = c.bhi[k];
  a.n_chunks = c.n_chunks;
  a.table = q.table_dev.as<StoreRaySlot>();
  a.mask = (uint32_t)store_ray_table_slots(c.n_chunks) - 1u;
  a.segs = st->seg_tab.as<uint32_t *>();
  a.seg_shift = st->seg_shift;
  hipStream_t s = st->ctx->stream;
  if (c.n_chunks)
    WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_ray_table_slots(c.n_chunks) * sizeof(StoreRaySlot), hipMemcpyHostToDevice, s));
  return ray_launch(q, s, a, store_raycast_kernel, store_raycast_grad_kernel);
}

} // namespace ws
