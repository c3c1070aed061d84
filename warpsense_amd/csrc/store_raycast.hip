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
#include "ws_field_store.h"

namespace ws
{
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
