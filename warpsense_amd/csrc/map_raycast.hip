// map_raycast.hip — ray cast of a device map (gfx950): the range image the sensor would see from a pose, with the hit points and,
// on request, the TSDF gradient at them.  The rules are stated in warpsense_hip.h at ws_map_raycast; ws_raycast.h walks them exactly,
// shortened only where the records provably stay the same, and this file gives it the window: the ring addressing, the z-pair loads:
//
//   raycast_kernel     one lane per ray: the march, the crossing, the record
//   raycast_grad_kernel  one lane per ray: six voxels around the hit
//
// What the march does not do per sample:
//   * divide.  p_k = o + trunc(d k step / L) per axis is carried as quotient and remainder of |d| step k by L: adding the
//     quotient and remainder of |d| step by L and one conditional carry gives the next sample exactly (|d| <= L, so the
//     quotient is at most k step <= max_range and the remainder stays below L < 2^31; all of it 32-bit).  trunc is odd, so the sign
//     of d goes on afterwards.  The base voxel floor((p - h) / res) is a multiply-shift (FastDiv, prepared on the host).
//   * gather a cell twice.  step = res / 2: the base voxel often stays; the 8 corner values and the cell's validity are kept
//     while it does.
//   * evaluate T where its sign is known.  The weights are >= 0 and sum to res^3 > 0: 8 positive corners give T > 0, 8
//     corners <= 0 give T <= 0.  Only a mixed cell is interpolated.  At a crossing both T are computed in full (T_{k-1} from a
//     fresh gather of its cell: once per ray).
//   * go on when nothing can follow.  Each axis of p_k is monotone in k, so the base voxel is too: once it has passed the last
//     cell of the window along an axis it moves away on (or stands still beside it), every later cell is invalid and no later
//     sample can be part of a hit.  The ray ends there, and at its hit.
//
// The corners are 4 pairs of z neighbours; a pair is one 8-byte load unless the ring's seam in z lies between the two.
// Plain launches on the context's stream; the output is indexed by ray: no compaction.  The one atomic is the hit counter
// (an integer sum, one add per wave).
#include "ws_field_window.h"

namespace ws
{
__global__ __launch_bounds__(64) void raycast_kernel(RayArgs a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  ri32x4 out = {0, 0, 0, -1};
  if (i < a.c.n)
  {
    WindowField fld(a);
    out = ray_march(a.c, fld, i);
    a.c.rec[i] = out;
  }
  ray_count_hits(out, a.c.hits);
}

__global__ __launch_bounds__(64) void raycast_grad_kernel(RayArgs a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.c.n) return;
  ray_gradient(a.c, WindowField(a), i);
}

int launch_raycast(ws_map *m, RayResult &q, int which, const int32_t origin[3], const int32_t *dirs_dev, size_t n, int32_t max_range, uint32_t flags)
{
  RayArgs a;
  a.data = m->data[which].as<uint32_t>();
  a.mp = m->par[which];
  for (int k = 0; k < 3; ++k)
  {
    a.wlo[k] = a.mp.pos[k] - a.mp.size[k] / 2;
    a.whi[k] = a.wlo[k] + a.mp.size[k] - 1;
  }
  a.c = ray_common(q, origin, dirs_dev, n, m->res, max_range, flags);
  return ray_launch(q, m->ctx->stream, a, raycast_kernel, raycast_grad_kernel);
}

} // namespace ws
