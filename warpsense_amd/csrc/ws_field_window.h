// ws_field_window.h — the window of a device map as the FIELD of ws_raycast.h: the ring addressing and the z-pair loads.  Shared by the
// ray cast (map_raycast.hip) and the point sample (map_sample.hip) of a window.
#pragma once

#include "ws_raycast.h"

namespace ws
{
struct RayArgs
{
  const uint32_t *data;
  MapParams mp;
  int32_t wlo[3], whi[3]; // the window in world voxels, inclusive
  RayCommon c;
};

// the window as the field of ws_raycast.h
struct WindowField
{
  static constexpr bool JUMPS = false;
  const RayArgs &a;
  __device__ __forceinline__ explicit WindowField(const RayArgs &args) : a(args) {}
  // beyond the window for good (b is monotone along sgn): nothing valid can follow
  __device__ __forceinline__ bool gone(const int32_t b[3], const int32_t sgn[3]) const
  {
    bool g = false;
#pragma unroll
    for (int x = 0; x < 3; ++x) g = g || (sgn[x] >= 0 && b[x] >= a.whi[x]) || (sgn[x] <= 0 && b[x] < a.wlo[x]);
    return g;
  }
  __device__ __forceinline__ uint32_t resume(const RayWalk &, const RayCommon &, const int32_t *, uint32_t k) const { return k + 1u; }
  // the raw entries of the 8 corners of the cell with base voxel b, index cx * 4 + cy * 2 + cz; false (raw untouched) if a corner is
  // outside the window
  __device__ __forceinline__ bool gather(const int32_t b[3], uint32_t raw[8]) const
  {
    if (b[0] < a.wlo[0] || b[0] >= a.whi[0] || b[1] < a.wlo[1] || b[1] >= a.whi[1] || b[2] < a.wlo[2] || b[2] >= a.whi[2]) return false;
    const int32_t sx = a.mp.size[0], sy = a.mp.size[1], sz = a.mp.size[2];
    const int32_t x0 = ring(b[0] - a.mp.pos[0] + a.mp.offset[0] + sx, sx), y0 = ring(b[1] - a.mp.pos[1] + a.mp.offset[1] + sy, sy);
    const int32_t z0 = ring(b[2] - a.mp.pos[2] + a.mp.offset[2] + sz, sz);
    const int32_t x1 = x0 + 1 == sx ? 0 : x0 + 1, y1 = y0 + 1 == sy ? 0 : y0 + 1;
    const bool seam = z0 + 1 == sz;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const int32_t xi = (j & 2) ? x1 : x0, yi = (j & 1) ? y1 : y0;
      const int64_t col = (int64_t)(xi * sy + yi) * (int64_t)sz; // size[0] * size[1] < 2^31 (ws_map_create)
      if (!seam)
      {
        const ru32x2_a4 p = *reinterpret_cast<const ru32x2_a4 *>(a.data + col + z0);
        raw[2 * j] = p.x;
        raw[2 * j + 1] = p.y;
      }
      else
      {
        raw[2 * j] = a.data[col + z0];
        raw[2 * j + 1] = a.data[col];
      }
    }
    return true;
  }
  // the 8 corners of the cell with base voxel b; invalid (values untouched) if a corner is outside the window or unobserved
  __device__ __forceinline__ void load(const int32_t b[3], bool any_weight, RayCell &c) const
  {
    uint32_t raw[8];
    c.valid = false;
    if (gather(b, raw)) ray_cell_fill(raw, any_weight, c);
  }
  // voxel v lies in the field: entry(v) may be asked for
  __device__ __forceinline__ bool holds(const int32_t v[3]) const
  {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && v[k] >= a.wlo[k] && v[k] <= a.whi[k];
    return ok;
  }
  // the six neighbours lie in the window: c - 1 and c + 1 do on every axis
  __device__ __forceinline__ bool grad_inside(const int32_t c[3]) const
  {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && c[k] > a.wlo[k] && c[k] < a.whi[k];
    return ok;
  }
  __device__ __forceinline__ bool entry(const int32_t v[3], uint32_t &raw) const
  {
    raw = a.data[get_index(a.mp, v[0], v[1], v[2])];
    return true;
  }
};

} // namespace ws
