// ws_surface.h — the per-voxel rules of the surface cloud (stated in include/warpsense_hip.h at ws_map_surface), shared by the cloud of
// a window (map_surface.hip) and the cloud of the chunk store (store_surface.hip): which voxel qualifies, what its record is and what
// the reference's marker holds for it.  Both files find their voxels in their own way and number the records with their own scans;
// everything that decides a byte of the output is here, once, and takes the entry as a value.
#pragma once

#include "ws_device.h"

namespace ws
{
// map.h:45: if (val.weight() <= 0 || abs(val.value()) >= tau) continue; -- abs on the value as int32, so -32768 never qualifies
__device__ __forceinline__ bool surf_pred(uint32_t raw, int32_t band) { return entry_weight(raw) > 0 && iabs32(entry_value(raw)) < band; }

// publish_local_map's point (map.h:51-53): (float)x * (float)map_resolution / 1000.f -- a rounded product, then a correctly
// rounded division (no contraction, no reciprocal: -ffp-contract=off and hipcc's default IEEE division)
__device__ __forceinline__ float surf_metres(int32_t v, float fres) { return (float)v * fres / 1000.f; }

// the record: x, y, z in world voxels, then the raw entry
__device__ __forceinline__ void surf_put_record(su32x4 *rec, unsigned long long o, int32_t x, int32_t y, int32_t z, uint32_t raw)
{
  const su32x4 r = {(uint32_t)x, (uint32_t)y, (uint32_t)z, raw};
  rec[o] = r;
}

// the marker: the point in metres (px, py: surf_metres of the column's x and y), then the colour
__device__ __forceinline__ void surf_put_marker(float *marker, unsigned long long o, float px, float py, int32_t z, uint32_t raw, float fres, float ftau)
{
  const int32_t val = entry_value(raw);
  float *m = marker + o * 7ull;
  m[0] = px;
  m[1] = py;
  m[2] = surf_metres(z, fres);
  // map.h:55-64: r = value / (float)tau, g = 0 for value >= 0, else r = 0, g = -value / (float)tau; b = 0, a = 1
  const float c = (float)(val >= 0 ? val : -val) / ftau;
  m[3] = val >= 0 ? c : 0.f;
  m[4] = val >= 0 ? 0.f : c;
  m[5] = 0.f;
  m[6] = 1.f;
}

} // namespace ws
