// ws_frontier.h — the per-voxel rules of the frontier (stated in include/warpsense_hip.h at ws_map_frontier), shared by the frontier of a
// window (map_frontier.hip) and the frontier of the chunk store (store_frontier.hip): the classes of a voxel, the bit of a neighbour
// and the record.  Both files find their voxels and their neighbours in their own way and number the records with their own scans;
// everything that decides a byte of a record is here, once, and takes the entry as a value.  The clustering works on the sorted
// records alone (frontier_clusters, map_frontier.hip) and serves both.
#pragma once

#include "ws_device.h"

namespace ws
{
// VALID iff weight > 0; with WS_FRONTIER_ANY_WEIGHT iff weight != 0 (dist_class, ws_device.h)
__device__ __forceinline__ bool fr_valid(uint32_t raw, bool any_weight)
{
  const int32_t w = entry_weight(raw);
  return any_weight ? w != 0 : w > 0;
}
// FREE iff valid and value >= min_value (0 <= min_value <= 32767: the value -32768 is never free); UNKNOWN iff not valid
__device__ __forceinline__ bool fr_free(uint32_t raw, bool any_weight, int32_t min_value) { return fr_valid(raw, any_weight) && entry_value(raw) >= min_value; }
__device__ __forceinline__ bool fr_unknown(uint32_t raw, bool any_weight) { return !fr_valid(raw, any_weight); }

// bit of the mask for an UNKNOWN neighbour one step along `axis`: -x +x -y +y -z +z are bits 0 .. 5
__device__ __forceinline__ uint32_t fr_bit(int axis, bool up) { return 1u << (2 * axis + (up ? 1 : 0)); }

// the record: x, y, z in world voxels, then the mask
__device__ __forceinline__ void fr_put_record(su32x4 *rec, unsigned long long o, int32_t x, int32_t y, int32_t z, uint32_t mask)
{
  const su32x4 r = {(uint32_t)x, (uint32_t)y, (uint32_t)z, mask};
  rec[o] = r;
}

} // namespace ws
