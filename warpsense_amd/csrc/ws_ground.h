// ws_ground.h — the rules of ws_map_ground / ws_store_ground and of the bridge to the distance field (stated in
// include/warpsense_hip.h): the levels of 64 voxels of a column from their class masks, the level a column keeps, the sub-voxel height,
// the record's word, the step between two heights and the class a ground record has in a column distance field.  Everything that
// decides a byte is here, as functions of values; map_ground.hip and store_ground.hip hold the walks that call them, api_query.hip and
// api_store_query.hip the host flow.
//
// A step of a column walk is 64 consecutive z voxels, bit b of a mask = voxel b of the step.  The walk goes DOWN the column and
// carries the masks of the step above: a level at bit 63 stands under bit 0 of that step, and headroom of up to 64 voxels above a
// voxel of this step ends in that step at the latest -- which is what bounds clear_vox by 64.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace ws
{
constexpr uint32_t GROUND_UNKNOWN = 0u, GROUND_GROUND = 1u, GROUND_BLOCKED = 2u, GROUND_VOID = 3u; // the class of a column
constexpr uint32_t GROUND_MAX_STEP = 65535u;

// the voxels of the step that starts at world z `base` which lie in [lo_z, hi_z]
__device__ __forceinline__ uint64_t ground_in_box(int64_t base, int64_t lo_z, int64_t hi_z)
{
  const int64_t b0 = lo_z > base ? lo_z - base : 0, b1 = hi_z < base + 63 ? hi_z - base : 63; // first and last bit
  if (b0 > 63 || b1 < 0 || b0 > b1) return 0ull;
  return (~0ull >> (63 - (b1 - b0))) << b0;
}

// where something can stand: an OCCUPIED voxel right under a FREE one (bit 63 under bit 0 of the step above)
__device__ __forceinline__ uint64_t ground_support(uint64_t occ, uint64_t fre, uint64_t fre_above) { return occ & ((fre >> 1) | (fre_above << 63)); }

// (hi : lo) >> n as 128 bits, 1 <= n <= 64
__device__ __forceinline__ void ground_shr(uint64_t &hi, uint64_t &lo, int32_t n)
{
  lo = n == 64 ? hi : (lo >> n) | (hi << (64 - n));
  hi = n == 64 ? 0ull : hi >> n;
}

// bit z: every one of the voxels z + 1 .. z + H is acceptable as headroom, 1 <= H <= 64.  acc: the acceptable voxels of this step,
// acc_above: those of the step above; whatever lies beyond the step above is never asked for.  A log-step AND: runs of 1, 2, 4 ..
// acceptable voxels upward from a bit, then the run of H out of two runs of the largest power of two that H holds.
__device__ __forceinline__ uint64_t ground_headroom(uint64_t acc, uint64_t acc_above, int32_t H)
{
  uint64_t hi = acc_above, lo = acc;
  int32_t len = 1;
  while (2 * len <= H)
  {
    uint64_t h2 = hi, l2 = lo;
    ground_shr(h2, l2, len);
    hi &= h2, lo &= l2;
    len *= 2;
  }
  if (len < H)
  {
    uint64_t h2 = hi, l2 = lo;
    ground_shr(h2, l2, H - len);
    hi &= h2, lo &= l2;
  }
  ground_shr(hi, lo, 1); // the run starts at z + 1
  return lo;
}

// the levels of a step: supported, and with headroom.  acc holds every FREE voxel (and the UNKNOWN ones of the box under
// WS_GROUND_UNKNOWN_HEADROOM); z + 1 itself must be FREE, which the support asks
__device__ __forceinline__ uint64_t ground_levels(uint64_t occ, uint64_t fre, uint64_t acc, uint64_t fre_above, uint64_t acc_above, int32_t H)
{
  return ground_support(occ, fre, fre_above) & ground_headroom(acc, acc_above, H);
}

// the level a step keeps out of its levels (!= 0): the lowest, under WS_GROUND_TOP the highest
__device__ __forceinline__ int32_t ground_pick(uint64_t levels, bool top) { return top ? 63 - __builtin_clzll(levels) : __builtin_ctzll(levels); }

// the zero crossing between v0 < 0 at z and v1 >= 0 at z + 1, in 1/256 voxel above z
__device__ __forceinline__ uint32_t ground_frac(int32_t v0, int32_t v1)
{
  const uint32_t f = (256u * (uint32_t)(-v0)) / (uint32_t)(v1 - v0); // -v0 <= 32768, v1 - v0 <= 65535
  return f < 255u ? f : 255u;
}

__device__ __forceinline__ int64_t ground_height(int32_t z, uint32_t w) { return (int64_t)z * 256 + (int64_t)(w & 0xffu); }
__device__ __forceinline__ uint32_t ground_class(uint32_t w) { return w >> 30; }
__device__ __forceinline__ uint32_t ground_step_of(uint32_t w) { return (w >> 8) & 0xffffu; }
__device__ __forceinline__ uint32_t ground_word(uint32_t frac, uint32_t step, uint32_t cls) { return frac | (step << 8) | (cls << 30); }

// the class of a column without a level
__device__ __forceinline__ uint32_t ground_no_level(bool any_occupied, bool any_free) { return any_occupied ? GROUND_BLOCKED : any_free ? GROUND_VOID : GROUND_UNKNOWN; }

// the step between two heights, as the record holds it
__device__ __forceinline__ uint32_t ground_step(int64_t h, int64_t hn)
{
  const uint64_t d = (uint64_t)(h > hn ? h - hn : hn - h);
  return d < (uint64_t)GROUND_MAX_STEP ? (uint32_t)d : GROUND_MAX_STEP;
}

// The class of a ground record in the column distance field of ws_*_ground_distance (those of dist_class): 1 FREE for GROUND with a
// step of at most max_step, 0 for UNKNOWN, else 2 OCCUPIED
__device__ __forceinline__ uint32_t ground_dist_class(uint32_t w, uint32_t max_step)
{
  const uint32_t cls = ground_class(w);
  return cls == GROUND_UNKNOWN ? 0u : (cls == GROUND_GROUND && ground_step_of(w) <= max_step) ? 1u : 2u;
}

// ---- what the two walks (map_ground.hip, store_ground.hip) share beside the rules
// the word a lane holds (the lane is wave-uniform): v0 and v1 come from the two lanes that hold them
__device__ __forceinline__ uint32_t ground_lane(uint32_t raw, int32_t at) { return (uint32_t)__builtin_amdgcn_readlane((int)raw, __builtin_amdgcn_readfirstlane(at)); }

// What a wave leaves of its column, and the workgroup's adds: the classes of the workgroup's four columns meet in LDS, thread c adds
// the columns of class c.  Every wave of the workgroup comes here, one without a column with active = false.
__device__ __forceinline__ void ground_publish(uint2 *lvl, unsigned long long *counts, bool active, uint64_t col, int32_t z, uint32_t word)
{
  __shared__ uint32_t wg_cls[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
  {
    wg_cls[wave] = active ? ground_class(word) : 4u;
    if (active) lvl[col] = make_uint2((uint32_t)z, word);
  }
  __syncthreads();
  if (threadIdx.x < 4)
  {
    uint32_t n = 0;
    for (int w = 0; w < 4; ++w) n += wg_cls[w] == threadIdx.x ? 1u : 0u;
    if (n) atomicAdd(&counts[threadIdx.x], (unsigned long long)n);
  }
}

} // namespace ws
