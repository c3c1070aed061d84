// ws_clearance.h — the rules of ws_map_clearance / ws_store_clearance (stated in include/warpsense_hip.h) once, as functions of values:
// for the kernels of map_clearance.hip, for the host-only entry points ws_clearance_centres and ws_clearance_margin, and for
// tests/cpp/clearance_units.hip, which runs them on the device against the host.  Integers only; every product and sum is int64.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

namespace ws
{
constexpr uint32_t CLEAR_MAX_SPHERES = 64;      // K: a sample's index is p * 64 + k
constexpr int32_t CLEAR_MAX_OFFSET = 1 << 20;   // |off_mm| of a sphere
constexpr int32_t CLEAR_MAX_LENGTH = 65535;     // radius_mm, soft_mm, P
constexpr int32_t CLEAR_NONE = 0x7fffffff;      // the margin of "no sample inside the box"
constexpr uint64_t CLEAR_NO_KEY = ~0ull;        // ... and its key: min_margin INT32_MAX, argmin 0xFFFFFFFF

struct ClearRecord // 32 bytes, one per trajectory
{
  int32_t min_margin, first_hit;
  uint32_t argmin, hits, outside, unknown;
  uint64_t cost;
};
static_assert(sizeof(ClearRecord) == 32, "the trajectory record of ws_map_clearance is 32 bytes");

struct ClearPose // 8 bytes, one per (trajectory, pose) under WS_CLEARANCE_POSES
{
  int32_t min_margin;
  uint16_t hits, outside;
};
static_assert(sizeof(ClearPose) == 8, "the pose record of ws_map_clearance is 8 bytes");

// floor(a / b), b > 0
__host__ __device__ inline int64_t clear_floor_div(int64_t a, int64_t b)
{
  const int64_t q = a / b;
  return q * b > a ? q - 1 : q;
}

// the exact floor square root of x < 2^36.  The float is an estimate and nothing more: the two loops make r the largest integer with
// r r <= x wherever it starts (it starts at most one off: a float carries 24 bits, r has 18)
__host__ __device__ inline uint32_t clear_isqrt(uint64_t x)
{
  uint64_t r = (uint64_t)__builtin_sqrtf((float)x);
  while (r * r > x) --r;
  while ((r + 1u) * (r + 1u) <= x) ++r;
  return (uint32_t)r;
}

// the centre of a sphere on axis a: pos_a + floor((sum_j rot[a][j] off_j + 2^29) / 2^30).  `pose`: rot_q30[9] row-major, pos_mm[3].
// Total over all int32 poses given a checked body: clearance_check limits |off| to 2^20 on the host (the body is always a host array), so
// |sum| <= 3 * 2^31 * 2^20 = 3 * 2^51 whatever the rotation holds.  Inside the stated domains of the pose the result fits int32
__host__ __device__ inline int64_t clear_centre(const int32_t pose[12], const int32_t off[3], int a)
{
  const int64_t s = (int64_t)pose[3 * a] * off[0] + (int64_t)pose[3 * a + 1] * off[1] + (int64_t)pose[3 * a + 2] * off[2];
  return (int64_t)pose[9 + a] + ((s + ((int64_t)1 << 29)) >> 30); // (an arithmetic shift is the floor division by 2^30)
}

// the voxel of a centre
__host__ __device__ inline int64_t clear_voxel(int64_t c, int32_t res) { return clear_floor_div(c, (int64_t)res); }

// the margin of a sample on a record with squared distance d2 (<= 65025) at resolution res (<= 1024): isqrt(d2 res^2) - radius
__host__ __device__ inline int32_t clear_margin(uint32_t d2, int32_t res, int32_t radius)
{
  return (int32_t)clear_isqrt((uint64_t)d2 * (uint64_t)((int64_t)res * res)) - radius;
}

// max(0, soft - margin)^2: below 2^34 (soft <= 65535, margin >= -65535)
__host__ __device__ inline uint64_t clear_penalty(int32_t margin, int32_t soft)
{
  const int64_t d = (int64_t)soft - margin;
  return d > 0 ? (uint64_t)(d * d) : 0ull;
}

// (margin, index) as one unsigned key whose minimum is the smallest margin and, among equals, the first sample
__host__ __device__ inline uint64_t clear_key(int32_t margin, uint32_t index) { return ((uint64_t)((uint32_t)margin ^ 0x80000000u) << 32) | index; }
// (spelled out: a library min() over two different 64-bit integer types may go through a type that drops the index)
__host__ __device__ inline uint64_t clear_min_key(uint64_t a, uint64_t b) { return b < a ? b : a; }
__host__ __device__ inline int32_t clear_key_margin(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }

// the box of a distance result as a sample meets it: the record index of voxel (x, y, z), or false OUTSIDE.  Under columns z is ignored
struct ClearBox
{
  int32_t lo[3];
  uint32_t ext[3];
  uint32_t columns;
};
__host__ __device__ inline bool clear_locate(const ClearBox &b, int64_t x, int64_t y, int64_t z, uint64_t *index)
{
  const int64_t u = x - b.lo[0], v = y - b.lo[1], w = b.columns ? 0 : z - b.lo[2];
  if (u < 0 || v < 0 || w < 0 || u >= (int64_t)b.ext[0] || v >= (int64_t)b.ext[1] || (!b.columns && w >= (int64_t)b.ext[2])) return false;
  const uint64_t col = (uint64_t)u * b.ext[1] + (uint64_t)v;
  *index = b.columns ? col : col * b.ext[2] + (uint64_t)w;
  return true;
}

// is (cost a, index a) the better pair?
__host__ __device__ inline bool clear_better(uint64_t cost_a, uint32_t idx_a, uint64_t cost_b, uint32_t idx_b)
{
  return cost_a < cost_b || (cost_a == cost_b && idx_a < idx_b);
}
} // namespace ws
