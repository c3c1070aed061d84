// ws_coarsen.h — the rule of ws_store_coarsen (stated in include/warpsense_hip.h): one coarse entry from the eight entries of the
// 2 x 2 x 2 voxels it covers.  Everything that decides a byte is here, as functions of integers that the host can run as well;
// store_coarsen.hip holds the kernel that calls them and api_store_pair.hip the plan.
#pragma once

#include "ws_device.h"

namespace ws
{
constexpr uint32_t COARSEN_WG = 256;    // four waves, one z column of a dst chunk per wave at a time
constexpr uint32_t COARSEN_TILES = 256; // workgroups per dst chunk: 16 x 16 tiles of 4 x 4 columns
constexpr uint32_t COARSEN_ROW = 12;    // words per row of the plan: dst slot, eight child slots (index cx * 4 + cy * 2 + cz), three unused
constexpr size_t COARSEN_MAX_CHUNKS = (size_t)1 << 23; // COARSEN_TILES workgroups each in one grid

// what the kernel is asked (all of it wave-uniform)
struct CoarsenArgs
{
  const uint32_t *rows;      // COARSEN_ROW words per listed chunk; an absent child is STORE_ABSENT
  uint32_t *const *src_segs; // base pointers of the segments of SRC, of DST
  uint32_t *const *dst_segs;
  uint32_t src_shift, dst_shift;
  uint32_t fill;             // fill_entry of DST (weight <= 0)
  int32_t min_observed;      // 1 .. 8
  unsigned long long *stats; // two sums: voxels that received a value, voxels with 1 <= n < min_observed; nullptr: not counted
};

// n, S and W of the observed children seen so far; W starts at INT32_MAX
struct CoarsenAcc
{
  int32_t n = 0, S = 0, W = INT32_MAX;
};

__host__ __device__ __forceinline__ void coarsen_add(CoarsenAcc &a, uint32_t raw)
{
  const int32_t v = (int32_t)(int16_t)(raw & 0xffffu), w = (int32_t)(int16_t)(raw >> 16);
  const bool observed = w > 0;
  a.n += observed ? 1 : 0;
  a.S += observed ? v : 0;
  a.W = observed && w < a.W ? w : a.W;
}

// ceil(2^32 / n) for n = 2 .. 8
__host__ __device__ constexpr uint32_t coarsen_magic(uint32_t n) { return (uint32_t)(((1ull << 32) + n - 1) / n); }

// floor(S / n) toward minus infinity for 1 <= n <= 8 and |S| <= 2^18 (eight int16 values).  u = S + 2^18 n lies in [0, 2^22) and
// floor(S / n) = floor(u / n) - 2^18.  floor(u / n) is the high word of u M with M = ceil(2^32 / n): the error M n - 2^32 < n <= 8
// gives u (M n - 2^32) < 2^25 < 2^32, so the quotient is exact; n = 1 has no 32-bit M and needs none.
__host__ __device__ __forceinline__ int32_t coarsen_div(int32_t S, int32_t n)
{
  const uint32_t u = (uint32_t)(S + (1 << 18) * n);
  uint32_t M = 0;
#pragma unroll
  for (uint32_t k = 2; k <= 8; ++k) M = (uint32_t)n == k ? coarsen_magic(k) : M;
  const uint32_t q = n == 1 ? u : (uint32_t)(((uint64_t)u * M) >> 32);
  return (int32_t)q - (1 << 18);
}

// the coarse entry: pack(floor(S / n), W) with n >= min_observed children observed, else `fill`
__host__ __device__ __forceinline__ uint32_t coarsen_entry(const CoarsenAcc &a, int32_t min_observed, uint32_t fill)
{
  if (a.n < min_observed) return fill; // (min_observed >= 1: n = 0 is fill)
  return ((uint32_t)coarsen_div(a.S, a.n) & 0xffffu) | ((uint32_t)a.W << 16);
}

// store_coarsen.hip: one launch over `n_chunks` rows of a.rows; it adds into a.stats, which the caller has cleared
int launch_store_coarsen(hipStream_t s, const CoarsenArgs &a, size_t n_chunks);

} // namespace ws
