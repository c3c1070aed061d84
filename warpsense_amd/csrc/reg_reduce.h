// reg_reduce.h — the exact integer sums of the registration kernels (gfx950), first of their four layers (reg_reduce.h, reg_gn.h,
// reg_points.h, reg_exchange.h): the grid shape, the 29 reduced terms and the reference's 44 words, the transposing wave reduction
// and the sums over a workgroup's waves and over the partials of a launch.
#pragma once

#include "ws_device.h"

namespace ws
{
#ifndef WS_REG_BLOCKS
#define WS_REG_BLOCKS 256
#endif
constexpr int REG_BLOCKS = WS_REG_BLOCKS; // one workgroup per CU
#ifndef WS_REG_THREADS
#define WS_REG_THREADS 512
#endif
constexpr int REG_THREADS = WS_REG_THREADS; // 8 waves: one point per lane for a 131 072-point scan (4 waves x 2 points: 10.7 vs 10.1 us)
constexpr int REG_TERMS = 29;    // 21 h + 6 g + e + c (slots 29..31 are padding)
static_assert(REG_TERMS <= 32, "slots");
constexpr int REG_SLOTS = 32;    // padded to a power of two for the transposing reduction
static_assert(REG_BLOCKS % (REG_THREADS / 64 * 2) == 0, "sum_partials: every wave sums an equal share of the workgroups, 2 lanes per slot");

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int mask)
{
  int lo = __shfl_xor((int)(uint32_t)((uint64_t)v & 0xffffffffull), mask, 64);
  int hi = __shfl_xor((int)(uint32_t)((uint64_t)v >> 32), mask, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// ---- transposing wave reduction of 32 int64 values, without the LDS crossbar -------------------------
// Stage `BIT` pairs lane l with lane l ^ BIT: lanes whose BIT is clear keep the lower HALF of the values they
// still carry and receive the partner's lower half, the others keep / receive the upper half, so every stage
// halves the values per lane: 16+8+4+2+1+1 = 32 exchanges for 32 values instead of 32 x 6.
//   BIT 32, 16: gfx950's v_permlane32_swap / v_permlane16_swap exchange exactly those halves of two registers
//               (no select, no address): one VALU instruction per 32-bit register pair;
//   BIT 8 .. 1: DPP lane permutations (row_ror:8, row_half_mirror + quad_perm, quad_perm).
__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src_lane)
{
  const int lo = __shfl((int)(uint32_t)((uint64_t)v & 0xffffffffull), src_lane, 64), hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src_lane, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t pack64(int lo, int hi) { return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo); }

template <int BIT>
__device__ __forceinline__ void swap_add_stage(int64_t &a, const int64_t b)
{
  // a: the value kept by lanes with BIT clear, b: kept by lanes with BIT set; result in a (for every lane: its kept slot)
  const int alo = (int)(uint32_t)((uint64_t)a & 0xffffffffull), ahi = (int)(uint32_t)((uint64_t)a >> 32);
  const int blo = (int)(uint32_t)((uint64_t)b & 0xffffffffull), bhi = (int)(uint32_t)((uint64_t)b >> 32);
  if constexpr (BIT == 32)
  {
    const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    a = wadd64(pack64(lo[0], hi[0]), pack64(lo[1], hi[1]));
  }
  else
  {
    const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    a = wadd64(pack64(lo[0], hi[0]), pack64(lo[1], hi[1]));
  }
}

template <int BIT>
__device__ __forceinline__ int dpp_xor(int v)
{
  if constexpr (BIT == 8) return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false); // row_ror:8
  if constexpr (BIT == 4)
  {
    const int m = __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false); // row_half_mirror: lane ^ 7
    return __builtin_amdgcn_update_dpp(0, m, 0x1b, 0xf, 0xf, false);         // quad_perm [3,2,1,0]: lane ^ 3
  }
  if constexpr (BIT == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4e, 0xf, 0xf, false); // quad_perm [2,3,0,1]
  return __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, false);                         // quad_perm [1,0,3,2]
}
template <int BIT>
__device__ __forceinline__ int64_t dpp_xor_i64(int64_t v)
{
  return pack64(dpp_xor<BIT>((int)(uint32_t)((uint64_t)v & 0xffffffffull)), dpp_xor<BIT>((int)(uint32_t)((uint64_t)v >> 32)));
}

// One pair of a transposing stage inside a 16-lane row (BIT 8 or 4): lanes without the bit end up with a + a(partner),
// lanes with it with b + b(partner), both in `a`.  Four DPP adds whose bank masks pick the two halves -- the partner comes
// over the DPP operand of the add itself (row_shl for the lower lanes, row_shr for the upper ones) -- instead of four
// selects, two to four DPP moves and two adds.  (s_nop: a VGPR written by the instruction before must not be read over DPP
// at once, and the compiler does not see what the asm reads.)
template <int BIT>
__device__ __forceinline__ void dpp_pair_add(int64_t &a, const int64_t b)
{
  static_assert(BIT == 8 || BIT == 4, "row-internal stages");
  uint32_t alo = (uint32_t)((uint64_t)a & 0xffffffffull), ahi = (uint32_t)((uint64_t)a >> 32);
  const uint32_t blo = (uint32_t)((uint64_t)b & 0xffffffffull), bhi = (uint32_t)((uint64_t)b >> 32);
  if constexpr (BIT == 8)
    asm volatile("s_nop 1\n\t"
                 "v_add_co_u32_dpp %0, vcc, %0, %0 row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_addc_co_u32_dpp %1, vcc, %1, %1, vcc row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_co_u32_dpp %0, vcc, %2, %2 row_shr:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_addc_co_u32_dpp %1, vcc, %3, %3, vcc row_shr:8 row_mask:0xf bank_mask:0xc"
                 : "+v"(alo), "+v"(ahi)
                 : "v"(blo), "v"(bhi)
                 : "vcc");
  else
    asm volatile("s_nop 1\n\t"
                 "v_add_co_u32_dpp %0, vcc, %0, %0 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_addc_co_u32_dpp %1, vcc, %1, %1, vcc row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_co_u32_dpp %0, vcc, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
                 "v_addc_co_u32_dpp %1, vcc, %3, %3, vcc row_shr:4 row_mask:0xf bank_mask:0xa"
                 : "+v"(alo), "+v"(ahi)
                 : "v"(blo), "v"(bhi)
                 : "vcc");
  a = (int64_t)(((uint64_t)ahi << 32) | alo);
}

template <int HALF, int BIT>
__device__ __forceinline__ void reduce_stage(int64_t (&v)[REG_SLOTS], int lane)
{
  if constexpr (BIT >= 16)
  {
#pragma unroll
    for (int i = 0; i < HALF; ++i) swap_add_stage<BIT>(v[i], v[i + HALF]);
  }
  else if constexpr (BIT >= 4)
  {
#pragma unroll
    for (int i = 0; i < HALF; ++i) dpp_pair_add<BIT>(v[i], v[i + HALF]);
  }
  else
  {
    const bool upper = (lane & BIT) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i)
    {
      const int64_t send = upper ? v[i] : v[i + HALF];
      const int64_t keep = upper ? v[i + HALF] : v[i];
      v[i] = wadd64(keep, dpp_xor_i64<BIT>(send));
    }
  }
}

// wave totals of REG_SLOTS per-lane values -> wave_part[wave][0..31] (valid after the trailing barrier)
__device__ __forceinline__ void wave_reduce32(int64_t (&v)[REG_SLOTS], int64_t (*wave_part)[REG_SLOTS])
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  reduce_stage<16, 32>(v, lane);
  reduce_stage<8, 16>(v, lane);
  reduce_stage<4, 8>(v, lane);
  reduce_stage<2, 4>(v, lane);
  reduce_stage<1, 2>(v, lane);
  v[0] = wadd64(v[0], dpp_xor_i64<1>(v[0]));
  // lane l now holds the wave total of slot (l >> 1)
  if ((lane & 1) == 0) wave_part[wave][lane >> 1] = v[0];
  __syncthreads();
}

// The same with the eight wave totals of a slot ADDED into wg_sum[slot] (LDS atomics, zero before) instead of laid side by
// side: the first wave then reads one value per slot instead of eight (valid after the trailing barrier).
// (the caller's barrier follows: a wave without points skips this call, not the barrier)
__device__ __forceinline__ void wave_reduce32_add(int64_t (&v)[REG_SLOTS], unsigned long long *wg_sum)
{
  const int lane = threadIdx.x & 63;
  reduce_stage<16, 32>(v, lane);
  reduce_stage<8, 16>(v, lane);
  reduce_stage<4, 8>(v, lane);
  reduce_stage<2, 4>(v, lane);
  reduce_stage<1, 2>(v, lane);
  v[0] = wadd64(v[0], dpp_xor_i64<1>(v[0]));
  if ((lane & 1) == 0) atomicAdd(&wg_sum[lane >> 1], (unsigned long long)v[0]);
}

// Sum REG_SLOTS per-lane values over the whole workgroup. Result: red[0..31] in LDS (valid after the
// trailing barrier).
__device__ __forceinline__ void block_reduce32(int64_t (&v)[REG_SLOTS], int64_t (*wave_part)[REG_SLOTS], int64_t *red)
{
  wave_reduce32(v, wave_part);
  if (threadIdx.x < REG_SLOTS)
  {
    int64_t s = 0;
#pragma unroll
    for (int w = 0; w < REG_THREADS / 64; ++w) s = wadd64(s, wave_part[w][threadIdx.x]);
    red[threadIdx.x] = s;
  }
  __syncthreads();
}

// block_reduce32 for a workgroup of WAVES waves
template <int WAVES>
__device__ __forceinline__ void block_reduce32(int64_t (&v)[REG_SLOTS], int64_t (*wave_part)[REG_SLOTS], int64_t *red)
{
  wave_reduce32(v, wave_part);
  if (threadIdx.x < REG_SLOTS)
  {
    int64_t s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s = wadd64(s, wave_part[w][threadIdx.x]);
    red[threadIdx.x] = s;
  }
  __syncthreads();
}

// row-major upper triangle index of (i <= j)
__host__ __device__ constexpr int tri_index(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

// The reference's 44 words -- h 6x6 column-major (math/matrix6x6.h:112-115), g[6], e, c -- and the slot of the 29 reduced terms
// word k is made from.  e and c are `int` in the reference (registration.cu:16-21): words 42 and 43 are their slot's low 32 bits,
// sign-extended (word_value).  h_slot: element (r, c) of the symmetric h, word 6 c + r, for callers that index h at run time.
__host__ __device__ constexpr int h_slot(int r, int c) { return r <= c ? tri_index(r, c) : tri_index(c, r); }
__host__ __device__ constexpr int word_slot(int k) { return k < 36 ? h_slot(k % 6, k / 6) : k < 42 ? 21 + (k - 36) : 27 + (k - 42); }
__device__ __forceinline__ int64_t word_value(int k, int64_t slot_value) { return k < 42 ? slot_value : (int64_t)(int32_t)slot_value; }

// 29 reduced terms -> the reference's 44 words
__device__ __forceinline__ void expand_sums(const int64_t *terms, int64_t *sums)
{
#pragma unroll
  for (int k = 0; k < 44; ++k) sums[k] = word_value(k, terms[word_slot(k)]);
}

// Sum of the partials [REG_BLOCKS][REG_SLOTS] a previous launch left in HBM -> red[0..31] in LDS.
// Lane l of wave w adds slot (l >> 1) over 32 of the wave's 64 workgroups: 32 independent, fully coalesced
// loads per lane (one memory latency), one shuffle, one LDS hop.
// COHERENT: the partials were written by other workgroups of the SAME launch -> agent-scope loads (sc1), which
// cannot be served from a stale line of this XCD's L2.
template <bool COHERENT = false>
__device__ __forceinline__ void sum_partials(const int64_t *pp, int64_t (*wave_part)[REG_SLOTS], int64_t *red)
{
  constexpr int WAVES = REG_THREADS / 64;
  constexpr int PER_LANE = REG_BLOCKS / (WAVES * 2); // workgroups summed by one lane
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane >> 1;
  const int64_t *base = pp + ((size_t)wave * (2 * PER_LANE) + (size_t)(lane & 1) * PER_LANE) * REG_SLOTS + slot;
  int64_t s = 0;
#pragma unroll
  for (int i = 0; i < PER_LANE; ++i)
  {
    const int64_t v = COHERENT ? __hip_atomic_load(const_cast<int64_t *>(&base[(size_t)i * REG_SLOTS]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                               : base[(size_t)i * REG_SLOTS];
    s = wadd64(s, v);
  }
  s = wadd64(s, shfl_xor_i64(s, 1));
  if ((lane & 1) == 0) wave_part[wave][slot] = s;
  __syncthreads();
  if (threadIdx.x < REG_SLOTS)
  {
    int64_t t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t = wadd64(t, wave_part[w][threadIdx.x]);
    red[threadIdx.x] = t;
  }
  __syncthreads();
}

} // namespace ws
