// ws_pack.h — the packed form of the store's chunks, stated in warpsense_hip.h (ws_store_pack): bricks, class codes, the header and
// the place of a brick's words in the payload.  The one statement of the format in code: the kernels (store_pack.hip), the host
// calls and the validation (api_pack.hip) all go through these helpers.  Integers only.
#pragma once

#include <cstdint>

#include "warpsense_hip.h"

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
constexpr uint32_t PACK_BRICKS = 512;      // bricks of a chunk: 8 x 8 x 8
constexpr uint32_t PACK_BRICK_WORDS = 512; // words of a brick: 8^3
constexpr uint32_t PACK_HDR = WS_PACK_HEADER_WORDS;
constexpr uint32_t PACK_HDR_KEY = 0, PACK_HDR_UNIFORM = 3, PACK_HDR_DENSE = 4, PACK_HDR_OFF_LO = 5, PACK_HDR_OFF_HI = 6, PACK_HDR_ZERO = 7, PACK_HDR_MAP = 8;
constexpr uint32_t PACK_DEFAULT = 0, PACK_UNIFORM = 1, PACK_DENSE = 2;

// brick number and word number inside the brick of the chunk word at (x, y, z), each 0 .. 63
__host__ __device__ inline uint32_t pack_brick_of(uint32_t x, uint32_t y, uint32_t z) { return ((x >> 3) * 8u + (y >> 3)) * 8u + (z >> 3); }
__host__ __device__ inline uint32_t pack_word_of(uint32_t x, uint32_t y, uint32_t z) { return (x & 7u) * 64u + (y & 7u) * 8u + (z & 7u); }
// the chunk index x*4096 + y*64 + z of word w of brick b
__host__ __device__ inline uint32_t pack_chunk_index(uint32_t b, uint32_t w)
{
  const uint32_t x = (b >> 6) * 8u + (w >> 6), y = ((b >> 3) & 7u) * 8u + ((w >> 3) & 7u), z = (b & 7u) * 8u + (w & 7u);
  return x * 4096u + y * 64u + z;
}

// the class of a brick from the two facts about its 512 words: one differs from fill, one differs from the brick's word 0
__host__ __device__ inline uint32_t pack_class(bool differs_from_fill, bool differs_from_word0)
{
  return !differs_from_fill ? PACK_DEFAULT : !differs_from_word0 ? PACK_UNIFORM : PACK_DENSE;
}
// payload words of a brick of class c
__host__ __device__ inline uint32_t pack_class_words(uint32_t c) { return c == PACK_UNIFORM ? 1u : c == PACK_DENSE ? PACK_BRICK_WORDS : 0u; }

// the class code of brick b in a header
__host__ __device__ inline uint32_t pack_map_code(const uint32_t *map /* the header from word 8 on */, uint32_t b) { return (map[b >> 4] >> (2u * (b & 15u))) & 3u; }
__host__ __device__ inline uint32_t pack_code(const uint32_t *header, uint32_t b) { return pack_map_code(header + PACK_HDR_MAP, b); }
__host__ __device__ inline void pack_set_code(uint32_t *header, uint32_t b, uint32_t c)
{
  uint32_t &w = header[PACK_HDR_MAP + (b >> 4)];
  w = (w & ~(3u << (2u * (b & 15u)))) | (c << (2u * (b & 15u)));
}
// payload words of the chunk of a header, and the index of its first one
__host__ __device__ inline uint64_t pack_chunk_words(const uint32_t *header) { return (uint64_t)header[PACK_HDR_UNIFORM] + (uint64_t)PACK_BRICK_WORDS * header[PACK_HDR_DENSE]; }
__host__ __device__ inline uint64_t pack_chunk_first(const uint32_t *header) { return (uint64_t)header[PACK_HDR_OFF_LO] | ((uint64_t)header[PACK_HDR_OFF_HI] << 32); }
__host__ __device__ inline void pack_set_first(uint32_t *header, uint64_t first)
{
  header[PACK_HDR_OFF_LO] = (uint32_t)first;
  header[PACK_HDR_OFF_HI] = (uint32_t)(first >> 32);
}

#ifdef __HIPCC__
// ---- the two scans of the kernels (store_pack.hip); tests/cpp/pack_units.hip runs them on the device on their own
constexpr uint32_t PACK_OFFSETS_WG = 256, PACK_SCAN_WG = 1024; // the workgroups the two functions below are written for

// The class map of a header into map[32] and the 512 brick offsets (payload words in front of a brick, inside its chunk) into
// off[512]; all 256 threads call it, and it ends with a barrier.  part[4]: scratch.
__device__ __forceinline__ void pack_brick_offsets(const uint32_t *header, uint32_t *map, uint32_t *off, uint32_t *part)
{
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  if (t < 32u) map[t] = header[PACK_HDR_MAP + t];
  __syncthreads();
  const uint32_t s0 = pack_class_words(pack_map_code(map, 2u * t)), s1 = pack_class_words(pack_map_code(map, 2u * t + 1u));
  uint32_t v = s0 + s1; // inclusive scan over the wave, then over the four waves
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1)
  {
    const uint32_t up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  if (lane == 63u) part[wave] = v;
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t w = 0; w < wave; ++w) before += part[w];
  off[2u * t] = before + v - s0 - s1;
  off[2u * t + 1u] = before + v - s1;
  __syncthreads();
}

__device__ __forceinline__ unsigned long long pack_wave_sum(unsigned long long v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The exclusive 64-bit scan of the chunks' payload words into the first-word fields of their n headers, in rounds of 1024 chunks;
// sums[3]: payload words, uniform bricks, dense bricks of all of them.  The 1024 threads of ONE workgroup call it.  wtot[16],
// red[2][16]: scratch in LDS.
__device__ __forceinline__ void pack_scan(uint32_t *headers, uint32_t n, unsigned long long *sums, unsigned long long *wtot, unsigned long long (*red)[PACK_SCAN_WG / 64])
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry = 0, n_uniform = 0, n_dense = 0;
  for (uint32_t base = 0; base < n; base += 1024u)
  {
    const uint32_t i = base + threadIdx.x; // (n < 2^31: no wrap)
    uint32_t *h = headers + (size_t)i * PACK_HDR;
    unsigned long long words = 0;
    if (i < n)
    {
      words = pack_chunk_words(h);
      n_uniform += h[PACK_HDR_UNIFORM], n_dense += h[PACK_HDR_DENSE];
    }
    unsigned long long v = words;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1)
    {
      const unsigned long long up = __shfl_up(v, o, 64);
      if (lane >= o) v += up;
    }
    if (lane == 63u) wtot[wave] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (uint32_t w = 0; w < 16u; ++w) before += w < wave ? wtot[w] : 0ull, all += wtot[w];
    if (i < n) pack_set_first(h, carry + before + v - words);
    carry += all;
    __syncthreads();
  }
  n_uniform = pack_wave_sum(n_uniform), n_dense = pack_wave_sum(n_dense);
  if (lane == 0u) red[0][wave] = n_uniform, red[1][wave] = n_dense;
  __syncthreads();
  if (threadIdx.x == 0u)
  {
    unsigned long long u = 0, d = 0;
    for (uint32_t w = 0; w < 16u; ++w) u += red[0][w], d += red[1][w];
    sums[0] = carry, sums[1] = u, sums[2] = d;
  }
}
#endif
} // namespace ws
