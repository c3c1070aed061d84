// ws_pack.h — the packed form of the store's chunks, stated in warpsense_hip.h (ws_store_pack): bricks, class codes, the header and
// the place of a brick's words in the payload.  The one statement of the format in code: the kernels (store_pack.hip), the host
// calls and the validation (api_pack.hip) all go through these helpers.  Integers only.
#pragma once

#include <cstdint>

#include "warpsense_hip.h"

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
} // namespace ws
