// tsdf_scatter.h — what every stage of the TSDF scatter (gfx950) shares, first layer: the arguments of its kernels, the switches more
// than one stage or the host reads, error bits, the addressing of voxels, tiles and records, and the stages' launchers as
// tsdf_update.hip calls them.  (The survey of the stages is at the head of tsdf_update.hip.)
#pragma once

#include "ws_march.h"
#include "ws_dda.h"

namespace ws
{
struct ScatterArgs
{
  const int32_t *xyz;
  int32_t *xyz_keep; // the set-up pass copies the scan here (ws_map::scan_dev: what a repeat of an aborted scan reads); NULL: xyz is that buffer
  uint32_t n;
  int32_t scanner_pos[3];
  int32_t up[3];
  MapParams map; // new_map's parameters (the reference indexes new_map in the scatter, update_tsdf.cu:55-125)
  int32_t tau;
  int32_t res;
  int32_t ntx, nty, ntz;
  int32_t all_keyed;     // new_map is not (tau, 0): every candidate goes through the order keys, no free-space pass
  int32_t keyed_len_neg; // smallest ray length with off-ray (negative-weight) candidates
  int32_t keyed_slack;   // see ray_setup_kernel
  RaySetup *rays;
  uint32_t *az_hist;   // [AZ_BINS + 1] rays per direction bin (last bin: rays that contribute nothing)
  uint32_t *az_off;    // [AZ_BINS]: number of rays that contribute (written by the direction sort)
  uint2 *ray_bin;      // [n] (direction bin, rank inside the bin) of every ray: set-up blocks -> sort blocks of the same launch
  uint32_t *ray_order; // ray indices sorted by direction bin
  const int32_t *fan_steps; // [256], see tail_bound
  uint8_t *vstate;     // two planes of one byte per voxel: VOX_* / off-ray free-space mark
  uint8_t *tile_dirty; // one byte per tile: touched by the free-space pass
  uint32_t *tile_nsub;  // [tiles] sub-chunks (entries) of the tile
  uint32_t *tile_ent;   // [tiles][TILE_DIRECT] entries: sub-chunk id << 5 | records - 1
  TileEntry *tile_list; // the tiles with records (the first entries of a tile append it; the resolve deals them out evenly)
  unsigned long long *rec; // the pool: sub-chunks of SUB_RECS records
  uint32_t sub_cap;
  uint32_t scan_seq;  // sequence number of this scatter
  unsigned long long *big_keys; // (tile, entry number) -> entry + 1 beyond TILE_DIRECT: keys, then uint32 values (big_mask + 1 slots)
  uint32_t big_mask;
  uint32_t rec_fmt;   // the scan's split of the record's key bits: S | F << 8 (rec_format, ws_internal.h)
  uint32_t *tail_stats; // records / (flush, tile) groups per workgroup of the tail march
  TsdfCounters *counters;
  uint32_t *status; // host-mapped: [0] sticky error bits, [4..5] record bound of the scan in flight, [6] its sequence number, [8] / [9] see ws_map::status_host
};
// 264 bytes of kernel arguments instead of 256 cost reg_loop_kernel 30 % (reg_loop.hip); the same bound here
static_assert(sizeof(ScatterArgs) <= 256, "ScatterArgs: more than 256 bytes of kernel arguments");

#define REC_S(a) ((int32_t)((a).rec_fmt & 0xffu))
#define REC_F(a) ((int32_t)((a).rec_fmt >> 8))
constexpr uint8_t VOX_KEYED = 1, VOX_TOUCHED = 2;
constexpr uint8_t VOX_NEGFREE = 8; // the resolve's merged view of the second byte plane (stored there as 1)
constexpr uint32_t ERR_RANGE = 2, ERR_FREE_BOUND = 4, ERR_INTERNAL = 8;

#ifndef WS_TAIL_SPLIT
#define WS_TAIL_SPLIT (8 / WS_TAIL_WAVES) // workgroups that share the tails of one group of 64 rays: eight parts in all
#endif
#ifndef WS_FREE_THREADS
#define WS_FREE_THREADS 256 // threads per workgroup of the free pass
#endif
#ifndef WS_FREE_FIRST
#define WS_FREE_FIRST 32 // sub-chunks every wave of the free pass owns from the start (see pool_grab; 16: 136 us, 32: 121, 64: 120)
#endif
#ifndef WS_SORT_BLOCKS
#define WS_SORT_BLOCKS 128 // (64 / 128 / 256 / 512 blocks: set-up + sort 29.0 / 28.0 / 29.1 / 34 us)
#endif
#ifndef WS_SORT_RINGS
#define WS_SORT_RINGS 16 // (tail march at 4 / 8 / 16 / 32 / 64 rings: 146 / 146 / 146 / 154 / 152 us, set-up pass 36 / 31 / 28 / 30 / 28)
#endif
static_assert(AZ_BINS == 2 * 4096, "WS_SORT_RINGS rings x 4096 / WS_SORT_RINGS sectors, above / below the sensor");

__device__ __forceinline__ void raise_error(TsdfCounters *c, uint32_t *status, uint32_t bits)
{
  atomicOr(&c->error, bits);
  __hip_atomic_fetch_or(status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); // sticky, host visible
}

__device__ __forceinline__ uint32_t tile_of(int32_t nty, int32_t ntz, int32_t sx, int32_t sy, int32_t sz)
{
  // ntx * nty < 2^24 (checked by ws_map_create): full-rate 24-bit multiplies
  const uint32_t col = __umul24((uint32_t)(sx >> TILE_XB), (uint32_t)nty) + (uint32_t)(sy >> TILE_YB);
  return __umul24(col, (uint32_t)ntz) + (uint32_t)(sz >> TILE_ZB);
}
// The voxel inside its tile, twice, straight from the storage coordinates: `local` = lx | ly | lz, z fastest -- what a record
// carries and the resolve's LDS arrays are indexed by (a column's 64 z spread over all banks; round 6 measured records in brick
// order: the resolve 107 -> 116 us, a wall's records then fall on 8 banks) -- and `vox` = vbrick(local), its byte in the tile's
// kilobyte of voxel bytes (ws_internal.h).
static_assert(TILE_XB == 2 && TILE_YB == 2 && TILE_ZB == 6, "vox_of / vbrick: 4 x 4 x 8 bricks of a 4 x 4 x 64 tile");
__device__ __forceinline__ uint32_t vox_of(int32_t sx, int32_t sy, int32_t sz)
{
  const uint32_t xy = (((uint32_t)sx & 3u) << 2) | ((uint32_t)sy & 3u);
  return (((uint32_t)sz & 0x38u) << 4) | (xy << 3) | ((uint32_t)sz & 7u);
}
__device__ __forceinline__ uint32_t local_of(int32_t sx, int32_t sy, int32_t sz)
{
  const uint32_t xy = (((uint32_t)sx & 3u) << 2) | ((uint32_t)sy & 3u);
  return (xy << TILE_ZB) | ((uint32_t)sz & 63u);
}
// vbrick backwards (the rare free-space candidate that becomes a record)
__device__ __forceinline__ uint32_t local_of_vox(uint32_t vox) { return ((vox & 0x78u) << 3) | ((vox >> 4) & 0x38u) | (vox & 7u); }
// Byte `vox` of tile `tile` in a plane of voxel bytes / record place `pos` of sub-chunk `id`.  SMALL: the planes and the pool are
// below 4 GB (every map up to 1025^3; decided per launch): the offset is ONE 32-bit instruction next to a base address in scalar
// registers, instead of a 64-bit shift and two 64-bit additions per access -- the marches are bound by vector-instruction issue.
template <bool SMALL>
__device__ __forceinline__ uint8_t *vox_ptr(uint8_t *plane, uint32_t tile, uint32_t vox)
{
  if (SMALL) return plane + (uint32_t)((tile << 10) | vox);
  return plane + (((size_t)tile << 10) | vox);
}
template <bool SMALL>
__device__ __forceinline__ unsigned long long *rec_ptr(unsigned long long *pool, uint32_t id, uint32_t pos)
{
  if (SMALL) return reinterpret_cast<unsigned long long *>(reinterpret_cast<uint8_t *>(pool) + (uint32_t)((((id << SUB_BITS) | pos)) << 3));
  return pool + (((size_t)id << SUB_BITS) | pos);
}

// entries of a tile beyond TILE_DIRECT: key and slot of (tile, entry number) in the hash (written by the marches, tsdf_pool.h; read by the resolve)
__device__ __forceinline__ unsigned long long big_key(uint32_t tile, uint32_t j) { return ((unsigned long long)tile << 24) | j; } // j < 2^23
__device__ __forceinline__ uint32_t big_slot(unsigned long long key, uint32_t mask) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask; }

// The launchers, one per stage file: each enqueues its kernels on `s` with a grid it works out itself and waits for nothing.
// small: 32-bit offsets into the voxel bytes and the record pool (vox_ptr / rec_ptr); s0: new_map is not (tau, 0), every candidate
// goes through the order keys; fuse: the resolve integrates straight into avg_map.
void enqueue_scatter_prep(ws_map *m, hipStream_t s);                              // tsdf_setup.hip
void launch_ray_setup(const ScatterArgs &sa, hipStream_t s);                      // tsdf_setup.hip: set-up pass + sort
void launch_march_tail(ws_map *m, const ScatterArgs &sa, bool small, hipStream_t s); // tsdf_tail.hip (sets m->tail_blocks)
void launch_march_free(const ScatterArgs &sa, bool small, hipStream_t s);         // tsdf_free.hip
void launch_tile_resolve(ws_map *m, const ScatterArgs &sa, bool s0, bool fuse, hipStream_t s); // tsdf_resolve.hip (sets m->resolve_blocks)
} // namespace ws
