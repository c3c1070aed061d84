// ws_changes.h — the rules of ws_store_changes (stated in include/warpsense_hip.h): the classes of a known side, the verdict on one
// voxel of CUR against the sample of REF at its place, and the record's word.  Everything that decides a byte is here, as functions
// of values; store_changes.hip holds the passes that call them and api_store_pair.hip the host flow.  The transform and the sample are
// those of the fuse (ws_fuse.h: fuse_pull, fuse_dead, fuse_sample over the StoreField lookup); the word space is that of the store's
// surface cloud and frontier (ws_store_words.h).
#pragma once

#include "ws_fuse.h"
#include "ws_store_words.h"

namespace ws
{
constexpr uint32_t CH_WORDS = 256;    // words per workgroup of the word passes (one per thread)
constexpr uint32_t CH_STATS_DEV = 5;  // 64-bit sums the count pass leaves: known on both sides, appeared, vanished, new ground, sum |nv - ev|
constexpr uint32_t CH_OCCUPIED = 1u, CH_FREE = 2u; // classes of a known side (0: neither)
constexpr uint32_t CH_APPEARED = 1u, CH_VANISHED = 2u; // kinds, the low two bits of a verdict (0: no change)
constexpr uint32_t CH_BOTH = 4u;      // verdict: known on both sides
constexpr uint32_t CH_NEW = 8u;       // verdict: known in CUR and not in REF

struct ChangesRule
{
  int32_t band, free_value, min_weight; // 1 <= band <= free_value <= 32767, 1 <= min_weight <= 32767
};

// OCCUPIED iff |d| < band; FREE iff d >= free_value (free_value >= band: never both); raw values, the store knows no tau
__device__ __forceinline__ uint32_t changes_class(int32_t d, const ChangesRule &r) { return d < r.band && d > -r.band ? CH_OCCUPIED : d >= r.free_value ? CH_FREE : 0u; }

// The verdict on a voxel of CUR with entry (ev, ew) against the sample of REF at its place ((nv, nw) if `valid`): 0 if CUR is not
// known; CH_NEW if REF is not; else CH_BOTH with the kind in the low bits, and diff = |nv - ev|
__device__ __forceinline__ uint32_t changes_verdict(int32_t ev, int32_t ew, bool valid, int32_t nv, int32_t nw, const ChangesRule &r, uint32_t &diff)
{
  diff = 0u;
  if (ew < r.min_weight) return 0u;
  if (!valid || nw < r.min_weight) return CH_NEW;
  diff = (uint32_t)(nv > ev ? nv - ev : ev - nv);
  const uint32_t ce = changes_class(ev, r), cn = changes_class(nv, r);
  const uint32_t kind = ce == CH_OCCUPIED && cn == CH_FREE ? CH_APPEARED : ce == CH_FREE && cn == CH_OCCUPIED ? CH_VANISHED : 0u;
  return CH_BOTH | kind;
}

// the fourth word of a record: the value REF holds at the place, and the kind
__device__ __forceinline__ uint32_t changes_word(int32_t nv, uint32_t kind) { return ((uint32_t)nv & 0xffffu) | (kind << 16); }

// what the passes are asked (kernel argument, all of it wave-uniform)
struct ChangesArgs : StoreWords // the listed chunks of CUR
{
  int32_t rot[9], pd[3], ps[3]; // ws_fuse_pose
  int32_t res, half;
  FastDiv rdiv;  // division by res
  FuseDiv tdiv;  // division by res^3
  int64_t res3;
  ChangesRule rule;
  uint32_t kinds;        // bit (kind - 1): the kind becomes a record
  int32_t lo[3], hi[3];  // the box, inclusive world voxels of CUR
  const StoreRaySlot *ref_table; // the lookup key -> slot of REF's chunks (store_ray_table_fill)
  uint32_t *const *ref_segs;
  uint32_t ref_mask, ref_shift;
  unsigned long long *mask;          // [n_words]
  uint32_t *blk_tot;                 // [n_words / 256]
  const unsigned long long *blk_off; // [n_words / 256] exclusive scan of blk_tot
  su32x4 *rec;                       // x, y, z, changes_word
  unsigned long long cap;            // records the output buffer holds
  unsigned long long *stats;         // count pass: CH_STATS_DEV sums, cleared by the caller
};

} // namespace ws
