// ws_reach.h — the rules of ws_map_reach / ws_store_reach (stated in warpsense_hip.h) once, for the kernels of map_reach.hip and for
// the host: which record of a distance result a path may visit, what a step costs, and where a world voxel lies in the records.
#pragma once

#include "ws_internal.h"

namespace ws
{
// a record `class | d2` of ws_map_distance is traversable iff it is FREE (or UNKNOWN under WS_REACH_UNKNOWN_FREE) and keeps the clearance
__host__ __device__ inline bool reach_traversable(uint32_t rec, uint32_t clear_d2, uint32_t flags)
{
  const uint32_t cls = rec >> 30;
  return (cls == 1u || (cls == 0u && (flags & WS_REACH_UNKNOWN_FREE) != 0u)) && (rec & 0xffffffu) >= clear_d2;
}

// a step that changes 1, 2 or 3 coordinates: face, edge, corner
__host__ __device__ constexpr uint32_t reach_weight(int da, int db, int dc) { return (da != 0) + (db != 0) + (dc != 0) == 1 ? 10u : (da != 0) + (db != 0) + (dc != 0) == 2 ? 14u : 17u; }

// (a, b, c) of a world voxel in the records of the box; false outside.  Under columns z is ignored and a = 0: the 8-neighbourhood of a
// column is the 26-neighbourhood of a box one record thick, and ascending (dx, dy) is ascending (da, db, dc).
__host__ __device__ inline bool reach_locate(const ReachBox &b, int32_t x, int32_t y, int32_t z, uint32_t p[3])
{
  const int64_t u = (int64_t)x - b.lo[0], v = (int64_t)y - b.lo[1], w = b.columns ? 0 : (int64_t)z - b.lo[2];
  const int64_t a = b.columns ? 0 : u, bb = b.columns ? u : v, c = b.columns ? v : w;
  if (a < 0 || bb < 0 || c < 0 || a >= (int64_t)b.e[0] || bb >= (int64_t)b.e[1] || c >= (int64_t)b.e[2]) return false;
  p[0] = (uint32_t)a, p[1] = (uint32_t)bb, p[2] = (uint32_t)c;
  return true;
}

// a reach result holds fewer than 2^32 / 17 records: the index fits 32 bits
__host__ __device__ inline uint32_t reach_index(const ReachBox &b, uint32_t a, uint32_t bb, uint32_t c) { return (a * b.e[1] + bb) * b.e[2] + c; }

// the neighbour p + (da, db, dc) of a record; false where the box ends
__host__ __device__ inline bool reach_neighbour(const ReachBox &b, const uint32_t p[3], int da, int db, int dc, uint32_t q[3])
{
  const int64_t a = (int64_t)p[0] + da, bb = (int64_t)p[1] + db, c = (int64_t)p[2] + dc;
  if (a < 0 || bb < 0 || c < 0 || a >= (int64_t)b.e[0] || bb >= (int64_t)b.e[1] || c >= (int64_t)b.e[2]) return false;
  q[0] = (uint32_t)a, q[1] = (uint32_t)bb, q[2] = (uint32_t)c;
  return true;
}

// the tile grid of a box: tile extents (REACH_VA .. VC for a volume, REACH_CA .. CC for columns), tiles per axis nt, tile id = (ta nt[1] + tb) nt[2] + tc
struct ReachGrid
{
  uint32_t nt[3];
  uint32_t n_tiles;
};
__host__ __device__ inline ReachGrid reach_grid(const ReachBox &b)
{
  const uint32_t t[3] = {(uint32_t)(b.columns ? REACH_CA : REACH_VA), (uint32_t)(b.columns ? REACH_CB : REACH_VB), (uint32_t)(b.columns ? REACH_CC : REACH_VC)};
  ReachGrid g;
  for (int k = 0; k < 3; ++k) g.nt[k] = (uint32_t)(((uint64_t)b.e[k] + t[k] - 1u) / t[k]);
  g.n_tiles = g.nt[0] * g.nt[1] * g.nt[2]; // (at most the number of records)
  return g;
}
} // namespace ws
