// ws_fuse.h — the rules of ws_store_fuse (stated in include/warpsense_hip.h): the pull transform of a dst voxel centre into the frame
// of SRC, the trilinear sample of SRC there with the zero-coefficient rule, and the weighted-average integrate into the dst entry.
// Everything that decides a byte is here, as functions of integers; store_fuse.hip holds the two passes that call them and
// api_store_pair.hip the plan.  The cell (base voxel, fractions, T) is that of ws_raycast.h / ws_sample.h; SRC is read through the chunk
// lookup of ws_field_store.h.
#pragma once

#include "ws_field_store.h"

namespace ws
{
constexpr uint32_t FUSE_WG = 256;           // four waves, one z column of a dst chunk per wave at a time
constexpr uint32_t FUSE_TILES = 256;        // workgroups per dst chunk: 16 x 16 tiles of 4 x 4 columns
constexpr int64_t FUSE_REACH = 1ll << 24;   // a dst voxel takes part iff |p - pivot_dst| < this on every axis (mm)
constexpr uint32_t FUSE_STATS_DEV = 4;      // 64-bit sums the count pass leaves: averaged, set, sum |nv - ev|, sum min(nw, ew)
constexpr size_t FUSE_MAX_CANDIDATES = (size_t)1 << 23; // FUSE_TILES workgroups each in one grid

// floor(n / d) for 0 <= n < 2^47 and 1 <= d <= 2^30 by multiply-shift, as FastDiv does for 31 bits: k = 47 + ceil(log2 d),
// M = ceil(2^k / d) < 2^49; the error M d - 2^k < d <= 2^(k - 47) gives n (M d - 2^k) < 2^k, so the quotient is exact.
struct FuseDiv
{
  uint64_t M;
  uint32_t k; // 47 .. 77
};
inline FuseDiv make_fuse_div(int64_t d)
{
  FuseDiv f;
  uint32_t l = 0;
  while ((1ll << l) < d) ++l;
  f.k = 47u + l;
  const unsigned __int128 p = (unsigned __int128)1 << f.k;
  f.M = (uint64_t)(p / (unsigned __int128)d) + ((p % (unsigned __int128)d) ? 1u : 0u);
  return f;
}

// a candidate chunk of DST: its key, and its slot (STORE_ABSENT: the chunk does not exist, every voxel of it holds fill_entry)
struct alignas(16) FuseCand
{
  int32_t cx, cy, cz;
  uint32_t slot;
};

// what both passes are asked (kernel argument: at most 256 bytes, all of it wave-uniform)
struct FuseArgs
{
  int32_t rot[9], pd[3], ps[3]; // ws_fuse_pose
  int32_t res, half, max_weight;
  uint32_t fill; // fill_entry of DST (weight <= 0)
  FastDiv rdiv;  // division by res
  FuseDiv tdiv;  // division by res^3
  int64_t res3;
  const FuseCand *cand;
  const StoreRaySlot *src_table; // the lookup key -> slot of SRC's chunks (store_ray_table_fill)
  uint32_t *const *src_segs;
  uint32_t *const *dst_segs;
  uint32_t src_mask, src_shift, dst_shift;
  uint32_t *counts;          // count pass: per candidate the voxels that receive a valid sample
  unsigned long long *stats; // count pass: FUSE_STATS_DEV sums
};
static_assert(sizeof(FuseArgs) <= 256, "the kernel arguments of ws_store_fuse stay within 256 bytes");

__device__ __forceinline__ uint64_t fuse_div(uint64_t n, const FuseDiv &d)
{
  const uint64_t hi = __umul64hi(n, d.M), lo = n * d.M;
  return d.k >= 64u ? hi >> (d.k - 64u) : (hi << (64u - d.k)) | (lo >> d.k);
}

// the chunk of SRC with this key through the field's one-chunk cache, nullptr if absent
__device__ __forceinline__ const uint32_t *fuse_src_chunk(StoreField &fld, int32_t cx, int32_t cy, int32_t cz)
{
  if (cx != fld.ck[0] || cy != fld.ck[1] || cz != fld.ck[2])
  {
    fld.cp = fld.lookup(cx, cy, cz);
    fld.ck[0] = cx, fld.ck[1] = cy, fld.ck[2] = cz;
  }
  return fld.cp;
}

// q = floor((rot (p - pivot_dst) + 2^29) / 2^30) + pivot_src on one axis; `base` is the part of the sum that x and y give, with the
// 2^29 (uniform over a column), dz = p_z - pivot_dst_z.  |sum| < 2^56.
__device__ __forceinline__ int64_t fuse_pull(int64_t base, int32_t rot_z, int32_t dz, int32_t pivot_src) { return ((base + (int64_t)rot_z * (int64_t)dz) >> 30) + (int64_t)pivot_src; }

// a component of q the sample calls dead
__device__ __forceinline__ bool fuse_dead(int64_t q) { return q <= -(1ll << 30) || q >= (1ll << 30); }

// The sample of SRC in the cell with base voxel b and fractions f (0 <= f < res): a corner whose trilinear coefficient is zero takes
// part neither in validity nor in the weight.  false: not valid.  nv = floor(T / res^3), nw = the smallest weight that takes part.
// Args: res, res3 and tdiv are read (FuseArgs; the ChangesArgs of ws_changes.h)
template <typename Args> __device__ __forceinline__ bool fuse_sample(const Args &a, StoreField &fld, const int32_t b[3], const int32_t f[3], int32_t &nv, int32_t &nw)
{
  const int32_t wx[2] = {a.res - f[0], f[0]}, wy[2] = {a.res - f[1], f[1]}, wz[2] = {a.res - f[2], f[2]};
  int64_t T = 0;
  int32_t wmin = INT32_MAX;
  bool valid = true;
#pragma unroll
  for (int j = 0; j < 8; ++j)
  {
    const int32_t coef = wx[j >> 2] * wy[(j >> 1) & 1] * wz[j & 1]; // <= res^3 <= 2^30
    if (coef == 0 || !valid) continue;
    const int32_t v[3] = {b[0] + (j >> 2), b[1] + ((j >> 1) & 1), b[2] + (j & 1)};
    const uint32_t *p = fuse_src_chunk(fld, v[0] >> 6, v[1] >> 6, v[2] >> 6);
    if (!p)
    {
      valid = false;
      continue;
    }
    const uint32_t raw = p[((uint32_t)v[0] & 63u) * (uint32_t)(STORE_CS * STORE_CS) + ((uint32_t)v[1] & 63u) * (uint32_t)STORE_CS + ((uint32_t)v[2] & 63u)];
    const int32_t w = entry_weight(raw);
    valid = w > 0;
    wmin = min(wmin, w);
    T += (int64_t)entry_value(raw) * (int64_t)coef;
  }
  if (!valid) return false;
  // -2^15 res^3 <= T < 2^15 res^3: the shifted numerator is in [0, 2^46)
  nv = (int32_t)fuse_div((uint64_t)(T + (a.res3 << 15)), a.tdiv) - 32768;
  nw = wmin;
  return true;
}

// wso_update_avg on the dst entry for a valid sample (nw > 0): the new entry
__device__ __forceinline__ uint32_t fuse_integrate(uint32_t existing, int32_t nv, int32_t nw, int32_t max_weight)
{
  const int32_t ev = entry_value(existing), ew = entry_weight(existing);
  if (ew <= 0) return pack_entry(nv, nw);
  const int32_t v = (ev * ew + nv * nw) / (ew + nw); // |numerator| < 2^31, C's truncating division
  return pack_entry(v, min(max_weight, ew + nw));
}

// store_fuse.hip: one pass over `n_candidates` chunks of a.cand; the count pass adds into a.counts and a.stats, which the caller has cleared
int launch_store_fuse(hipStream_t s, const FuseArgs &a, size_t n_candidates, bool write);

} // namespace ws
