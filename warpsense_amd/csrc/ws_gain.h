// ws_gain.h — the rules of the view gain (stated in include/warpsense_hip.h at ws_map_view_gain), shared by the view gain of a window
// (map_gain.hip) and of the chunk store (store_gain.hip).  Both walk the samples p_k of ws_raycast.h (RayWalk) from m origins along one
// fan of n directions, look up the ONE entry of a sample's voxel and count it by class; what differs is where the entries lie.
// Everything that decides a byte of a record is here, once: gain_march takes a FIELD, an object of the including file with
//
//   bool entry(v, raw)   the raw entry of voxel v of the box; false: there is no such voxel in memory (an absent chunk: UNKNOWN)
//
// The box is the call's (GainCommon): a voxel outside it counts for nothing and blocks nothing.
//
//   gain_prep_kernel    one lane per direction of the fan: L, quotient and remainder of |d| step by L and the signs, once per call
//                       instead of once per (view, ray): one integer square root and three 64-bit divisions
//   gain_march          one lane per (view, ray): the walk
//   gain_reduce         the wave's lanes into the view's record: ballot / popcount for the ray counts, cross-lane adds for the sums,
//                       then one integer atomic add per wave and field.  Integer sums are exact in any order: the same bytes on
//                       every run.  No float anywhere.
//   gain_best_kernel    the largest unknown_k2 of the call's records
#pragma once

#include "ws_raycast.h"

namespace ws
{
struct GainRecord // 32 bytes, one per view
{
  unsigned long long unknown_k2, free_k2;
  uint32_t unknown, free_n, blocked, live;
};
static_assert(sizeof(GainRecord) == 32, "the view record of ws_map_view_gain is 32 bytes");

struct GainRay // 8 bytes, one per (view, ray) under WS_GAIN_RAYS
{
  uint32_t unknown;
  int32_t stop; // k of the blocking sample, -1 none, -2 dead
};

struct alignas(16) GainPrep // 32 bytes, one per direction: what RayWalk::start computes
{
  uint32_t L; // 0: a dead ray
  uint32_t qd[3], rd[3];
  uint32_t sgn; // 2 bits per axis: 0 zero, 1 positive, 2 negative
};

struct GainCommon
{
  const int32_t *origins; // m x 3
  const int32_t *dirs;    // n x 3
  uint32_t m, n;
  GainPrep *prep;         // n
  int32_t lo[3], hi[3];   // the box, inclusive world voxels; lo > hi on an axis: empty
  int32_t res, step;
  uint32_t K;             // samples 0 .. K
  FastDiv rdiv;           // division by res
  int32_t min_value;
  uint32_t flags;
  GainRecord *rec;        // m, zero when the march starts
  GainRay *rays;          // m x n, view-major; nullptr without WS_GAIN_RAYS
  unsigned long long *best;
};

// ... from a checked call and the buffers of a result holder (origins and directions are in its staging)
inline GainCommon gain_common(const GainResult &q, const GainCall &c)
{
  GainCommon a;
  a.origins = q.org.as<int32_t>();
  a.dirs = q.dirs.as<int32_t>();
  a.m = (uint32_t)c.m;
  a.n = (uint32_t)c.n;
  a.prep = static_cast<GainPrep *>(q.prep.p);
  for (int k = 0; k < 3; ++k) a.lo[k] = c.lo[k], a.hi[k] = c.hi[k];
  a.res = c.res;
  a.step = c.res / 2 > 1 ? c.res / 2 : 1;
  a.K = (uint32_t)(c.max_range / a.step);
  a.rdiv = make_fastdiv(c.res);
  a.min_value = c.min_value;
  a.flags = c.flags;
  a.rec = static_cast<GainRecord *>(q.rec.p);
  a.rays = (c.flags & WS_GAIN_RAYS) ? static_cast<GainRay *>(q.rays.p) : nullptr;
  a.best = q.best.dev;
  return a;
}

__device__ __forceinline__ void gain_prep(const GainCommon &a, uint32_t i)
{
  RayCommon rc;
  rc.dirs = a.dirs;
  rc.flags = 0u;
  rc.step = a.step;
  RayWalk w;
  GainPrep p = {};
  if (w.start(rc, i))
  {
    p.L = w.L;
#pragma unroll
    for (int x = 0; x < 3; ++x)
    {
      p.qd[x] = w.qd[x];
      p.rd[x] = w.rd[x];
      p.sgn |= (w.sgn[x] > 0 ? 1u : (w.sgn[x] < 0 ? 2u : 0u)) << (2 * x);
    }
  }
  a.prep[i] = p;
}

// what one lane brings to its view's record
struct GainLane
{
  uint32_t unknown = 0, free_n = 0;
  unsigned long long unknown_k2 = 0, free_k2 = 0;
  int32_t stop = -2;
};

// The walk of (view, ray).  Shortened against the rules only where the bytes stay the same: the class of a voxel is kept while the
// voxel stays (step = res / 2: a voxel repeats), and the ray ends once its voxel has passed the box for good -- each axis of p_k is
// monotone in k, so beyond the box along an axis it moves away on (or stands still beside it) every later sample is outside.
template <class Field> __device__ __forceinline__ GainLane gain_march(const GainCommon &a, Field &fld, const int32_t o[3], const GainPrep &p)
{
  GainLane out;
  if (p.L == 0u) return out;
  out.stop = -1;
  const bool any_weight = (a.flags & WS_GAIN_ANY_WEIGHT) != 0;
  RayWalk w;
  w.L = p.L;
#pragma unroll
  for (int x = 0; x < 3; ++x)
  {
    const uint32_t s = (p.sgn >> (2 * x)) & 3u;
    w.qd[x] = p.qd[x], w.rd[x] = p.rd[x], w.q[x] = w.r[x] = 0u;
    w.sgn[x] = s == 1u ? 1 : (s == 2u ? -1 : 0);
  }
  int32_t cv[3] = {INT32_MIN, INT32_MIN, INT32_MIN}; // voxel of `cls` (no sample has this one: p / res > INT32_MIN)
  int cls = 0;                                       // 0 outside the box, 1 UNKNOWN, 2 FREE, 3 OCCUPIED
  for (uint32_t k = 0; k <= a.K; ++k)
  {
    int32_t v[3], f;
    bool gone = false;
#pragma unroll
    for (int x = 0; x < 3; ++x)
    {
      v[x] = floor_div(o[x] + w.sgn[x] * (int32_t)w.q[x], a.rdiv, f); // (|o| + max_range fits: checked by the host)
      gone = gone || (w.sgn[x] >= 0 && v[x] > a.hi[x]) || (w.sgn[x] <= 0 && v[x] < a.lo[x]);
    }
    if (gone) break;
    if (v[0] != cv[0] || v[1] != cv[1] || v[2] != cv[2])
    {
      cv[0] = v[0], cv[1] = v[1], cv[2] = v[2];
      const bool inside = v[0] >= a.lo[0] && v[0] <= a.hi[0] && v[1] >= a.lo[1] && v[1] <= a.hi[1] && v[2] >= a.lo[2] && v[2] <= a.hi[2];
      cls = 0;
      if (inside)
      {
        uint32_t raw = 0u;
        cls = 1;
        if (fld.entry(v, raw) && ray_valid(raw, any_weight)) cls = entry_value(raw) >= a.min_value ? 2 : 3;
      }
    }
    if (cls == 3)
    {
      out.stop = (int32_t)k;
      break;
    }
    const unsigned long long k2 = (unsigned long long)(k * k); // k <= 8191
    if (cls == 1) out.unknown += 1u, out.unknown_k2 += k2;
    if (cls == 2) out.free_n += 1u, out.free_k2 += k2;
    w.advance();
  }
  return out;
}

__device__ __forceinline__ unsigned long long gain_wave_sum(unsigned long long v)
{
  for (int d = 32; d > 0; d >>= 1)
  {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(v & 0xffffffffull), d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// every lane of the wave calls this (`active`: the lane has a ray); the per-ray record, then the wave's share of the view's record
__device__ __forceinline__ void gain_reduce(const GainCommon &a, uint32_t view, uint32_t i, bool active, const GainLane &r)
{
  if (active && a.rays)
  {
    GainRay out;
    out.unknown = r.unknown;
    out.stop = r.stop;
    a.rays[(size_t)view * (size_t)a.n + i] = out;
  }
  const uint32_t live = (uint32_t)__popcll(__ballot(active && r.stop != -2)), blocked = (uint32_t)__popcll(__ballot(active && r.stop >= 0));
  // (counts first: a ray has at most 8192 samples, 64 rays 2^19)
  const unsigned long long counts = gain_wave_sum(active ? ((unsigned long long)r.free_n << 32) | r.unknown : 0ull);
  const unsigned long long uk2 = gain_wave_sum(active ? r.unknown_k2 : 0ull), fk2 = gain_wave_sum(active ? r.free_k2 : 0ull);
  if ((threadIdx.x & 63u) != 0u) return;
  GainRecord *g = a.rec + view;
  if (uk2) atomicAdd(&g->unknown_k2, uk2);
  if (fk2) atomicAdd(&g->free_k2, fk2);
  if ((uint32_t)counts) atomicAdd(&g->unknown, (uint32_t)counts);
  if ((uint32_t)(counts >> 32)) atomicAdd(&g->free_n, (uint32_t)(counts >> 32));
  if (blocked) atomicAdd(&g->blocked, blocked);
  if (live) atomicAdd(&g->live, live);
}

// the largest unknown_k2 of the m records: a maximum, exact in any order
__device__ __forceinline__ void gain_best(const GainCommon &a)
{
  unsigned long long best = 0ull;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < a.m; j += gridDim.x * blockDim.x) best = max(best, a.rec[j].unknown_k2);
  for (int d = 32; d > 0; d >>= 1)
  {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(best & 0xffffffffull), d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), d, 64);
    best = max(best, ((unsigned long long)hi << 32) | lo);
  }
  if ((threadIdx.x & 63u) == 0u && best) atomicMax(a.best, best);
}

// The launch sequence, whatever the field: `Args` is the including file's, with the GainCommon `c`.  Events: 1 the records are clear
// and the fan is prepared ... 2 the march ... 3 the maximum; it arrives in q.best.host once the stream has been synchronised
template <typename Args> int gain_launch(GainResult &q, hipStream_t s, const Args &a, void (*prep)(Args), void (*march)(Args), void (*best)(Args))
{
  WS_HIP(hipMemsetAsync(a.c.rec, 0, (size_t)a.c.m * sizeof(GainRecord), s));
  WS_HIP(hipMemsetAsync(a.c.best, 0, sizeof(unsigned long long), s));
  q.timer.mark(1, s);
  hipLaunchKernelGGL(prep, dim3((a.c.n + 255u) / 256u), dim3(256), 0, s, a);
  hipLaunchKernelGGL(march, dim3((a.c.n + 63u) / 64u, a.c.m), dim3(64), 0, s, a);
  q.timer.mark(2, s);
  hipLaunchKernelGGL(best, dim3((a.c.m + 255u) / 256u), dim3(256), 0, s, a);
  q.timer.mark(3, s);
  WS_HIP(hipGetLastError());
  return q.best.fetch(s);
}

} // namespace ws
