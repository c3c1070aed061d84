// map_clearance.hip — clearance of candidate trajectories against a distance result (gfx950): T trajectories of P poses, a body of K
// spheres, and per trajectory the smallest margin, the first colliding pose, the counts and a soft cost, in one launch.  The rules are
// stated in warpsense_hip.h at ws_map_clearance and written down in ws_clearance.h; this file reads the `class | d2` records of a
// DistResult alone, so it serves the window of a map, the store and the ground bridge alike.
//
//   clearance_kernel       one workgroup of 256 lanes per trajectory.  G, the power of two >= K, consecutive lanes form a group that takes
//                          one pose at a time, lane k of the group sphere k; the 256 / G groups stride over the poses.  A lane rotates its own
//                          offset (nine int64 multiply-adds) and gathers one record.  Under WS_CLEARANCE_POSES the group folds its
//                          lanes (G <= 64: it lies in one wave) and stores the pose record.  Each lane keeps its own partial over its poses; the
//                          wave folds a biased (margin, index) key by min, first_hit by min, counts and cost by adds; the four waves meet
//                          in LDS and lane 0 stores the record.  No atomics, nothing to clear.
//   clearance_best_kernel  one workgroup over the T records: the smallest (cost, index) among the trajectories that qualify
#include "ws_clearance.h"
#include "ws_internal.h"

namespace ws
{
constexpr uint32_t CLEAR_WG = 256, CLEAR_BEST_WG = 1024;

struct ClearArgs
{
  ClearBox box;
  const uint32_t *dist; // the records of the distance result (never read when the box is empty)
  const int32_t *poses; // [t][p][12]
  const int32_t *body;  // [k][4]
  ClearRecord *rec;     // [t]
  ClearPose *pose_rec;  // [t][p], nullptr without WS_CLEARANCE_POSES
  unsigned long long *best;
  uint32_t t, p, k, g;  // g: lanes of a group, the power of two >= k
  int32_t res, soft;
  uint32_t outside_ok;
};

__device__ __forceinline__ uint32_t clear_shfl(uint32_t v, int d) { return (uint32_t)__shfl_xor((int)v, d, 64); }
__device__ __forceinline__ uint64_t clear_shfl64(uint64_t v, int d)
{
  return ((uint64_t)clear_shfl((uint32_t)(v >> 32), d) << 32) | clear_shfl((uint32_t)(v & 0xffffffffull), d);
}

struct ClearPartial // what a lane, a wave, a workgroup has seen of a trajectory
{
  uint64_t key, cost, hit_out; // hit_out: hits << 32 | outside (each at most 2^22)
  uint32_t first_hit, unknown;
};

__device__ __forceinline__ void clear_fold(ClearPartial &a, const ClearPartial &b)
{
  a.key = clear_min_key(a.key, b.key);
  a.first_hit = min(a.first_hit, b.first_hit);
  a.hit_out += b.hit_out;
  a.unknown += b.unknown;
  a.cost += b.cost;
}

__global__ __launch_bounds__(CLEAR_WG) void clearance_kernel(ClearArgs a)
{
  __shared__ int32_t body[CLEAR_MAX_SPHERES * 4];
  __shared__ ClearPartial part[CLEAR_WG / 64];
  const uint32_t traj = blockIdx.x, lane = threadIdx.x;
  if (lane < a.k * 4u) body[lane] = a.body[lane]; // (k <= 64: one word per lane)
  __syncthreads();
  const uint32_t k = lane & (a.g - 1u), group = lane / a.g, groups = CLEAR_WG / a.g;
  const bool sphere = k < a.k;
  const int32_t off[3] = {sphere ? body[4 * k] : 0, sphere ? body[4 * k + 1] : 0, sphere ? body[4 * k + 2] : 0};
  const int32_t radius = sphere ? body[4 * k + 3] : 0;
  ClearPartial mine = {CLEAR_NO_KEY, 0ull, 0ull, 0xffffffffu, 0u};
  // (every lane of a wave runs the same rounds: the folds below are whole-wave shuffles)
  for (uint32_t p0 = 0; p0 < a.p; p0 += groups)
  {
    const uint32_t p = p0 + group;
    const bool active = sphere && p < a.p;
    bool hit = false, outside = false;
    int32_t margin = CLEAR_NONE;
    if (active)
    {
      const int32_t *pose = a.poses + ((size_t)traj * a.p + p) * 12u;
      int32_t m[12];
      for (int j = 0; j < 12; ++j) m[j] = pose[j];
      const int64_t x = clear_voxel(clear_centre(m, off, 0), a.res), y = clear_voxel(clear_centre(m, off, 1), a.res),
                    z = clear_voxel(clear_centre(m, off, 2), a.res);
      uint64_t at;
      if (clear_locate(a.box, x, y, z, &at))
      {
        const uint32_t r = a.dist[at];
        margin = clear_margin(r & 0xffffffu, a.res, radius);
        hit = margin < 0;
        mine.key = clear_min_key(mine.key, clear_key(margin, p * CLEAR_MAX_SPHERES + k));
        if (hit) mine.first_hit = min(mine.first_hit, p), mine.hit_out += 1ull << 32;
        if ((r >> 30) == 0u) mine.unknown += 1u;
        mine.cost += clear_penalty(margin, a.soft);
      }
      else
        outside = true, mine.hit_out += 1ull;
    }
    if (a.pose_rec)
    {
      // the group's lanes into lane 0 of the group: xor distances below g stay inside it
      uint32_t pm = (uint32_t)margin ^ 0x80000000u, cnt = ((hit ? 1u : 0u) << 16) | (outside ? 1u : 0u);
      for (uint32_t d = a.g >> 1; d > 0u; d >>= 1)
      {
        pm = min(pm, clear_shfl(pm, (int)d));
        cnt += clear_shfl(cnt, (int)d);
      }
      if (k == 0u && p < a.p)
      {
        ClearPose out;
        out.min_margin = (int32_t)(pm ^ 0x80000000u);
        out.hits = (uint16_t)(cnt >> 16);
        out.outside = (uint16_t)(cnt & 0xffffu);
        a.pose_rec[(size_t)traj * a.p + p] = out;
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1)
  {
    ClearPartial o;
    o.key = clear_shfl64(mine.key, d), o.cost = clear_shfl64(mine.cost, d), o.hit_out = clear_shfl64(mine.hit_out, d);
    o.first_hit = clear_shfl(mine.first_hit, d), o.unknown = clear_shfl(mine.unknown, d);
    clear_fold(mine, o);
  }
  if ((lane & 63u) == 0u) part[lane >> 6] = mine;
  __syncthreads();
  if (lane != 0u) return;
  for (uint32_t w = 1; w < CLEAR_WG / 64u; ++w) clear_fold(mine, part[w]);
  ClearRecord out;
  out.min_margin = clear_key_margin(mine.key);
  out.first_hit = (int32_t)mine.first_hit; // (0xFFFFFFFF is -1)
  out.argmin = (uint32_t)(mine.key & 0xffffffffull);
  out.hits = (uint32_t)(mine.hit_out >> 32);
  out.outside = (uint32_t)(mine.hit_out & 0xffffffffull);
  out.unknown = mine.unknown;
  out.cost = mine.cost;
  a.rec[traj] = out;
}

// the smallest (cost, index) among the records without a hit and, unless outside_ok, without an outside sample: a minimum, exact in any order
__global__ __launch_bounds__(CLEAR_BEST_WG) void clearance_best_kernel(ClearArgs a)
{
  __shared__ uint64_t cost_s[CLEAR_BEST_WG / 64];
  __shared__ uint32_t idx_s[CLEAR_BEST_WG / 64];
  uint64_t cost = ~0ull;
  uint32_t idx = 0xffffffffu;
  for (uint32_t j = threadIdx.x; j < a.t; j += CLEAR_BEST_WG)
  {
    const ClearRecord r = a.rec[j];
    if (r.hits == 0u && (a.outside_ok || r.outside == 0u) && clear_better(r.cost, j, cost, idx)) cost = r.cost, idx = j;
  }
  for (int d = 32; d > 0; d >>= 1)
  {
    const uint64_t oc = clear_shfl64(cost, d);
    const uint32_t oi = clear_shfl(idx, d);
    if (clear_better(oc, oi, cost, idx)) cost = oc, idx = oi;
  }
  if ((threadIdx.x & 63u) == 0u) cost_s[threadIdx.x >> 6] = cost, idx_s[threadIdx.x >> 6] = idx;
  __syncthreads();
  if (threadIdx.x != 0u) return;
  for (uint32_t w = 1; w < CLEAR_BEST_WG / 64u; ++w)
    if (clear_better(cost_s[w], idx_s[w], cost, idx)) cost = cost_s[w], idx = idx_s[w];
  *a.best = idx == 0xffffffffu ? ~0ull : (unsigned long long)idx; // (int64: -1 for none)
}

int launch_clearance(ClearanceResult &q, const DistResult &d, hipStream_t s, const ClearCall &c, const int32_t *poses_dev)
{
  ClearArgs a;
  const bool columns = (d.flags & WS_DISTANCE_COLUMNS) != 0;
  for (int k = 0; k < 3; ++k) a.box.lo[k] = d.lo[k], a.box.ext[k] = d.n ? d.ext[k] : 0u; // (no records: every sample is OUTSIDE)
  a.box.columns = columns ? 1u : 0u;
  a.dist = d.rec.as<uint32_t>();
  a.poses = poses_dev;
  a.body = q.body.as<int32_t>();
  a.rec = q.rec.as<ClearRecord>();
  a.pose_rec = (c.flags & WS_CLEARANCE_POSES) ? q.pose_rec.as<ClearPose>() : nullptr;
  a.best = q.best.dev;
  a.t = (uint32_t)c.t, a.p = (uint32_t)c.p, a.k = c.k;
  a.g = 1u;
  while (a.g < c.k) a.g <<= 1;
  a.res = c.res, a.soft = c.soft;
  a.outside_ok = (c.flags & WS_CLEARANCE_OUTSIDE_OK) ? 1u : 0u;
  q.timer.mark(1, s);
  hipLaunchKernelGGL(clearance_kernel, dim3((unsigned)c.t), dim3(CLEAR_WG), 0, s, a);
  q.timer.mark(2, s);
  hipLaunchKernelGGL(clearance_best_kernel, dim3(1), dim3(CLEAR_BEST_WG), 0, s, a);
  q.timer.mark(3, s);
  WS_HIP(hipGetLastError());
  return q.best.fetch(s);
}

} // namespace ws
