// map_ground.hip — the ground layer of a device map (gfx950): per (x, y) column of a box the one level something can stand on, its
// sub-voxel height and the largest height step to the neighbouring columns.  The rules are stated in warpsense_hip.h at ws_map_ground
// and written as functions of values in ws_ground.h; this file holds the walk over the ring and the two passes over the records that
// the window and the chunk store share.
//
//   ground_levels_kernel   pass 1: a wave per (x, y) column, four columns of consecutive y per workgroup, lane = z (the addressing of
//                          dist_classify_kernel).  The wave walks the column DOWN in steps of 64 voxels from the box's first z: two
//                          ballots give the OCCUPIED and the FREE voxels of a step as wave-uniform 64-bit words, the levels of the step
//                          are bit arithmetic on them and on the words carried from the step above (ws_ground.h), and the two values
//                          around the level come out of the lanes that hold them with a read-lane.  One add per workgroup and class.
//   ground_steps_kernel    pass 2: a lane per column, the 3 x 3 stencil over the 8-byte records of pass 1 into the records of the result
//   ground_sites_kernel    pass 0 of ws_*_ground_distance: a lane per column, the ground record -> class bits and g0 of a column
//                          distance field; the line passes behind it are dist_passes (map_distance.hip)
//
// Integers only, plain launches on the context's stream; the atomics are the class counters and the site counter.
#include "ws_device.h"
#include "ws_ground.h"

namespace ws
{
struct GroundArgs
{
  BoxArgs box;
  uint32_t col0;   // first column of this launch
  int32_t H;       // clear_vox
  uint32_t flags;
  uint2 *lvl;      // {z, word} per column
  unsigned long long *counts; // [4]
};

__global__ __launch_bounds__(256) void ground_levels_kernel(GroundArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t col64 = (uint64_t)a.col0 + (uint64_t)blockIdx.x * 4u + (uint64_t)wave;
  const bool active = col64 < (uint64_t)a.box.n_cols; // (the same for the whole wave)
  const bool any_weight = (a.flags & WS_GROUND_ANY_WEIGHT) != 0, unknown_ok = (a.flags & WS_GROUND_UNKNOWN_HEADROOM) != 0, top = (a.flags & WS_GROUND_TOP) != 0;
  int32_t level_z = 0;
  uint32_t word = 0;
  if (active)
  {
    int32_t x, y, zs0;
    const int64_t cbase = box_column(a.box, (uint32_t)col64, x, y, zs0);
    const int32_t sz = a.box.mp.size[2], ez = a.box.ez;
    bool found = false, any_occ = false, any_fre = false;
    int32_t v0 = 0, v1 = 0;
    uint64_t fre_above = 0ull, acc_above = 0ull; // above the box nothing is acceptable
    int32_t first_above = 0;                     // the value of voxel 0 of the step above
    for (int32_t z0 = ((ez - 1) >> 6) << 6; z0 >= 0; z0 -= 64)
    {
      const int32_t z = z0 + lane; // (relative to the box's first z)
      const bool in = z < ez;
      int32_t zi = zs0 + (in ? z : 0); // the ring's seam in z: the run goes on at storage z 0
      if (zi >= sz) zi -= sz;
      const uint32_t raw = in ? a.box.data[cbase + zi] : 0u; // (outside the box: weight 0, neither of the two ballots)
      const uint32_t cls = dist_class(raw, any_weight);
      const uint64_t occ = __ballot(cls == 2u), fre = __ballot(cls == 1u);
      const uint64_t acc = unknown_ok ? ground_in_box(z0, 0, (int64_t)ez - 1) & ~occ : fre;
      const uint64_t levels = ground_levels(occ, fre, acc, fre_above, acc_above, a.H);
      any_occ = any_occ || occ != 0ull;
      any_fre = any_fre || fre != 0ull;
      if (levels != 0ull)
      {
        const int32_t b = ground_pick(levels, top);
        v0 = entry_value(ground_lane(raw, b));
        v1 = b == 63 ? first_above : entry_value(ground_lane(raw, b + 1));
        level_z = a.box.lo[2] + z0 + b;
        found = true;
        if (top) break; // the highest level of the column
      }
      fre_above = fre, acc_above = acc;
      first_above = entry_value(ground_lane(raw, 0));
    }
    word = found ? ground_word(ground_frac(v0, v1), 0u, GROUND_GROUND) : ground_word(0u, 0u, ground_no_level(any_occ, any_fre));
  }
  ground_publish(a.lvl, a.counts, active, col64, level_z, word);
}

struct GroundStepArgs
{
  const uint2 *lvl;
  uint2 *rec;
  uint32_t nx, ny;
  uint32_t col0, n_cols; // first column of this launch, columns of the box
};

__global__ __launch_bounds__(256) void ground_steps_kernel(GroundStepArgs a)
{
  const uint64_t col = (uint64_t)a.col0 + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (col >= (uint64_t)a.n_cols) return;
  uint2 r = a.lvl[col];
  if (ground_class(r.y) == GROUND_GROUND)
  {
    const uint32_t xr = (uint32_t)(col / a.ny), yr = (uint32_t)(col - (uint64_t)xr * a.ny);
    const int64_t h = ground_height((int32_t)r.x, r.y);
    uint32_t step = 0u;
    for (int dx = -1; dx <= 1; ++dx)
      for (int dy = -1; dy <= 1; ++dy)
      {
        const int64_t xn = (int64_t)xr + dx, yn = (int64_t)yr + dy;
        if ((dx == 0 && dy == 0) || xn < 0 || yn < 0 || xn >= (int64_t)a.nx || yn >= (int64_t)a.ny) continue;
        const uint2 n = a.lvl[(uint64_t)xn * a.ny + (uint64_t)yn];
        if (ground_class(n.y) == GROUND_GROUND) step = max(step, ground_step(h, ground_height((int32_t)n.x, n.y)));
      }
    r.y = ground_word(r.y & 0xffu, step, GROUND_GROUND);
  }
  a.rec[col] = r;
}

struct GroundSiteArgs
{
  const uint2 *rec;
  uint32_t *out;
  uint16_t *plane;
  unsigned long long *sites;
  uint32_t col0, n_cols;
  uint32_t max_step, r2;
  uint32_t unknown_occ;
};

__global__ __launch_bounds__(256) void ground_sites_kernel(GroundSiteArgs a)
{
  const uint64_t col = (uint64_t)a.col0 + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  bool site = false;
  if (col < (uint64_t)a.n_cols)
  {
    const uint32_t cls = ground_dist_class(a.rec[col].y, a.max_step);
    site = cls == 2u || (a.unknown_occ && cls == 0u);
    a.out[col] = cls << 30;
    a.plane[col] = (uint16_t)(site ? 0u : a.r2);
  }
  const uint32_t n_sites = (uint32_t)__popcll(__ballot(site));
  if ((threadIdx.x & 63) == 0 && n_sites) atomicAdd(a.sites, (unsigned long long)n_sites);
}

// Pass 1 over the ring (events 0, 1): the class counters are cleared in front of it.
int launch_ground_levels(ws_map *m, GroundResult &q, int which, const int32_t lo[3], const int32_t ext[3], int32_t H, uint32_t flags)
{
  GroundArgs a;
  a.box = box_args(m, which, lo, ext);
  a.H = H;
  a.flags = flags;
  a.lvl = q.lvl.as<uint2>();
  a.counts = q.counts.dev;
  hipStream_t s = m->ctx->stream;
  WS_HIP(hipMemsetAsync(a.counts, 0, 4 * sizeof(unsigned long long), s));
  q.timer.mark(0, s);
  for (uint64_t c0 = 0; c0 < (uint64_t)a.box.n_cols; c0 += GROUND_PER_LAUNCH)
  {
    a.col0 = (uint32_t)c0;
    const uint32_t cols = (uint32_t)std::min<uint64_t>((uint64_t)a.box.n_cols - c0, GROUND_PER_LAUNCH);
    hipLaunchKernelGGL(ground_levels_kernel, dim3((cols + 3u) / 4u), dim3(256), 0, s, a);
  }
  q.timer.mark(1, s);
  return WS_OK;
}

// Pass 2 (events 1, 2) behind a pass 1 that has written q.lvl: the steps, into q.rec.  Both sources of a ground layer come here.
int ground_steps(hipStream_t s, GroundResult &q, uint32_t nx, uint32_t ny)
{
  GroundStepArgs a;
  a.lvl = q.lvl.as<uint2>();
  a.rec = q.rec.as<uint2>();
  a.nx = nx, a.ny = ny;
  a.n_cols = nx * ny; // (fits: ground_check refuses more than 2^32 - 1 columns)
  for (uint64_t c0 = 0; c0 < (uint64_t)a.n_cols; c0 += GROUND_PER_LAUNCH)
  {
    a.col0 = (uint32_t)c0;
    const uint32_t cols = (uint32_t)std::min<uint64_t>((uint64_t)a.n_cols - c0, GROUND_PER_LAUNCH);
    hipLaunchKernelGGL(ground_steps_kernel, dim3((cols + 255u) / 256u), dim3(256), 0, s, a);
  }
  q.timer.mark(2, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

// Pass 0 of a column distance field over the records of a ground result (events 0, 1 of d): the site counter is cleared in front of it.
int launch_ground_sites(hipStream_t s, const GroundResult &q, DistResult &d, uint32_t max_step, int32_t R, uint32_t flags)
{
  GroundSiteArgs a;
  a.rec = q.rec.as<uint2>();
  a.out = d.rec.as<uint32_t>();
  a.plane = d.plane.as<uint16_t>();
  a.sites = d.sites.dev;
  a.n_cols = (uint32_t)q.n;
  a.max_step = max_step;
  a.r2 = (uint32_t)(R * R);
  a.unknown_occ = (flags & WS_DISTANCE_UNKNOWN_OCCUPIED) != 0 ? 1u : 0u;
  WS_HIP(hipMemsetAsync(a.sites, 0, sizeof(unsigned long long), s));
  d.timer.mark(0, s);
  for (uint64_t c0 = 0; c0 < (uint64_t)a.n_cols; c0 += GROUND_PER_LAUNCH)
  {
    a.col0 = (uint32_t)c0;
    const uint32_t cols = (uint32_t)std::min<uint64_t>((uint64_t)a.n_cols - c0, GROUND_PER_LAUNCH);
    hipLaunchKernelGGL(ground_sites_kernel, dim3((cols + 255u) / 256u), dim3(256), 0, s, a);
  }
  d.timer.mark(1, s);
  return WS_OK;
}

} // namespace ws
