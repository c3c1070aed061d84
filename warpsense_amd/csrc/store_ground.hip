// store_ground.hip — pass 1 of the ground layer of the chunk store (ws_store_ground, include/warpsense_hip.h): the levels of
// map_ground.hip, read straight out of the 64^3 chunks of the global map in device memory, wherever they lie.  Pass 2 and the bridge to
// the distance field are those of map_ground.hip (ground_steps, launch_ground_sites), on the same records.
//
//   store_ground_levels_kernel   the shape of store_dist_classify_kernel<true>: a wave per (x, y) column of the box, four columns of
//                                consecutive y per workgroup, lane = z.  The wave walks z DOWN in chunk-aligned steps of 64: a chunk
//                                row of 64 z voxels is ONE wave-wide, 256-byte aligned load, two ballots turn it into the OCCUPIED and
//                                the FREE word of the step, and the rest is scalar bit arithmetic on them (ws_ground.h).  The words of
//                                the step above are carried, with the value of its voxel 0: a level at lz = 63 and headroom across a
//                                chunk border need no second load.
//
// A voxel of an absent chunk is unknown, whatever the store's fill entry is; the lookup is that of store_distance.hip, one per step.
// The walk keeps to the z range of the listed chunks, cut to the box.  What the box holds beyond it is unknown: it cannot carry a
// level, and as headroom it matters in the one step above the walk only, whose word is the box's own mask.
// Integers only, plain launches on the context's stream; the atomics are the class counters (one add per workgroup and class).
#include "ws_device.h"
#include "ws_ground.h"

namespace ws
{
struct StoreGroundArgs
{
  int32_t lo[3];
  int32_t hi_z;
  int32_t zlo, zhi;       // the z range of the listed chunks, cut to the box (zlo > zhi: none)
  uint32_t ny;
  uint32_t col0, n_cols;  // first column of this launch, columns of the box
  int32_t H;              // clear_vox
  uint32_t flags;
  uint2 *lvl;             // {z, word} per column
  unsigned long long *counts; // [4]
  const StoreRaySlot *table;
  uint32_t mask;          // table places - 1
  uint32_t *const *segs;  // base pointers of the store's segments
  uint32_t seg_shift;
};

__global__ __launch_bounds__(256) void store_ground_levels_kernel(StoreGroundArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t col64 = (uint64_t)a.col0 + (uint64_t)blockIdx.x * 4u + (uint64_t)wave;
  const bool active = col64 < (uint64_t)a.n_cols; // (the same for the whole wave)
  const bool any_weight = (a.flags & WS_GROUND_ANY_WEIGHT) != 0, unknown_ok = (a.flags & WS_GROUND_UNKNOWN_HEADROOM) != 0, top = (a.flags & WS_GROUND_TOP) != 0;
  int32_t level_z = 0;
  uint32_t word = 0;
  if (active && a.zlo <= a.zhi)
  {
    const uint32_t col = (uint32_t)col64;
    const uint32_t xr = col / a.ny, yr = col - xr * a.ny;
    const int32_t x = (int32_t)((int64_t)a.lo[0] + (int64_t)xr), y = (int32_t)((int64_t)a.lo[1] + (int64_t)yr); // voxels of the box
    const int32_t cx = x >> 6, cy = y >> 6;
    const uint32_t row = ((uint32_t)x & 63u) * (uint32_t)(STORE_CS * STORE_CS) + ((uint32_t)y & 63u) * (uint32_t)STORE_CS;
    const int64_t lo_z = a.lo[2], hi_z = a.hi_z;
    bool found = false, any_occ = false, any_fre = false;
    int32_t v0 = 0, v1 = 0;
    const int32_t c_lo = a.zlo >> 6, c_hi = a.zhi >> 6;
    // the step above the walk: no listed chunk, so nothing FREE; what the box holds of it is UNKNOWN
    uint64_t fre_above = 0ull, acc_above = unknown_ok ? ground_in_box(((int64_t)c_hi + 1) * STORE_CS, lo_z, hi_z) : 0ull;
    int32_t first_above = 0; // the value of voxel 0 of the step above
    for (int32_t cz = c_hi;; --cz)
    {
      const int64_t base = (int64_t)cz * STORE_CS; // (keys are floor(int32 / 64): 64 k + 63 fits)
      const uint64_t box = ground_in_box(base, lo_z, hi_z);
      const uint32_t slot = store_ray_find(a.table, a.mask, cx, cy, cz); // (uniform)
      uint32_t raw = 0u; // (an absent chunk and a voxel outside the box: weight 0, neither of the two ballots)
      if (slot != STORE_ABSENT)
      {
        const uint32_t *p = a.segs[slot >> a.seg_shift] + (size_t)(slot & ((1u << a.seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS + row;
        if ((box >> lane) & 1ull) raw = p[lane];
      }
      const uint32_t cls = dist_class(raw, any_weight);
      const uint64_t occ = __ballot(cls == 2u), fre = __ballot(cls == 1u);
      const uint64_t acc = unknown_ok ? box & ~occ : fre;
      const uint64_t levels = ground_levels(occ, fre, acc, fre_above, acc_above, a.H);
      any_occ = any_occ || occ != 0ull;
      any_fre = any_fre || fre != 0ull;
      if (levels != 0ull)
      {
        const int32_t b = ground_pick(levels, top);
        v0 = entry_value(ground_lane(raw, b));
        v1 = b == 63 ? first_above : entry_value(ground_lane(raw, b + 1));
        level_z = (int32_t)(base + b);
        found = true;
        if (top) break; // the highest level of the column
      }
      fre_above = fre, acc_above = acc;
      first_above = entry_value(ground_lane(raw, 0));
      if (cz == c_lo) break;
    }
    word = found ? ground_word(ground_frac(v0, v1), 0u, GROUND_GROUND) : ground_word(0u, 0u, ground_no_level(any_occ, any_fre));
  }
  ground_publish(a.lvl, a.counts, active, col64, level_z, word);
}

// the table's upload, the class counters' clearing, then pass 1 (events 0, 1) in launches of at most GROUND_PER_LAUNCH columns
int launch_store_ground_levels(ws_store *st, ws_store::Ground &q, const StoreDistCall &c, int32_t H, uint32_t flags)
{
  StoreGroundArgs a;
  for (int k = 0; k < 3; ++k) a.lo[k] = c.lo[k];
  a.hi_z = c.hi[2];
  a.zlo = c.zlo, a.zhi = c.zhi;
  a.ny = c.ny;
  a.n_cols = c.nx * c.ny;
  a.H = H;
  a.flags = flags;
  a.lvl = q.lvl.as<uint2>();
  a.counts = q.counts.dev;
  a.table = q.table_dev.as<StoreRaySlot>();
  a.mask = (uint32_t)store_ray_table_slots(c.n_chunks) - 1u;
  a.segs = st->seg_tab.as<uint32_t *>();
  a.seg_shift = st->seg_shift;
  hipStream_t s = st->ctx->stream;
  if (c.n_chunks)
    WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_ray_table_slots(c.n_chunks) * sizeof(StoreRaySlot), hipMemcpyHostToDevice, s));
  WS_HIP(hipMemsetAsync(a.counts, 0, 4 * sizeof(unsigned long long), s));
  q.timer.mark(0, s);
  for (uint64_t c0 = 0; c0 < (uint64_t)a.n_cols; c0 += GROUND_PER_LAUNCH)
  {
    a.col0 = (uint32_t)c0;
    const uint32_t cols = (uint32_t)std::min<uint64_t>((uint64_t)a.n_cols - c0, GROUND_PER_LAUNCH);
    hipLaunchKernelGGL(store_ground_levels_kernel, dim3((cols + 3u) / 4u), dim3(256), 0, s, a);
  }
  q.timer.mark(1, s);
  return WS_OK;
}

} // namespace ws
