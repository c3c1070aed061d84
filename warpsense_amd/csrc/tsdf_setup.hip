// tsdf_setup.hip — set-up of the TSDF scatter (gfx950): the preparation pass (everything the scatter expects to be zero), the per-ray
// constants with the rays' bound on their records, and the sort of the rays by the cell their end lies in.  (Survey: tsdf_update.hip.)
#include "tsdf_scatter.h"

namespace ws
{
size_t ray_setup_bytes() { return sizeof(RaySetup); }

// everything the scatter expects to be zero / empty, in ONE launch (after map creation and after the buffers were resized:
// in steady state every kernel of a scan puts back the scratch it has consumed, there is no clean-up launch)
struct PrepArgs
{
  TsdfCounters *counters;
  uint32_t *az_hist;
  uint32_t n_hist;
  uint32_t *tile_nsub;
  uint8_t *tile_dirty;
  int64_t n_tiles;
  unsigned long long *big_keys;
  uint32_t big_slots;
};
__global__ __launch_bounds__(256) void scatter_prep_kernel(PrepArgs p)
{
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  if (tid < (int64_t)(offsetof(TsdfCounters, last_records) / 4)) reinterpret_cast<uint32_t *>(p.counters)[tid] = 0;
  if (tid == 0) p.counters->abort = p.counters->error = 0;
  for (int64_t i = tid; i < p.n_hist; i += stride) p.az_hist[i] = 0;
  for (int64_t i = tid; i < p.n_tiles; i += stride) p.tile_nsub[i] = 0;
  for (int64_t i = tid; i < (int64_t)(2 * tile_flag_plane_bytes(p.n_tiles)); i += stride) p.tile_dirty[i] = 0;
  uint32_t *big_vals = reinterpret_cast<uint32_t *>(p.big_keys + p.big_slots);
  for (int64_t i = tid; i < p.big_slots; i += stride)
  {
    p.big_keys[i] = KEY_INF;
    big_vals[i] = 0;
  }
}

// Upper bound of the scatter targets of the ray steps [k0, k1): sum of iter_steps = 2*delta_z/res + 1 (update_tsdf.cu:101-102)
// = (k1 - k0) + sum_j #{steps with delta_z >= ceil(j*res/2)}.  Exact when every sample is a candidate; additive over ranges.
// fan_steps[j] = first step k with delta_z(len_k) >= ceil(j*res/2), len_k = 1 + k*(res/2): a function of res alone, tabulated
// on the host when the map is created (fill_fan_steps) -- two 64-bit divisions per j and ray otherwise.
__device__ __forceinline__ unsigned long long tail_bound(int64_t k0, int64_t k1, int64_t len_end, const int32_t *fan_steps)
{
  if (k1 <= k0) return 0;
  unsigned long long ub = (unsigned long long)(k1 - k0);
  if ((int64_t)DZ_PER_DISTANCE * len_end >= (1ll << 31)) return ub * 256; // DZ * len wraps in the reference's int: any fan width the key admits
  for (int j = 1; j < 256; ++j)
  {
    const int64_t kj = fan_steps[j];
    if (kj >= k1) break; // non-decreasing in j
    ub += (unsigned long long)(k1 - (kj > k0 ? kj : k0));
  }
  return ub;
}

// update_tsdf.cu:52-63 for one ray per lane, plus the split of the ray into free-space steps and tail
__device__ __forceinline__ void ray_setup_block(const ScatterArgs &a)
{
  __shared__ unsigned long long ub_wave[4];
  __shared__ uint32_t s_bkey[512], s_bcnt[512]; // bins of this workgroup's rays: key, count (then: first rank)
  __shared__ int32_t s_fan[256];                // fan_steps (tail_bound walks it entry by entry: a chain of dependent loads from memory otherwise)
  s_bkey[threadIdx.x] = s_bkey[threadIdx.x + 256] = 0xffffffffu;
  s_bcnt[threadIdx.x] = s_bcnt[threadIdx.x + 256] = 0;
  s_fan[threadIdx.x] = a.fan_steps[threadIdx.x];
  __syncthreads();
  uint32_t my_bin = 0;
  const uint32_t ix = blockIdx.x * 256u + threadIdx.x;
  if (ix == 0)
  {
    // what the marches of this scan count up (the previous scan's integrate pass has read its tile list by now)
    a.counters->chunk_cursor = 0;
    a.counters->free_cursor = 0;
    a.counters->n_listed = 0;
    a.counters->n_appended = 0;
    a.counters->abort = 0; // (set by later launches only: the key-range verdict of this pass goes to range_seq)
    a.counters->last_free_keyed = 0;
    a.counters->last_unlisted = 0;
  }
  RaySetup r;
  r.dx = r.dy = r.dz = r.distance = r.ivx = r.ivy = r.ivz = r.steps = 0;
  r.div_m = 0;
  r.spare = 0;
  r.div_k = 0;
  r.pad = 0;
  r.kfirst = 0;
  r.ub = 0;
  const int32_t res = a.res, tau = a.tau, half = res / 2;
  const bool frame_biased_ok = make_march_frame(a.scanner_pos, res, tau, a.map).biased_ok;
  bool ok = false;
  int32_t px = 0, py = 0, pz = 0;
  int32_t hvx = 0, hvy = 0, hvz = 0; // voxel of the scan point
  if (ix < a.n)
  {
    px = a.xyz[3 * (size_t)ix + 0];
    py = a.xyz[3 * (size_t)ix + 1];
    pz = a.xyz[3 * (size_t)ix + 2];
    if (a.xyz_keep)
    {
      // (the verdict on the record pool comes after ws_tsdf_update_dev has returned; a repeat must not depend on what
      // the caller has done with its buffer since)
      a.xyz_keep[3 * (size_t)ix + 0] = px;
      a.xyz_keep[3 * (size_t)ix + 1] = py;
      a.xyz_keep[3 * (size_t)ix + 2] = pz;
    }
    // cu_to_map (cuda/util.h:111-114) + in_bounds_with_buffer_pos (update_tsdf.cu:55)
    const float fr = (float)res;
    const int32_t cx = (int32_t)floorf(__fdiv_rn((float)px, fr));
    const int32_t cy = (int32_t)floorf(__fdiv_rn((float)py, fr));
    const int32_t cz = (int32_t)floorf(__fdiv_rn((float)pz, fr));
    ok = in_bounds_buffer(a.map, cx, cy, cz, (int64_t)(tau / res / 2));
    hvx = cx;
    hvy = cy;
    hvz = cz;
  }
  if (ok)
  {
    // cu_to_mm (cuda/util.h:116-123)
    const int32_t posx = wadd(wmul(a.scanner_pos[0], res), half);
    const int32_t posy = wadd(wmul(a.scanner_pos[1], res), half);
    const int32_t posz = wadd(wmul(a.scanner_pos[2], res), half);
    const int32_t dx = wsub(px, posx), dy = wsub(py, posy), dz = wsub(pz, posz);
    const int32_t distance = l2norm_i(dx, dy, dz);
    // distance == 0: guard (the reference divides by zero here; src/cpu/update_tsdf.cpp:593 has the guard)
    if (distance > 0)
    {
      // update_tsdf.cu:59-63, in int64 like the reference's `long`
      const int64_t MR = MATRIX_RESOLUTION;
      const int64_t ndx = div_trunc_i64(wmul64(dx, MR), distance), ndy = div_trunc_i64(wmul64(dy, MR), distance), ndz = div_trunc_i64(wmul64(dz, MR), distance);
      const int64_t ux = a.up[0], uy = a.up[1], uz = a.up[2];
      const int64_t c1x = wsub64(wmul64(ndy, uz), wmul64(ndz, uy)) / MR;
      const int64_t c1y = wsub64(wmul64(ndz, ux), wmul64(ndx, uz)) / MR;
      const int64_t c1z = wsub64(wmul64(ndx, uy), wmul64(ndy, ux)) / MR;
      int64_t ivx = wsub64(wmul64(ndy, c1z), wmul64(ndz, c1y));
      int64_t ivy = wsub64(wmul64(ndz, c1x), wmul64(ndx, c1z));
      int64_t ivz = wsub64(wmul64(ndx, c1y), wmul64(ndy, c1x));
      const int64_t inorm = l2norm_l(ivx, ivy, ivz);
      if (inorm != 0) // guard (src/cpu/update_tsdf.cpp:602)
      {
        ivx = div_trunc_i64(wmul64(ivx, MR), inorm);
        ivy = div_trunc_i64(wmul64(ivy, MR), inorm);
        ivz = div_trunc_i64(wmul64(ivz, MR), inorm);
        const int64_t len_end = (int64_t)distance + tau;
        const int64_t steps = div_trunc_i64(len_end - 1, half) + 1;
        const int64_t max_delta_z = (int64_t)DZ_PER_DISTANCE * len_end / MATRIX_RESOLUTION;
        const bool small_iv = ivx >= INT32_MIN && ivx <= INT32_MAX && ivy >= INT32_MIN && ivy <= INT32_MAX && ivz >= INT32_MIN && ivz <= INT32_MAX;
        if (steps > (int64_t)(1 << (a.rec_fmt & 0xffu)) || (max_delta_z * 2) / res + 1 > (int64_t)((1 << (a.rec_fmt >> 8)) - 1) || !small_iv)
        {
          // Outside the range of the record's step / fan fields for a scan of this many points.  With the widest split (scans of
          // up to 16 384 points: 65 536 steps, 255 fan steps) that is the end: the ray is dropped and the error is sticky.  A
          // larger scan is ABORTED instead (range_seq = scan_seq; nothing of it reaches the maps) and the host repeats it in
          // pieces of 16 384 points, each with the widest split, one after the other into new_map (settle_tsdf: the serial order
          // is the order of the points, so consecutive pieces folded on top of each other are the same schedule).
          if ((a.rec_fmt & 0xffu) == 16u && (a.rec_fmt >> 8) == 8u)
            raise_error(a.counters, a.status, ERR_RANGE);
          else
            __hip_atomic_store(&a.counters->range_seq, a.scan_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        else
        {
          r.dx = dx; r.dy = dy; r.dz = dz;
          r.distance = distance;
          r.ivx = (int32_t)ivx; r.ivy = (int32_t)ivy; r.ivz = (int32_t)ivz;
          r.steps = (int32_t)steps;
          const FastDiv fd = make_fastdiv_dev(distance);
          r.div_m = (uint32_t)fd.M; // (below 2^32: make_fastdiv)
          r.div_k = fd.k;
          // conditions of march_steps_fast (ws_march.h): no int32 wrap in d*len, pos + d, voxel centres,
          // delta_z*iv and step*res*iv, nor in the squared distance to the hit point (|p - centre| <= len_end + 2 res)
          const int64_t dmax = max(max(llabs((long long)dx), llabs((long long)dy)), llabs((long long)dz));
          const int64_t pmax = max(max(llabs((long long)posx), llabs((long long)posy)), llabs((long long)posz));
          const int64_t ivmax = max(max(llabs(ivx), llabs(ivy)), llabs(ivz));
          // dmax <= distance: beyond ~46 m the reference's int sum of squares wraps and `distance` is not the length
          // of the ray any more — the walk's "less than one voxel per step" then fails
          // (res * distance < 2^32: the column-change walk keeps W = res * dist in 32 bits, ws_dda.h -- ADVICE r5; only a map of
          // metre-sized voxels gets near it)
          const bool fast = dmax <= distance && dmax * len_end < (1ll << 31) && pmax + dmax + 2 * (int64_t)res + tau < (1ll << 30) &&
                            (int64_t)res * distance < (1ll << 32) &&
                            (2 * max_delta_z + res) * ivmax < (1ll << 31) &&
                            (len_end + 2 * (int64_t)res) * (len_end + 2 * (int64_t)res) < (1ll << 31);
          r.pad = fast ? RAY_FAST : 0;
          {
            // the whole ray, its fans included, inside the window with room to spare: the per-candidate in_bounds tests
            // (update_tsdf.cu:73,113) cannot fail.  Both ends inside a box shrunk by the fan reach (convexity does the rest).
            const int64_t margin = 4 + (max_delta_z + res) / res;
            const int64_t endx = (int64_t)posx + div_trunc_i64((int64_t)dx * len_end, distance), endy = (int64_t)posy + div_trunc_i64((int64_t)dy * len_end, distance),
                          endz = (int64_t)posz + div_trunc_i64((int64_t)dz * len_end, distance);
            const int64_t ev[3] = {div_trunc_i64(endx, res), div_trunc_i64(endy, res), div_trunc_i64(endz, res)};
            bool inside = fast && frame_biased_ok; // (div_res_b / ring_b, ws_march.h: the window's coordinates fit their bias)
            for (int k = 0; k < 3; ++k)
            {
              const int64_t lim = (int64_t)(a.map.size[k] / 2) - margin;
              inside = inside && llabs((long long)((int64_t)a.scanner_pos[k] - a.map.pos[k])) <= lim && llabs((long long)(ev[k] - a.map.pos[k])) <= lim;
            }
            if (inside) r.pad |= RAY_SIMPLE;
          }

          // Split of the ray.  A candidate is "free space" iff its value is +tau: the on-ray one is (tau, +64), the off-ray
          // ones of its fan (tau, -64), whichever ray they come from -- so neither needs a record: the first is a byte per voxel
          // (its order only matters on a voxel that also has records: earliest key, free-space hash), the second never takes
          // part in the order at all (|value| == tau cannot block a positive candidate, and it only wins where nothing else
          // landed: a second byte plane).  ALL candidates of a ray are of that kind while len < distance - tau - slack: a
          // voxel centre further than tau from the hit point gives min(dist, tau) == tau.  The slack covers |centre - proj|
          // (1.5 voxels per axis for the double-width cell of trunc division + the fan offset).  The bound argues with
          // exact positions: rays whose `int` products wrap (not `fast`) and scans into a non-default new_map send every
          // step through the order keys.  (Until round 3 the tail also began at the first step with a fan, 8.2 m at 50 mm:
          // a quarter of the benchmark scan's records were free space with a fan.)
          int32_t kfirst = 0;
          if (fast && !a.all_keyed)
          {
            const int32_t keyed_len = min(a.keyed_len_neg, distance - tau - a.keyed_slack);
            kfirst = keyed_len > 1 ? max(0, (keyed_len - 1) / half - 1) : 0;
            if (kfirst > (int32_t)steps) kfirst = (int32_t)steps;
          }
          r.kfirst = kfirst;
          // records this ray can make: the scatter targets of its tail + one per free-space step (a free-space candidate that
          // lands on a voxel with records joins them)
          const unsigned long long ub = tail_bound(kfirst, steps, len_end, s_fan) + (unsigned long long)kfirst;
          r.ub = ub > 0xffffffffull ? 0xffffffffu : (uint32_t)ub;
        }
      }
    }
  }
  // Sort bin of the ray; bin AZ_BINS = unused ray.  The tails are sorted by WHERE THE RAY ENDS -- the tail of a ray lies within
  // tau of its end, so the 64 rays of a wave of the tail march put their records into the few tiles around one cell -- in
  // polar cells around the sensor (16 rings x 256 sectors, above / below the sensor), the FAR rings first: see below.
  // (Rounds 1-3 sorted by direction, 1024 azimuths x 8 elevations: rays of one direction bin that graze the floor end metres
  // apart -- 435 k (wave, tile) pairs per scan; a 64 x 64 grid of square cells in Morton order: 297 k, tail march 178 us; the
  // polar cells: 244 k, 146 us -- two thirds of that gain is the order of the work items.)
  if (ix < a.n)
  {
    uint32_t bin = AZ_BINS;
    if (r.steps > 0)
    {
      const int32_t cwx = (a.map.size[0] + 63) / 64, cwy = (a.map.size[1] + 63) / 64;
      int bx = (hvx - a.map.pos[0] + a.map.size[0] / 2) / cwx, by = (hvy - a.map.pos[1] + a.map.size[1] / 2) / cwy;
      bx = bx < 0 ? 0 : (bx > 63 ? 63 : bx);
      by = by < 0 ? 0 : (by > 63 ? 63 : by);
      // polar cells around the sensor -- WS_SORT_RINGS rings x 4096 / WS_SORT_RINGS sectors, above / below -- the FAR rings first: rays that end far away
      // carry fans (up to three times the records), and work items in descending order of their length leave the shortest
      // for the end of the launch, when the compute units run empty
      const float fdx = (float)r.dx, fdy = (float)r.dy;
      constexpr int RINGS = WS_SORT_RINGS, SECTORS = 4096 / RINGS;
      const float ringw = (float)(a.map.size[0] > a.map.size[1] ? a.map.size[0] : a.map.size[1]) * (float)res * (0.5f / (float)RINGS);
      int ring = (int)(sqrtf(fdx * fdx + fdy * fdy) / ringw);
      ring = ring < 0 ? 0 : (ring > RINGS - 1 ? RINGS - 1 : ring);
      int sec = (int)((atan2f(fdy, fdx) + 3.14159265f) * ((float)SECTORS / 6.2831853f));
      sec = sec < 0 ? 0 : (sec > SECTORS - 1 ? SECTORS - 1 : sec);
      bin = (uint32_t)(((RINGS - 1 - ring) * 2 + (hvz >= a.scanner_pos[2] ? 1 : 0)) * SECTORS + sec);
      (void)bx;
      (void)by;
    }
    r.pad |= (int32_t)(bin << 1); // bits 1 .. 14 (RAY_SIMPLE is bit 30)
    my_bin = bin;
    a.rays[ix] = r;
  }
  // The ray's rank inside its bin comes from the bin's counter (the sort blocks place it without a second atomic) -- through
  // the workgroup: its rays count themselves per bin in LDS first, and ONE add per (workgroup, bin) reserves their ranks.  A
  // cell near the sensor holds thousands of rays, and a returning atomic per ray on such a counter took the set-up pass from
  // 30 to 69 us; the 256 rays of a workgroup are neighbours in the scan and share a few dozen bins.  (It also keeps such
  // neighbours together in the sorted order.)  Everything travels at agent scope (performed at the coherent level): the
  // sort blocks run on other XCDs in the next launch.
  __syncthreads(); // (the table was emptied on entry)
  int my_slot = -1;
  uint32_t my_lrank = 0;
  if (ix < a.n)
  {
    uint32_t h = (my_bin * 0x9E3779B1u) >> (32 - 9);
    for (;;)
    {
      const uint32_t cur = s_bkey[h];
      if (cur == my_bin) break;
      if (cur == 0xffffffffu)
      {
        const uint32_t old = atomicCAS(&s_bkey[h], 0xffffffffu, my_bin);
        if (old == 0xffffffffu || old == my_bin) break;
      }
      h = (h + 1) & 511u;
    }
    my_slot = (int)h;
    my_lrank = atomicAdd(&s_bcnt[h], 1u);
  }
  // The records this scan can make (sum of the per-ray bounds): every scan sizes the record buffers itself.
  unsigned long long ub = r.ub;
  for (int d = 32; d > 0; d >>= 1) ub += __shfl_down(ub, d, 64);
  if ((threadIdx.x & 63) == 0) ub_wave[threadIdx.x >> 6] = ub;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 2; ++q)
  {
    const int sl = (int)threadIdx.x + 256 * q;
    const uint32_t c = s_bcnt[sl];
    if (c) s_bcnt[sl] = __hip_atomic_fetch_add(&a.az_hist[s_bkey[sl]], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (my_slot >= 0)
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(&a.ray_bin[ix]), (unsigned long long)my_bin | ((unsigned long long)(s_bcnt[my_slot] + my_lrank) << 32),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // one fire-and-forget add per workgroup; the direction sort -- the next launch -- hands the total to the host
  if (threadIdx.x == 0) atomicAdd(&a.counters->ub_total, ub_wave[0] + ub_wave[1] + ub_wave[2] + ub_wave[3]);
}

// Counting sort of the rays by direction bin (a launch of its own behind the set-up pass: fused into it, with the sort
// blocks waiting for the set-up blocks' arrival count, it measured 50 us against 37 for two launches -- the waiting blocks'
// polls queue in front of the adds they wait for).  Every sort block scans the 8193-entry histogram itself (32 KB, one block
// scan).  Block 0 also hands the scan's record bounds to the host (host-mapped memory: the values, then the sequence number
// the host spins on), which sizes the buffers before the marches may do anything -- the capacity never rests on a guess.
__global__ __launch_bounds__(256) void ray_sort_kernel(ScatterArgs a)
{
  __shared__ uint32_t s_off[AZ_BINS + 2];
  __shared__ uint32_t wave_sums[4];
  constexpr int TOTAL = AZ_BINS + 1;
  constexpr int PER = (TOTAL + 255) / 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(a.status + 4), a.counters->ub_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(a.status + 6, a.scan_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const int lo = threadIdx.x * PER, hi = min(lo + PER, TOTAL);
  uint32_t h[PER];
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j)
  {
    const int i = lo + j;
    h[j] = i < hi ? a.az_hist[i] : 0u;
    v += h[j];
  }
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wave_sums[wave] = x;
  __syncthreads();
  uint32_t run = x - v;
  for (int w = 0; w < wave; ++w) run += wave_sums[w];
#pragma unroll
  for (int j = 0; j < PER; ++j)
  {
    const int i = lo + j;
    if (i < hi) s_off[i] = run;
    run += h[j];
  }
  if (hi == TOTAL && lo < hi) s_off[TOTAL] = run;
  __syncthreads();
  const uint32_t b = blockIdx.x, nb = gridDim.x;
  if (b == 0 && threadIdx.x == 0) a.az_off[AZ_BINS] = s_off[AZ_BINS]; // rays that contribute: the tail march's grid
  // (four rays per trip, their loads in flight together: one after the other the trips were a chain of memory round trips)
  for (uint32_t ix0 = b * 256u + threadIdx.x; ix0 < a.n; ix0 += nb * 256u * 4u)
  {
    unsigned long long br[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u)
    {
      const uint32_t ix = ix0 + u * nb * 256u;
      br[u] = *reinterpret_cast<const unsigned long long *>(&a.ray_bin[ix < a.n ? ix : ix0]);
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u)
    {
      const uint32_t ix = ix0 + u * nb * 256u;
      if (ix < a.n) a.ray_order[s_off[(uint32_t)br[u]] + (uint32_t)(br[u] >> 32)] = ix;
    }
  }
}
__global__ __launch_bounds__(256) void ray_setup_kernel(ScatterArgs a) { ray_setup_block(a); }

constexpr int PREP_GRID = 512;
static PrepArgs make_prep_args(ws_map *m)
{
  PrepArgs p;
  p.counters = m->counters.as<TsdfCounters>();
  p.az_hist = m->az_hist.as<uint32_t>();
  p.n_hist = (uint32_t)(AZ_BINS + 1);
  p.tile_nsub = m->tile_nsub.as<uint32_t>();
  p.tile_dirty = m->tile_dirty.as<uint8_t>();
  p.n_tiles = m->n_tiles;
  p.big_keys = m->big_keys.as<unsigned long long>();
  p.big_slots = m->big_slots;
  return p;
}
void enqueue_scatter_prep(ws_map *m, hipStream_t s)
{
  hipLaunchKernelGGL(scatter_prep_kernel, dim3(PREP_GRID), dim3(256), 0, s, make_prep_args(m));
  m->status.as<uint32_t>()[10] = 0;
}
int launch_scatter_prep(ws_map *m)
{
  enqueue_scatter_prep(m, m->ctx->stream);
  WS_HIP(hipGetLastError());
  m->prepped = true;
  return WS_OK;
}
// the set-up pass and, behind it, the sort (a launch of its own: ray_sort_kernel)
void launch_ray_setup(const ScatterArgs &sa, hipStream_t s)
{
  const dim3 block(256);
  const dim3 grid_setup((unsigned)(((size_t)sa.n + 255) / 256));
  hipLaunchKernelGGL(ray_setup_kernel, grid_setup, block, 0, s, sa);
  hipLaunchKernelGGL(ray_sort_kernel, dim3(min(grid_setup.x, (unsigned)WS_SORT_BLOCKS)), block, 0, s, sa);
}

// fan_steps[j] of tail_bound for one resolution (host side, once per map).  j = 0 is unused.
void fill_fan_steps(int32_t *fan_steps, int32_t res, int32_t ntz, int32_t nty)
{
  {
    // behind the fan table: the multiply-shift constants of the divisions by ntz and nty (tile id -> tile coordinates when a tile
    // goes on the scan's list, list_tile: two general 32-bit divisions per listed tile otherwise)
    const FastDiv dz = make_fastdiv(ntz), dy = make_fastdiv(nty);
    fan_steps[256] = (int32_t)(uint32_t)dz.M;
    fan_steps[257] = dz.k - 32; // (-1 for a divisor of 1: the quotient is the dividend)
    fan_steps[258] = (int32_t)(uint32_t)dy.M;
    fan_steps[259] = dy.k - 32;
  }
  const int64_t half = res / 2 > 0 ? res / 2 : 1;
  fan_steps[0] = 0;
  for (int64_t j = 1; j < 256; ++j)
  {
    const int64_t cj = (j * res + 1) / 2;                                                   // delta_z that gives 2*delta_z/res >= j
    const int64_t Lj = (cj * MATRIX_RESOLUTION + DZ_PER_DISTANCE - 1) / DZ_PER_DISTANCE;   // first length with that delta_z
    const int64_t kj = (Lj - 1 + half - 1) / half;                                          // first step with len_k >= Lj
    fan_steps[j] = (int32_t)(kj > (1ll << 30) ? (1ll << 30) : kj);                          // beyond the steps the record admits anyway
  }
}
} // namespace ws
