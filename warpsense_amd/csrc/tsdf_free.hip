// tsdf_free.hip — the free pass of the TSDF scatter (gfx950): the steps before the tails, one byte per voxel.  (Survey: tsdf_update.hip.)
#include "tsdf_pool.h"

namespace ws
{
// What a free-space candidate does to its voxel, in two halves: the byte of the voxel is REQUESTED when the candidate is
// popped from the queue and USED one emit phase later.  The free pass is not bound by instruction issue alone: shortening
// the sample phase from ~115 to ~60 instructions moved it from 137 to 126 us, taking this load's round trip off the wave's
// path to 122 us; what remains is the scattered byte traffic itself (21 M byte loads, 9 M byte stores, one cache line each).
struct FreePending
{
  uint32_t tile;
  uint32_t vox;  // voxel inside the tile (brick order: vox_of)
  uint32_t ix;   // ray
  int32_t k;     // ray step
  uint32_t b;    // the voxel's byte (in flight until the next step)
  bool valid;
};
// sx, sy, sz: storage coordinates of the candidate's voxel
template <bool SMALL>
__device__ __forceinline__ void free_request(const ScatterArgs &a, FreePending &p, bool valid, uint32_t ix, int32_t k, int32_t sx, int32_t sy, int32_t sz)
{
  p.valid = valid;
  // unconditional (clamped) load: nothing waits for it here
  p.tile = valid ? tile_of(a.nty, a.ntz, sx, sy, sz) : 0u;
  p.vox = valid ? vox_of(sx, sy, sz) : 0u;
  p.ix = ix;
  p.k = k;
  p.b = *vox_ptr<SMALL>(a.vstate, p.tile, p.vox);
}
// the sub-chunks of the records the free pass makes (one each): a wave of the compacting walk keeps the rest of the 64 it
// took from the pool (fb_next, fb_left: uniform); the general walk -- lanes in varying company -- asks for what it needs
struct FreeBlock
{
  uint32_t next, left;
};
template <bool CACHED, bool SMALL>
__device__ __forceinline__ void free_finish(const ScatterArgs &a, const FreePending &p, uint32_t &n_keyed, FreeBlock &fb)
{
  const uint32_t b = p.b;
  // (the ballot of a conjunction goes through a vector register and back -- v_cndmask + v_cmp; two ballots and a scalar AND do not)
  const unsigned long long km = __ballot(p.valid) & __ballot((b & VOX_KEYED) != 0);
  const bool keyed = p.valid && (b & VOX_KEYED);
  if (km)
  {
    // the voxel also has ordered candidates (from the tails): this one, (tau, +64) at its place in the order, joins the
    // records of the tile (25 000 of the benchmark scan's 21 million free-space candidates)
    const int lane = threadIdx.x & 63;
    const uint32_t n = (uint32_t)__popcll(km);
    const int leader = __ffsll((long long)km) - 1;
    uint32_t first;
    if (CACHED)
    {
      if (fb.left < n)
      {
        uint32_t g = 0;
        if (lane == leader) g = free_grab(a, 64u);
        fb.next = (uint32_t)__builtin_amdgcn_readlane((int)g, leader);
        fb.left = fb.next == SUB_LOST ? 0u : 64u;
      }
      first = fb.left ? fb.next : SUB_LOST;
      if (fb.left)
      {
        fb.next += n;
        fb.left -= n;
      }
    }
    else
    {
      uint32_t g = 0;
      if (lane == leader) g = free_grab(a, n);
      first = (uint32_t)__builtin_amdgcn_readlane((int)g, leader);
    }
    if (keyed)
    {
      const uint32_t id = first == SUB_LOST ? SUB_LOST : first + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
      // (the answer of the atomic in there picked up one emit phase later, under the next batch's voxel bytes: no gain, measured)
      append_single(a, p.tile, id, make_rec(p.ix, p.k, 0, a.tau, local_of_vox(p.vox), REC_S(a), REC_F(a)));
      n_keyed += 1;
    }
  }
  if (p.valid && b == 0)
  {
    // free space only (the common case): the result will be (tau, 64) whoever comes first.  (Two candidates of one voxel
    // whose loads both saw 0 both store: idempotent.)
    *vox_ptr<SMALL>(a.vstate, p.tile, p.vox) = VOX_TOUCHED;
    // (remembering the tiles a workgroup has marked in an LDS set instead of this load: 126 -> 140 us, measured; an atomic
    // that puts the tile on the scan's list at its first mark: 123 -> 355 us -- the load sees stale zeros from the L1 of its
    // compute unit all through the kernel, harmless for a byte store, a blocking round trip for a returning atomic)
    if (a.tile_dirty[p.tile] == 0) a.tile_dirty[p.tile] = 1;
  }
}
// both halves at once (general walk)
template <bool SMALL>
__device__ __forceinline__ void free_emit(const ScatterArgs &a, const MarchFrame &f, uint32_t ix, int32_t k, int32_t vx, int32_t vy, int32_t vz, uint32_t &n_keyed)
{
  FreePending p;
  FreeBlock none = {0, 0};
  free_request<SMALL>(a, p, true, ix, k, ring_fast(vx, f.ringK[0], a.map.size[0]), ring_fast(vy, f.ringK[1], a.map.size[1]),
                      ring_fast(vz, f.ringK[2], a.map.size[2]));
  free_finish<false, SMALL>(a, p, n_keyed, none);
}

#ifndef WS_FREE_LANES
#define WS_FREE_LANES 4
#endif
constexpr int FREE_LANES = WS_FREE_LANES; // lanes that share the free-space part of one ray

// 64 rays per workgroup, 4 lanes per ray (round 2 walk: 32 lanes 163 us, 16: 146, 8: 141, 4: 147, 1: 280; round 3 walk: 8: 123, 4: 120, 2: 131): lane c walks the steps [c*CH, (c+1)*CH) of the free-space part of its ray,
// so every lane has the same amount of work whatever the ray length.  Waves whose rays are all RAY_SIMPLE use the
// compacting walk (ws_march.h): samples for all lanes, candidates through a per-wave LDS queue, 64 at a time.
// (Round 4 measured the free part extended over the steps that carry a fan -- 8.2 m to the tail at 50 mm, their off-ray
// targets as marks in the second byte plane: 10.8 M records instead of 14.4 M and a tail march of 146 instead of 187 us, but
// a free pass of 195-230 instead of 123 us whatever the lane layout: out there neighbouring rays are more than a voxel
// apart, every candidate is a cold cache line, and THIS pass waits for the byte it loads where the tail march only stores.)
#ifndef WS_FREE_WGS
#define WS_FREE_WGS 6 // workgroups per CU the register budget is set for (round 5's walk over column changes, 5 / 6 / 7 / 8: 105 / 103 / 102 / 120 us;
                      // six: 80 VGPRs, one spilled outside the loops; seven: 72 with 15 spilled; round 4's stepped walk: 121 / 120 / 117 / 147)
#endif
template <bool SMALL> // SMALL: 32-bit offsets into the voxel bytes (vox_ptr)
__global__ __launch_bounds__(WS_FREE_THREADS, WS_FREE_WGS * 256 / WS_FREE_THREADS) void march_free_kernel(ScatterArgs a)
{
#ifdef WS_FREE_TIMING
  const long long t_free_begin = wall_clock64();
#endif
  if (a.counters->abort != 0 || a.counters->range_seq == a.scan_seq) return; // (out of sub-chunks, or a ray beyond the key range: the host repeats the scan)
  __shared__ uint32_t s_keyed[WS_FREE_THREADS / 64];
  const uint32_t ix = blockIdx.x * (uint32_t)(WS_FREE_THREADS / FREE_LANES) + threadIdx.x / (uint32_t)FREE_LANES;
  const int32_t c = (int32_t)(threadIdx.x % (uint32_t)FREE_LANES);
  const int lane = threadIdx.x & 63;
  uint32_t n_keyed = 0;
  RaySetup r;
  r.steps = 0;
  r.kfirst = 0;
  r.pad = 0;
  if (ix < a.n) r = a.rays[ix];
  const int32_t kend = min(r.steps, r.kfirst);
  const int32_t ch = (kend + FREE_LANES - 1) / FREE_LANES;
  const int32_t k0 = c * ch;
  const int32_t k1 = min(k0 + ch, kend);
  const bool work = k0 < k1;
  const int32_t tau = a.tau;
  const MarchFrame f = make_march_frame(a.scanner_pos, a.res, tau, a.map);
  const int32_t res = f.res, half = f.half, dist = r.distance;
  if (!__all(!work || ((r.pad & RAY_SIMPLE) && r.distance >= 2)))
  {
    // a ray of this wave wraps in int32 or leaves the window: the general walk with all its tests
    if (work)
      march_steps<true>(f, r, k0, k1, [&](int32_t k, int32_t step, int32_t vx, int32_t vy, int32_t vz, int32_t value, bool positive) {
        // every candidate of these steps is free space: on the ray, further than tau from the hit point
        if (!(positive && value == tau))
        {
          raise_error(a.counters, a.status, ERR_FREE_BOUND); // impossible by the bound; never lose a candidate silently
          return;
        }
        free_emit<SMALL>(a, f, ix, k, vx, vy, vz, n_keyed);
      });
  }
  else if (__any(work))
  {
    // One loop iteration per CANDIDATE (ws_dda.h): the lane walks from one column change of its part of the ray to the next --
    // the steps at which x or y enters a new voxel are two Bresenham sequences -- and computes the sample's position from the
    // step number by one exact multiply-shift per axis.  No sample phase, no queue: rounds 3-4 stepped every sample (613 k wave
    // iterations of ~60 instructions for the benchmark scan) and moved the 21 M candidates through LDS to 333 k emit phases of
    // ~85; this loop runs 370 k times (tools/lane_model.py: 89 % of its lane slots carry a candidate).  The voxel byte of a
    // candidate is requested in one iteration and used in the next, as before.
    FreePending pend;
    FreeBlock fblock = {a.sub_cap - (blockIdx.x * (uint32_t)(WS_FREE_THREADS / 64) + (threadIdx.x >> 6) + 1u) * FREE_WAVE_FIRST, pool_holds_static(a) ? FREE_WAVE_FIRST : 0u};
    pend.valid = false;
    pend.tile = pend.vox = pend.ix = pend.b = 0;
    pend.k = 0;
    const uint32_t adx = (uint32_t)(r.dx < 0 ? -r.dx : r.dx), ady = (uint32_t)(r.dy < 0 ? -r.dy : r.dy), adz = (uint32_t)(r.dz < 0 ? -r.dz : r.dz);
    const int32_t smx = r.dx < 0 ? -1 : 0, smy = r.dy < 0 ? -1 : 0, smz = r.dz < 0 ? -1 : 0;
    const int32_t sposx = (f.posx ^ smx) - smx, sposy = (f.posy ^ smy) - smy, sposz = (f.posz ^ smz) - smz;
    // The walk lives in MIRRORED coordinates (every axis turned so that the ray travels in the positive direction: a = s pos + q),
    // and so does the rest of the step: the fan base offset c0 = trunc(delta_z * iv / 32768) (update_tsdf.cu:103-110 with one fan
    // step) with the mirrored s iv -- delta_z >= 0, so the product's sign is s iv's and the rounding toward zero a per-ray bias in
    // front of an arithmetic shift (trunc15_biased) --, the truncating division by res (trunc is odd: trunc(e / res) = s trunc(s e /
    // res)), and the sign comes back in the ONE instruction that adds the ring buffer's constant: x = s (qm - divBq) + offset - pos =
    // (qm ^ sm) + Kc, Kc = ringB for s = +1 and ringB + 2 divBq + 1 for s = -1 (v_xad_u32).  Two instructions per axis less than
    // un-mirroring the position first.
    const int32_t ivmx = (r.ivx ^ smx) - smx, ivmy = (r.ivy ^ smy) - smy, ivmz = (r.ivz ^ smz) - smz;
    const int32_t bvx = iv_bias(ivmx), bvy = iv_bias(ivmy), bvz = iv_bias(ivmz);
    const uint32_t kcx = (uint32_t)f.ringB[0] + (smx ? 2u * (uint32_t)f.divBq + 1u : 0u), kcy = (uint32_t)f.ringB[1] + (smy ? 2u * (uint32_t)f.divBq + 1u : 0u),
                   kcz = (uint32_t)f.ringB[2] + (smz ? 2u * (uint32_t)f.divBq + 1u : 0u);
    const uint32_t hdx = adx * (uint32_t)half, hdy = ady * (uint32_t)half, hdz = adz * (uint32_t)half, dzh = (uint32_t)(DZ_PER_DISTANCE * half);
    DdaRay R;
    R.M32 = r.div_m;
    R.sh = r.div_k - 32;
    DdaAxis wx, wy;
    wx.K = wy.K = wx.Ksp = wy.Ksp = DDA_NEVER;
    wx.rho = wy.rho = wx.wq = wy.wq = wx.wr = wy.wr = 0;
    wx.D = wy.D = 1;
    uint32_t k = DDA_NEVER; // the lane's next candidate (ray step)
    if (work)
    {
      const int32_t kinit = k0 > 0 ? k0 - 1 : 0;
      const int32_t len0 = 1 + kinit * half;
      const uint32_t qx = dda_q(adx, len0, R), qy = dda_q(ady, len0, R);
      dda_axis_init(wx, adx, sposx, qx, dist, res, half);
      dda_axis_init(wy, ady, sposy, qy, dist, res, half);
      k = min(wx.K, wy.K);
      // the sample k == 0 is compared with the voxel column (0, 0) (update_tsdf.cu:65,71): a candidate of its own in front
      if (k0 == 0 && (div_res(sposx + (int32_t)qx, f) != 0 || div_res(sposy + (int32_t)qy, f) != 0)) k = 0;
    }
    // One step of the walk: finish the candidate whose voxel byte the PREVIOUS step requested (it has had a whole step to
    // arrive), request the byte of the lane's next candidate, move on to the next column change.  (gfx950 retires loads and
    // stores in order behind one counter and the stores here are under branches, so the wait for a byte is a wait for
    // everything in flight; a variant that issued the same load and two stores in every step -- `vmcnt(3)` instead -- was no
    // faster: DESIGN.md section 5.)
    auto step = [&](auto special, FreePending &req) {
      const bool active = k < (uint32_t)k1;
      // ---- the sample's position (update_tsdf.cu:69) and its single on-ray target (:103-112 with iter_steps == 1)
      // (|d| * len_k = (|d| half) k + |d|, 100 * len_k = (100 half) k + 100: one multiply-add each)
      const int32_t ax = sposx + (int32_t)dda_qn(hdx * k + adx, R), ay = sposy + (int32_t)dda_qn(hdy * k + ady, R), az = sposz + (int32_t)dda_qn(hdz * k + adz, R);
      const int32_t dz = (int32_t)(dzh * k + (uint32_t)DZ_PER_DISTANCE) >> 15; // (DZ_PER_DISTANCE * len) >> 15; no fan in the free-space part: dz * 2 < res
      const int32_t ex = ax - trunc15_biased(dz, ivmx, bvx), ey = ay - trunc15_biased(dz, ivmy, bvy), ez = az - trunc15_biased(dz, ivmz, bvz);
      free_finish<true, SMALL>(a, req, n_keyed, fblock);
      free_request<SMALL>(a, req, active, ix, (int32_t)k, ring_m(div_res_b(ex, f), (uint32_t)smx, kcx, a.map.size[0]),
                          ring_m(div_res_b(ey, f), (uint32_t)smy, kcy, a.map.size[1]), ring_m(div_res_b(ez, f), (uint32_t)smz, kcz, a.map.size[2]));
      // ---- on to the next column change
      const bool cx = active && wx.K == k, cy = active && wy.K == k;
      if (cx)
      {
        const bool sp = decltype(special)::value && wx.Ksp == k;
        dda_axis_advance(wx);
        if (decltype(special)::value && sp) dda_axis_after_zero_cell(wx, adx, sposx, dist, res);
      }
      if (cy)
      {
        const bool sp = decltype(special)::value && wy.Ksp == k;
        dda_axis_advance(wy);
        if (decltype(special)::value && sp) dda_axis_after_zero_cell(wy, ady, sposy, dist, res);
      }
      if (active) k = min(wx.K, wy.K);
    };
    auto walk = [&](auto special) {
      while (__any(k < (uint32_t)k1)) step(special, pend);
    };
    // (a ray that crosses the cell around zero -- the one cell that is 2 res - 1 wide -- needs a look at every crossing: a
    // loop of its own for the waves that hold such a ray)
    if (__any(work && (wx.Ksp != DDA_NEVER || wy.Ksp != DDA_NEVER)))
      walk(std::true_type{});
    else
      walk(std::false_type{});
    free_finish<true, SMALL>(a, pend, n_keyed, fblock); // the last candidate
  }
  // statistics: free-space candidates that became records
  for (int d = 32; d > 0; d >>= 1) n_keyed += __shfl_down(n_keyed, d, 64);
  if (lane == 0) s_keyed[threadIdx.x >> 6] = n_keyed;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    uint32_t all = 0;
    for (int w = 0; w < WS_FREE_THREADS / 64; ++w) all += s_keyed[w];
    if (all) atomicAdd(&a.counters->last_free_keyed, all);
#ifdef WS_FREE_TIMING
    // (instead of the tail march's statistics: 10 ns ticks this workgroup took, and when it started -- tools/free_timing.py)
    a.tail_stats[blockIdx.x] = (uint32_t)(wall_clock64() - t_free_begin);
    a.tail_stats[WS_TAIL_STATS + blockIdx.x] = (uint32_t)t_free_begin;
#endif
  }
}

void launch_march_free(const ScatterArgs &sa, bool small, hipStream_t s)
{
  const size_t n = sa.n;
  const dim3 grid_free((unsigned)((n + WS_FREE_THREADS / FREE_LANES - 1) / (WS_FREE_THREADS / FREE_LANES)));
  if (small)
    hipLaunchKernelGGL(march_free_kernel<true>, grid_free, dim3(WS_FREE_THREADS), 0, s, sa);
  else
    hipLaunchKernelGGL(march_free_kernel<false>, grid_free, dim3(WS_FREE_THREADS), 0, s, sa);
}
} // namespace ws
