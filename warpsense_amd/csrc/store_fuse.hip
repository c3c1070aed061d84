// store_fuse.hip — the two passes of ws_store_fuse (include/warpsense_hip.h; the rules are in ws_fuse.h, the plan in api_store_pair.hip):
// one chunk store resampled on the lattice of another under a rigid pull transform and integrated into it.
//
//   store_fuse_kernel<false>   count pass: per candidate dst chunk the voxels that receive a valid sample, and the sums of the
//                              statistics; it writes nothing else
//   store_fuse_kernel<true>    write pass over the candidates with a non-zero count: the same sample again, integrated in place
//
// A workgroup is 4 x 4 z columns of one dst chunk; a wave owns one column of 64 voxels at a time, lane = z, so the read-modify-write
// of DST is one coalesced 256-byte access.  The x and y terms of the transform are formed once per column from wave-uniform values;
// a lane adds its z term.  SRC is gathered through StoreField::lookup with its one-chunk cache, up to eight loads per lane.  A
// column none of whose lanes falls into a present chunk of SRC is left after one lookup per lane.  Re-sampling instead of staging the
// samples of the count pass follows map_surface.hip's count / emit shape: no buffer follows the number of voxels.
#include "ws_fuse.h"

namespace ws
{
__device__ __forceinline__ uint32_t fuse_wave_sum(uint32_t v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool WRITE> __global__ __launch_bounds__(FUSE_WG) void store_fuse_kernel(FuseArgs a)
{
  const uint32_t ci = blockIdx.x / FUSE_TILES, tile = blockIdx.x % FUSE_TILES;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  const FuseCand c = a.cand[ci];
  uint32_t *const dchunk = c.slot == STORE_ABSENT ? nullptr : a.dst_segs[c.slot >> a.dst_shift] + (size_t)(c.slot & ((1u << a.dst_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
  StoreRayArgs sa; // (only what lookup() reads)
  sa.table = a.src_table, sa.mask = a.src_mask, sa.segs = a.src_segs, sa.seg_shift = a.src_shift;
  StoreField fld(sa);

  // p - pivot_dst per axis, 64-bit until it is known to lie within the reach
  const uint32_t lx = (tile >> 4) * 4u + wave;
  const int64_t dx64 = ((int64_t)c.cx * STORE_CS + (int64_t)lx) * a.res + a.half - (int64_t)a.pd[0];
  const int64_t dz64 = ((int64_t)c.cz * STORE_CS + (int64_t)lane) * a.res + a.half - (int64_t)a.pd[2];
  const bool in_x = dx64 > -FUSE_REACH && dx64 < FUSE_REACH, in_z = dz64 > -FUSE_REACH && dz64 < FUSE_REACH;
  const int32_t dx = (int32_t)dx64, dz = (int32_t)dz64;

  uint32_t n_avg = 0, n_set = 0, s_diff = 0, s_minw = 0; // per lane: at most 4 voxels
  for (uint32_t i = 0; i < 4u; ++i)
  {
    const uint32_t ly = (tile & 15u) * 4u + i;
    const int64_t dy64 = ((int64_t)c.cy * STORE_CS + (int64_t)ly) * a.res + a.half - (int64_t)a.pd[1];
    if (!in_x || dy64 <= -FUSE_REACH || dy64 >= FUSE_REACH) continue; // (uniform)
    const int32_t dy = (int32_t)dy64;
    int32_t b[3], f[3];
    bool live = in_z;
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      const int64_t base = (int64_t)a.rot[3 * k] * dx + (int64_t)a.rot[3 * k + 1] * dy + (1ll << 29);
      const int64_t q = fuse_pull(base, a.rot[3 * k + 2], dz, a.ps[k]);
      live = live && !fuse_dead(q);
      b[k] = floor_div(live ? (int32_t)q - a.half : 0, a.rdiv, f[k]);
    }
    // the corner (0, 0, 0) always takes part: without its chunk there is no valid sample
    live = live && fuse_src_chunk(fld, b[0] >> 6, b[1] >> 6, b[2] >> 6) != nullptr;
    if (__ballot(live) == 0ull) continue;
    int32_t nv = 0, nw = 0;
    const bool valid = live && fuse_sample(a, fld, b, f, nv, nw);
    const uint32_t at = lx * (uint32_t)(STORE_CS * STORE_CS) + ly * (uint32_t)STORE_CS + lane;
    if (WRITE)
    {
      if (valid) dchunk[at] = fuse_integrate(dchunk[at], nv, nw, a.max_weight);
    }
    else if (valid)
    {
      const uint32_t e = dchunk ? dchunk[at] : a.fill;
      const int32_t ev = entry_value(e), ew = entry_weight(e);
      if (ew > 0)
      {
        n_avg += 1u;
        s_diff += (uint32_t)(nv > ev ? nv - ev : ev - nv);
        s_minw += (uint32_t)min(nw, ew);
      }
      else
        n_set += 1u;
    }
  }
  if (!WRITE)
  {
    // integer adds: exact whatever the order
    n_avg = fuse_wave_sum(n_avg), n_set = fuse_wave_sum(n_set), s_diff = fuse_wave_sum(s_diff), s_minw = fuse_wave_sum(s_minw);
    if (lane == 0u && (n_avg | n_set))
    {
      atomicAdd(a.counts + ci, n_avg + n_set);
      if (n_avg) atomicAdd(a.stats + 0, (unsigned long long)n_avg);
      if (n_set) atomicAdd(a.stats + 1, (unsigned long long)n_set);
      if (s_diff) atomicAdd(a.stats + 2, (unsigned long long)s_diff);
      if (s_minw) atomicAdd(a.stats + 3, (unsigned long long)s_minw);
    }
  }
}

int launch_store_fuse(hipStream_t s, const FuseArgs &a, size_t n_candidates, bool write)
{
  if (n_candidates == 0) return WS_OK;
  const dim3 grid((uint32_t)(n_candidates * FUSE_TILES)), block(FUSE_WG);
  if (write)
    hipLaunchKernelGGL(store_fuse_kernel<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(store_fuse_kernel<false>, grid, block, 0, s, a);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
