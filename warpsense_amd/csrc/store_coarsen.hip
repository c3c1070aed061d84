// store_coarsen.hip — the one pass of ws_store_coarsen (include/warpsense_hip.h; the rule is in ws_coarsen.h, the plan in
// api_store_pair.hip): whole chunks of DST rebuilt from the up to eight chunks of SRC they cover, 2 x 2 x 2 voxels into one.
//
// A workgroup is 4 x 4 z columns of one dst chunk; a wave owns one column of 64 coarse voxels at a time, lane = z, so the store is one
// coalesced 256-byte access.  The children of a column lie in four columns of SRC (x and y pairs) of 128 consecutive z words: a lane
// loads the pair (2 z, 2 z + 1) as one 8-byte access, four 512-byte loads per wave and column.  The child chunk in x and y is the same
// for the whole workgroup (X >> 5, Y >> 5: a tile never straddles 32); in z the lanes 0 .. 31 read the child cz = 0 and the lanes
// 32 .. 63 the child cz = 1, a per-lane select between two bases.  A lane whose child chunk is absent loads nothing; a workgroup whose
// two z children are both absent writes fill without a load.  Every word of the dst chunk is written, so a chunk the call created needs
// no fill launch.
#include "ws_coarsen.h"

namespace ws
{
__device__ __forceinline__ uint32_t coarsen_wave_sum(uint32_t v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(COARSEN_WG) void store_coarsen_kernel(CoarsenArgs a)
{
  __shared__ uint32_t part[2][COARSEN_WG / 64];
  const uint32_t ci = blockIdx.x / COARSEN_TILES, tile = blockIdx.x % COARSEN_TILES;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  const uint32_t *row = a.rows + (size_t)ci * COARSEN_ROW;
  const uint32_t X = (tile >> 4) * 4u + wave, Y0 = (tile & 15u) * 4u;
  const uint32_t child = (X >> 5) * 4u + (Y0 >> 5) * 2u; // the child cz = 0 of this tile; cz = 1 follows it
  const uint32_t dslot = row[0], s0 = row[1 + child], s1 = row[2 + child];
  uint32_t *const dcol = a.dst_segs[dslot >> a.dst_shift] + (size_t)(dslot & ((1u << a.dst_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS + X * (uint32_t)(STORE_CS * STORE_CS) + lane;
  const uint32_t *const c0 = s0 == STORE_ABSENT ? nullptr : a.src_segs[s0 >> a.src_shift] + (size_t)(s0 & ((1u << a.src_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
  const uint32_t *const c1 = s1 == STORE_ABSENT ? nullptr : a.src_segs[s1 >> a.src_shift] + (size_t)(s1 & ((1u << a.src_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;

  uint32_t n_value = 0, n_short = 0; // per lane: at most 4 voxels
  if (!c0 && !c1) // (uniform)
  {
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) dcol[(Y0 + i) * (uint32_t)STORE_CS] = a.fill;
  }
  else
  {
    const uint32_t *const cp = lane < 32u ? c0 : c1;
    // the pair of this lane in the fine column (2 (X & 31), 2 (Y & 31)): words 2 (lane & 31) and the next
    const uint32_t at = 2u * (X & 31u) * (uint32_t)(STORE_CS * STORE_CS) + 2u * (Y0 & 31u) * (uint32_t)STORE_CS + 2u * (lane & 31u);
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i)
    {
      CoarsenAcc acc;
      if (cp)
      {
        const uint2 *p = reinterpret_cast<const uint2 *>(cp + at + 2u * i * (uint32_t)STORE_CS);
        const uint2 q00 = p[0], q01 = p[STORE_CS / 2], q10 = p[STORE_CS * STORE_CS / 2], q11 = p[STORE_CS * STORE_CS / 2 + STORE_CS / 2];
        coarsen_add(acc, q00.x), coarsen_add(acc, q00.y), coarsen_add(acc, q01.x), coarsen_add(acc, q01.y);
        coarsen_add(acc, q10.x), coarsen_add(acc, q10.y), coarsen_add(acc, q11.x), coarsen_add(acc, q11.y);
      }
      dcol[(Y0 + i) * (uint32_t)STORE_CS] = coarsen_entry(acc, a.min_observed, a.fill);
      n_value += acc.n >= a.min_observed ? 1u : 0u;
      n_short += acc.n >= 1 && acc.n < a.min_observed ? 1u : 0u;
    }
  }
  if (a.stats) // (uniform) integer adds: exact whatever the order
  {
    n_value = coarsen_wave_sum(n_value), n_short = coarsen_wave_sum(n_short);
    if (lane == 0u) part[0][wave] = n_value, part[1][wave] = n_short;
    __syncthreads();
    if (threadIdx.x < 2u)
    {
      const uint32_t sum = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
      if (sum) atomicAdd(a.stats + threadIdx.x, (unsigned long long)sum);
    }
  }
}

int launch_store_coarsen(hipStream_t s, const CoarsenArgs &a, size_t n_chunks)
{
  if (n_chunks == 0) return WS_OK;
  hipLaunchKernelGGL(store_coarsen_kernel, dim3((uint32_t)(n_chunks * COARSEN_TILES)), dim3(COARSEN_WG), 0, s, a);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
