// ws_sample.h — the rules of the point sample (stated in include/warpsense_hip.h at ws_map_sample), shared by the sample of a window
// (map_sample.hip) and the sample of the chunk store (store_sample.hip).  A point is ONE cell of the ray cast's field: the base voxel,
// the 8 corner entries, the validity and T are those of ws_raycast.h, taken through the same FIELD objects (ws_field_window.h,
// ws_field_store.h); what is new is what is made of them -- the 16-byte record, the class, the gradient at the nearest voxel -- and
// the ordered selection of input points by class:
//
//   sample_body      one lane per point: 8 gathers (6 more with WS_SAMPLE_GRADIENT), the record, the class
//   sample_tally     the class counts of a workgroup: ballots per wave, LDS per workgroup, one integer atomic per class and workgroup;
//                    with a selection also the workgroup's number of selected points (for the scan)
//   sample_emit      the selected points of a workgroup, in input order, behind those of the workgroups before it
//
// A workgroup is SAMPLE_WG = 256 consecutive points in all three.
#pragma once

#include "ws_raycast.h"

namespace ws
{
constexpr uint32_t SAMPLE_WG = 256, SAMPLE_WAVES = SAMPLE_WG / 64;

// what a sample call is asked, whatever the field
struct SampleCommon
{
  const int32_t *pts; // n x 3 map-frame points, mm
  uint32_t n;
  int32_t res, half, band;
  int64_t res3;
  FastDiv rdiv; // division by res
  uint32_t flags;
  uint32_t select; // bit c: class c is selected
  ri32x4 *rec;
  int32_t *grad;
  int32_t *sel;
  unsigned long long sel_cap; // points `sel` holds
  unsigned long long *counts; // [4] per class, [4] the scan's total
  uint32_t *blk_tot;                 // [workgroups] selected points
  const unsigned long long *blk_off; // [workgroups] exclusive scan of blk_tot
};
inline uint32_t sample_blocks(size_t n) { return (uint32_t)((n + SAMPLE_WG - 1) / SAMPLE_WG); }
inline uint32_t sample_select_mask(uint32_t flags) { return (flags / WS_SAMPLE_SELECT_UNKNOWN) & 15u; }
// ... into the buffers of a result holder
inline SampleCommon sample_common(const SampleResult &q, const int32_t *pts_dev, size_t n, int32_t res, int32_t band, uint32_t flags)
{
  SampleCommon a;
  a.pts = pts_dev;
  a.n = (uint32_t)n;
  a.res = res;
  a.half = res / 2;
  a.band = band;
  a.res3 = (int64_t)res * res * res;
  a.rdiv = make_fastdiv(res);
  a.flags = flags;
  a.select = sample_select_mask(flags);
  a.rec = static_cast<ri32x4 *>(q.rec.p);
  a.grad = static_cast<int32_t *>(q.grad.p);
  a.sel = static_cast<int32_t *>(q.sel.p);
  a.sel_cap = q.sel.cap;
  a.counts = q.counts.dev;
  a.blk_tot = static_cast<uint32_t *>(q.blk_tot.p);
  a.blk_off = static_cast<const unsigned long long *>(q.blk_off.p);
  return a;
}

// floor(T / res^3) for |T| < 2^46, res^3 <= 2^30
__device__ __forceinline__ int32_t sample_floor_T(int64_t T, int64_t res3)
{
  int64_t q = div_trunc_i64(T, res3);
  if (q * res3 > T) --q;
  return (int32_t)q;
}

__device__ __forceinline__ uint32_t sample_class(int32_t d, int32_t band) { return d >= band ? 1u : (d <= -band ? 3u : 2u); }

// Point i of the call (i < n): its record, and the gradient if asked for.  `live`: the field holds anything at all (a store call
// without a listed chunk has no table to look into).  Returns the class.
template <class Field> __device__ __forceinline__ uint32_t sample_body(const SampleCommon &a, Field &fld, bool live, uint32_t i)
{
  const bool any_weight = (a.flags & WS_SAMPLE_ANY_WEIGHT) != 0;
  int32_t p[3];
  bool dead = false;
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    p[k] = a.pts[3 * (size_t)i + k];
    dead = dead || p[k] <= -(1 << 30) || p[k] >= (1 << 30);
  }
  ri32x4 out = {0, 0, 0, 0};
  int32_t grad[3] = {0, 0, 0};
  if (!dead && live)
  {
    int32_t b[3], f[3], g[3], fg;
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      b[k] = floor_div(p[k] - a.half, a.rdiv, f[k]);
      g[k] = floor_div(p[k], a.rdiv, fg); // b or b + 1
    }
    uint32_t raw[8];
    if (fld.gather(b, raw))
    {
      RayCell cell;
      ray_cell_fill(raw, any_weight, cell);
      const int at = (g[0] - b[0]) * 4 + (g[1] - b[1]) * 2 + (g[2] - b[2]);
      uint32_t near = 0u;
      int32_t wmin = INT32_MAX;
#pragma unroll
      for (int j = 0; j < 8; ++j)
      {
        near = j == at ? raw[j] : near;
        const int32_t w = entry_weight(raw[j]);
        wmin = min(wmin, any_weight && w < 0 ? -w : w);
      }
      out.w = (int32_t)near;
      if (cell.valid)
      {
        out.x = sample_floor_T(ray_cell_T(cell, f, a.res), a.res3);
        out.y = wmin;
        out.z = (int32_t)sample_class(out.x, a.band);
      }
    }
    else if (fld.holds(g)) // the cell has a corner outside the field, or in an absent chunk: the nearest voxel may still be there
    {
      uint32_t near = 0u;
      if (fld.entry(g, near)) out.w = (int32_t)near;
    }
    if (a.flags & WS_SAMPLE_GRADIENT) ray_gradient_at(fld, g, any_weight, grad);
  }
  a.rec[i] = out;
  if (a.flags & WS_SAMPLE_GRADIENT)
  {
    a.grad[3 * (size_t)i + 0] = grad[0];
    a.grad[3 * (size_t)i + 1] = grad[1];
    a.grad[3 * (size_t)i + 2] = grad[2];
  }
  return (uint32_t)out.z;
}

// The class counts of the workgroup (every thread calls this; cls is 4 for a thread without a point): integer adds, so the counts
// are exact whatever the order
__device__ __forceinline__ void sample_tally(const SampleCommon &a, uint32_t cls)
{
  __shared__ uint32_t wcnt[SAMPLE_WAVES][4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t c = 0; c < 4; ++c)
  {
    const unsigned long long m = __ballot(cls == c);
    if (lane == 0) wcnt[wave][c] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  uint32_t tot = 0;
  if (threadIdx.x < 4)
  {
#pragma unroll
    for (uint32_t w = 0; w < SAMPLE_WAVES; ++w) tot += wcnt[w][threadIdx.x];
    if (tot) atomicAdd(a.counts + threadIdx.x, (unsigned long long)tot);
  }
  if (a.select)
  {
    // (lanes 0 .. 3 of wave 0 hold the four totals)
    uint32_t s = (threadIdx.x < 4 && ((a.select >> threadIdx.x) & 1u)) ? tot : 0u;
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (threadIdx.x == 0) a.blk_tot[blockIdx.x] = s;
  }
}

// The selected points of the workgroup in input order: point i goes to blk_off[workgroup] + selected points of the workgroup before
// it.  Nothing at or beyond sel_cap is written.
__device__ __forceinline__ void sample_emit(const SampleCommon &a)
{
  __shared__ uint32_t wsel[SAMPLE_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * SAMPLE_WG + threadIdx.x;
  const bool take = i < a.n && ((a.select >> ((uint32_t)a.rec[i < a.n ? i : 0].z & 3u)) & 1u);
  const unsigned long long m = __ballot(take);
  if (lane == 0) wsel[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (uint32_t w = 0; w < SAMPLE_WAVES; ++w) before += w < wave ? wsel[w] : 0u;
  const unsigned long long at =
      a.blk_off[blockIdx.x] + before + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (take && at < a.sel_cap)
  {
    a.sel[3 * at + 0] = a.pts[3 * (size_t)i + 0];
    a.sel[3 * at + 1] = a.pts[3 * (size_t)i + 1];
    a.sel[3 * at + 2] = a.pts[3 * (size_t)i + 2];
  }
}

// exclusive scan of the workgroups' selected counts (ws_device.h: the scan of the surface cloud)
__device__ __forceinline__ void sample_scan(const SampleCommon &a, uint32_t blocks) { scan_block_totals(a.blk_tot, const_cast<unsigned long long *>(a.blk_off), blocks, a.counts + 4); }

// The launch sequence, whatever the field: `Args` is the including file's, with the SampleCommon `s`.  The sample pass (events 1, 2),
// then with a selection the scan and the emit pass (events 2, 3); the counts arrive in q.counts.host (pinned) once the stream has
// been synchronised
template <typename Args> int sample_launch(SampleResult &q, hipStream_t st, const Args &a, void (*sample)(Args), void (*scan)(Args, uint32_t), void (*emit)(Args))
{
  const uint32_t blocks = sample_blocks(a.s.n);
  WS_HIP(hipMemsetAsync(a.s.counts, 0, 5 * sizeof(unsigned long long), st));
  q.timer.mark(1, st);
  hipLaunchKernelGGL(sample, dim3(blocks), dim3(SAMPLE_WG), 0, st, a);
  q.timer.mark(2, st);
  if (a.s.select)
  {
    hipLaunchKernelGGL(scan, dim3(1), dim3(1024), 0, st, a, blocks);
    hipLaunchKernelGGL(emit, dim3(blocks), dim3(SAMPLE_WG), 0, st, a);
  }
  q.timer.mark(3, st);
  WS_HIP(hipGetLastError());
  return q.counts.fetch(st, 4);
}

} // namespace ws
