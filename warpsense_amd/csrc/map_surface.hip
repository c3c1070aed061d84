// map_surface.hip — the surface cloud of a device map (gfx950): what publish_local_map
// (include/warpsense/visualization/map.h:14-121) collects on the host from a downloaded map, as an ORDERED stream compaction on the
// device.  A voxel qualifies if weight > 0 && abs(value) < band (map.h:45, band = tau there); the output is in ascending world
// (x, y, z), z fastest -- the order in which the reference's collapse(3) schedule(static) loop concatenates its per-thread results
// -- so it is the same bytes on every run.
//
//   surface_kernel<COUNT>    qualifying voxels per (x, y) column of the box, and per workgroup (SURF_COLS consecutive columns)
//   surface_scan_kernel      exclusive scan of the workgroup totals (one workgroup; the last element is the total)
//   surface_kernel<EMIT..>   the predicate again; a record goes to (workgroup base + columns before + rank inside the column)
//
// Plain launches on the context's stream, nothing waits for another workgroup, no atomics.
// Memory is z fastest and rotated by `offset` on every axis (get_index, ws_device.h), so the world-order z run of one column is at
// most two contiguous storage runs: [zs0, size_z) then [0, ...).  Each run is read as ALIGNED 16-byte loads (four voxels per lane,
// 1 KiB per wave instruction) whose first and last group are masked: size_z is odd for the reference's maps, so no column starts on
// a 16-byte boundary.  The maps carry 16 bytes of slack behind the last voxel (ws_map_create), which the last group may touch.
// Which voxel qualifies, its record and its marker are the rules of ws_surface.h, which the cloud of the chunk store shares.
#include "ws_surface.h"

namespace ws
{
constexpr int SURF_COLS = 16; // columns per workgroup: four per wave, one after the other
constexpr int SURF_WAVES = 4;
constexpr int SURF_COUNT = 0, SURF_EMIT = 1, SURF_EMIT_MARKER = 2;

struct SurfArgs
{
  BoxArgs box;
  int32_t band, tau, res;
  uint32_t *col_cnt;                  // [n_cols]
  uint32_t *blk_tot;                  // [workgroups]
  const unsigned long long *blk_off;  // [workgroups] exclusive scan of blk_tot
  su32x4 *rec;                        // x, y, z, raw
  float *marker;                      // 7 floats per record: x y z (metres) r g b a
  unsigned long long cap;             // records the output buffers hold
};

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask)
{
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

template <int MODE>
__global__ __launch_bounds__(256) void surface_kernel(SurfArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t col0 = blockIdx.x * (uint32_t)SURF_COLS;
  uint32_t before = 0; // EMIT: records of the workgroup's columns before column `lane`
  unsigned long long base = 0;
  if (MODE != SURF_COUNT)
  {
    const uint32_t c = (lane < SURF_COLS && col0 + lane < a.box.n_cols) ? a.col_cnt[col0 + lane] : 0u;
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < SURF_COLS; d <<= 1)
    {
      const uint32_t t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    before = inc - c;
    base = a.blk_off[blockIdx.x];
  }
  const float fres = (float)a.res, ftau = (float)a.tau;
  uint32_t wave_total = 0;
  for (int k = 0; k < SURF_COLS / SURF_WAVES; ++k)
  {
    const int ci = wave * (SURF_COLS / SURF_WAVES) + k;
    const uint32_t col = col0 + (uint32_t)ci;
    if (col >= a.box.n_cols) break; // (the same for the whole wave)
    int32_t x, y, zs0;
    const int64_t cbase = box_column(a.box, col, x, y, zs0);
    const int32_t len_a = min(a.box.ez, a.box.mp.size[2] - zs0); // voxels up to the ring seam; the rest starts at storage z 0
    unsigned long long out = base + __shfl(before, ci, 64);
    const float px = surf_metres(x, fres), py = surf_metres(y, fres);
    uint32_t cnt = 0;
#pragma unroll
    for (int run = 0; run < 2; ++run)
    {
      const int32_t len = run ? a.box.ez - len_a : len_a;
      if (len <= 0) continue;
      const int32_t zw0 = a.box.lo[2] + (run ? len_a : 0); // world z of the run's first voxel
      const int64_t first = cbase + (run ? 0 : zs0), last = first + len;
      for (int64_t g0 = first & ~(int64_t)3; g0 < last; g0 += 256)
      {
        const int64_t g = g0 + 4 * lane;
        su32x4 v = {0u, 0u, 0u, 0u};
        if (g < last) v = __builtin_nontemporal_load(reinterpret_cast<const su32x4 *>(a.box.data + g));
        const uint32_t raw[4] = {v.x, v.y, v.z, v.w};
        bool q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = g + j >= first && g + j < last && surf_pred(raw[j], a.band);
        if (MODE == SURF_COUNT)
        {
          cnt += (uint32_t)q[0] + (uint32_t)q[1] + (uint32_t)q[2] + (uint32_t)q[3];
        }
        else
        {
          // world order = lane major, then the lane's four voxels: records of lower lanes first
          const unsigned long long b0 = __ballot(q[0]), b1 = __ballot(q[1]), b2 = __ballot(q[2]), b3 = __ballot(q[3]);
          unsigned long long o = out + (lanes_below(b0) + lanes_below(b1) + lanes_below(b2) + lanes_below(b3));
          const int32_t z0 = zw0 + (int32_t)(g - first);
#pragma unroll
          for (int j = 0; j < 4; ++j)
          {
            if (!q[j]) continue;
            if (o < a.cap) // (the count pass sized the buffers; a map that changed in between must not write beyond them)
            {
              surf_put_record(a.rec, o, x, y, z0 + j, raw[j]);
              if (MODE == SURF_EMIT_MARKER) surf_put_marker(a.marker, o, px, py, z0 + j, raw[j], fres, ftau);
            }
            ++o;
          }
          out += (unsigned long long)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
        }
      }
    }
    if (MODE == SURF_COUNT)
    {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
      if (lane == 0) a.col_cnt[col] = cnt;
      wave_total += cnt;
    }
  }
  if (MODE == SURF_COUNT)
  {
    __shared__ uint32_t wtot[SURF_WAVES];
    if (lane == 0) wtot[wave] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) a.blk_tot[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  }
}

// exclusive scan of the workgroup totals
__global__ __launch_bounds__(1024) void surface_scan_kernel(const uint32_t *tot, unsigned long long *off, uint32_t n, unsigned long long *total)
{
  scan_block_totals(tot, off, n, total);
}

static uint32_t surf_blocks(uint32_t n_cols) { return (n_cols + SURF_COLS - 1) / SURF_COLS; }

static SurfArgs surf_args(const ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t band, size_t cap)
{
  SurfArgs a;
  a.box = box_args(m, which, lo, ext);
  a.band = band;
  a.tau = m->tau;
  a.res = m->res;
  a.col_cnt = static_cast<uint32_t *>(m->surf.col_cnt.p);
  a.blk_tot = static_cast<uint32_t *>(m->surf.blk_tot.p);
  a.blk_off = static_cast<unsigned long long *>(m->surf.blk_off.p);
  a.rec = static_cast<su32x4 *>(m->surf.rec.p);
  a.marker = static_cast<float *>(m->surf.marker.p);
  a.cap = cap;
  return a;
}

size_t surface_blocks_for(int64_t n_cols) { return (size_t)surf_blocks((uint32_t)n_cols); }

// passes 1 and 2; the total arrives in m->surf.total.host (pinned) once the stream has been synchronised
int launch_surface_count(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t band)
{
  const SurfArgs a = surf_args(m, which, lo, ext, band, 0);
  const uint32_t blocks = surf_blocks(a.box.n_cols);
  hipStream_t s = m->ctx->stream;
  QueryTimer &t = m->surf.timer;
  t.mark(0, s);
  hipLaunchKernelGGL((surface_kernel<SURF_COUNT>), dim3(blocks), dim3(256), 0, s, a);
  t.mark(1, s);
  hipLaunchKernelGGL(surface_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)a.blk_tot, static_cast<unsigned long long *>(m->surf.blk_off.p), blocks, m->surf.total.dev);
  t.mark(2, s);
  WS_HIP(hipGetLastError());
  return m->surf.total.fetch(s);
}

// pass 3: no record at or beyond `cap` is written
int launch_surface_emit(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t band, bool marker, size_t cap)
{
  const SurfArgs a = surf_args(m, which, lo, ext, band, cap);
  const uint32_t blocks = surf_blocks(a.box.n_cols);
  hipStream_t s = m->ctx->stream;
  m->surf.timer.mark(3, s);
  if (marker)
    hipLaunchKernelGGL((surface_kernel<SURF_EMIT_MARKER>), dim3(blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((surface_kernel<SURF_EMIT>), dim3(blocks), dim3(256), 0, s, a);
  m->surf.timer.mark(4, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
