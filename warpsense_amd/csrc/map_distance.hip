// map_distance.hip — the distance field of a device map (gfx950): per voxel of a box the squared Euclidean distance, in voxels, to
// the nearest occupied (or never observed) voxel of that box, clamped at R^2.  The rules are stated in warpsense_hip.h at
// ws_map_distance; this file gets to the same records by the separable form of the minimum:
//
//   dist_classify_kernel   pass 0: reads the ring once (a wave per (x, y) column, lanes along z), writes the class bits into the
//                          records and g0 = 0 at a site, R^2 elsewhere, into a 16-bit plane in dense box order;
//                          <COLUMNS>: the same read, reduced along z to one class and one g0 per column
//   dist_line_kernel       g'(i) = min(g(i), min over 1 <= |d| <= R of g(i + d) + d^2) along an axis that is NOT the fastest one
//                          (x, y): lanes along the fastest axis, so every load of a wave is one contiguous run and the position i
//                          on the line and the offset d are the same for the whole wave
//   dist_row_kernel        the same along the fastest axis (z; y for columns): 256 consecutive voxels of a line and R voxels on
//                          either side are staged in LDS, a lane per output; the result goes into the records next to the class
//
// Every g stays <= R^2 <= 65 025, so the planes carry 2 bytes per voxel; sums are formed in 32-bit registers.  A true d2 <= R^2
// has |d| <= R on every axis, so the window and the clamp after each pass lose nothing.
// The window is bounded by what is already known: a candidate at offset d can only win if d^2 < g'(i) so far, so a wave stops
// at the first d whose square has reached the largest running minimum of its lanes (one compare and a branch on its mask).
// Next to a site that is a handful of steps; only voxels that stay at the clamp walk all R.
// Plain launches on the context's stream, no floating point; the one atomic is the site counter (one add per wave).
#include "ws_device.h"

namespace ws
{
constexpr int DIST_ROW = 256;     // outputs per workgroup of dist_row_kernel
constexpr int DIST_MAX_R = 255;   // ws_map_distance: 1 <= R <= 255
constexpr uint32_t DIST_OUTSIDE = 0xffffu; // beyond the end of a line: never a minimum (0xffff + d^2 > R^2)

struct DistArgs
{
  BoxArgs box;
  uint32_t r2;
  uint32_t flags;
  uint32_t *rec;
  uint16_t *plane;
  unsigned long long *sites;
};

template <bool COLUMNS>
__global__ __launch_bounds__(256) void dist_classify_kernel(DistArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t col = blockIdx.x * 4u + (uint32_t)wave;
  if (col >= a.box.n_cols) return; // (the same for the whole wave)
  const bool any_weight = (a.flags & WS_DISTANCE_ANY_WEIGHT) != 0, unknown_occ = (a.flags & WS_DISTANCE_UNKNOWN_OCCUPIED) != 0;
  int32_t x, y, zs0;
  const int64_t cbase = box_column(a.box, col, x, y, zs0);
  const int32_t sz = a.box.mp.size[2];
  const uint64_t out0 = (uint64_t)col * (uint64_t)a.box.ez;
  uint32_t n_sites = 0;
  bool occ = false, unk = false, fre = false; // COLUMNS: what the column holds
  for (int32_t z0 = 0; z0 < a.box.ez; z0 += 64)
  {
    const int32_t z = z0 + lane;
    const bool in = z < a.box.ez;
    int32_t zi = zs0 + (in ? z : 0); // the ring's seam in z: the run goes on at storage z 0
    if (zi >= sz) zi -= sz;
    const uint32_t cls = dist_class(a.box.data[cbase + zi], any_weight);
    const bool site = in && (cls == 2u || (unknown_occ && cls == 0u));
    if (COLUMNS)
    {
      occ = occ || __ballot(in && cls == 2u) != 0ull;
      unk = unk || __ballot(in && cls == 0u) != 0ull;
      fre = fre || __ballot(in && cls == 1u) != 0ull;
    }
    else
    {
      if (in)
      {
        a.rec[out0 + (uint64_t)z] = cls << 30;
        a.plane[out0 + (uint64_t)z] = (uint16_t)(site ? 0u : a.r2);
      }
      n_sites += (uint32_t)__popcll(__ballot(site));
    }
  }
  if (COLUMNS)
  {
    const bool site = occ || (unknown_occ && unk);
    const uint32_t cls = occ ? 2u : (site ? 0u : (fre ? 1u : 0u));
    if (lane == 0)
    {
      a.rec[col] = cls << 30;
      a.plane[col] = (uint16_t)(site ? 0u : a.r2);
    }
    n_sites = site ? 1u : 0u;
  }
  if (lane == 0 && n_sites) atomicAdd(a.sites, (unsigned long long)n_sites);
}

struct DistLineArgs
{
  const uint16_t *in;
  uint16_t *out;
  uint32_t inner; // voxels of the fastest part: consecutive in memory, one per lane
  uint32_t line;  // voxels along the pass's axis, `inner` apart
  uint32_t i0, o0; // first line position / outer index of this launch (grids hold 65 535 in y and z)
  int32_t R;
};

// grid: (inner / 64, positions on the line, outer)
__global__ __launch_bounds__(64) void dist_line_kernel(DistLineArgs a)
{
  const uint32_t j = blockIdx.x * 64u + threadIdx.x, i = a.i0 + blockIdx.y, o = a.o0 + blockIdx.z;
  const bool active = j < a.inner;
  const uint16_t *base = a.in + ((uint64_t)o * a.line) * (uint64_t)a.inner + (active ? j : a.inner - 1u); // an idle lane reads the last one
  const uint64_t at = (uint64_t)i * a.inner;
  uint32_t best = active ? (uint32_t)base[at] : 0u;
  const uint32_t below = min((uint32_t)a.R, i), above = min((uint32_t)a.R, a.line - 1u - i); // (uniform)
  const uint32_t both = min(below, above), far = max(below, above);
  uint32_t d = 1;
  for (; d <= both; ++d)
  {
    const uint32_t d2 = d * d;
    if (__ballot(d2 < best) == 0ull) break; // no lane can still gain: d^2 alone has reached every running minimum
    const uint64_t s = (uint64_t)d * a.inner;
    const uint32_t v = min((uint32_t)base[at - s], (uint32_t)base[at + s]);
    best = min(best, v + d2);
  }
  if (d > both) // one side has run into the end of the line
  {
    for (; d <= far; ++d)
    {
      const uint32_t d2 = d * d;
      if (__ballot(d2 < best) == 0ull) break;
      const uint64_t s = (uint64_t)d * a.inner;
      best = min(best, (uint32_t)(below > above ? base[at - s] : base[at + s]) + d2);
    }
  }
  if (active) a.out[((uint64_t)o * a.line + i) * (uint64_t)a.inner + j] = (uint16_t)best;
}

struct DistRowArgs
{
  const uint16_t *in;
  uint32_t *rec;
  uint32_t len; // voxels of a line, consecutive in memory
  int32_t R;
};

// grid: (lines, segments of DIST_ROW outputs)
__global__ __launch_bounds__(DIST_ROW) void dist_row_kernel(DistRowArgs a)
{
  __shared__ uint16_t tile[DIST_ROW + 2 * DIST_MAX_R + 2];
  const int32_t z0 = (int32_t)blockIdx.y * DIST_ROW, R = a.R, t = (int32_t)threadIdx.x;
  const uint64_t row = (uint64_t)blockIdx.x * (uint64_t)a.len;
  for (int32_t k = t; k < DIST_ROW + 2 * R; k += DIST_ROW)
  {
    const int32_t z = z0 - R + k;
    tile[k] = (z >= 0 && z < (int32_t)a.len) ? a.in[row + (uint64_t)z] : (uint16_t)DIST_OUTSIDE;
  }
  __syncthreads();
  const int32_t z = z0 + t;
  const bool active = z < (int32_t)a.len;
  const uint16_t *c = tile + R + t;
  uint32_t best = active ? (uint32_t)c[0] : 0u;
  for (int32_t d = 1; d <= R; ++d)
  {
    const uint32_t d2 = (uint32_t)(d * d);
    if (__ballot(d2 < best) == 0ull) break;
    best = min(best, min((uint32_t)c[-d], (uint32_t)c[d]) + d2);
  }
  if (active) a.rec[row + (uint64_t)z] = (a.rec[row + (uint64_t)z] & 0xc0000000u) | best;
}

static void dist_line(hipStream_t s, const uint16_t *in, uint16_t *out, uint32_t outer, uint32_t line, uint32_t inner, int32_t R)
{
  DistLineArgs a;
  a.in = in;
  a.out = out;
  a.inner = inner;
  a.line = line;
  a.R = R;
  for (uint32_t o0 = 0; o0 < outer; o0 += 65535u)
    for (uint32_t i0 = 0; i0 < line; i0 += 65535u)
    {
      a.o0 = o0;
      a.i0 = i0;
      hipLaunchKernelGGL(dist_line_kernel, dim3((uint32_t)(((uint64_t)inner + 63u) / 64u), std::min(line - i0, 65535u), std::min(outer - o0, 65535u)), dim3(64), 0, s, a);
    }
}

// Pass 0 over the ring (events 0, 1): the site counter is cleared in front of it.
int launch_dist_classify(ws_map *m, DistResult &q, int which, const int32_t lo[3], const int32_t ext[3], int32_t R, uint32_t flags)
{
  DistArgs a;
  a.box = box_args(m, which, lo, ext);
  a.r2 = (uint32_t)(R * R);
  a.flags = flags;
  a.rec = q.rec.as<uint32_t>();
  a.plane = q.plane.as<uint16_t>();
  a.sites = q.sites.dev;
  hipStream_t s = m->ctx->stream;
  WS_HIP(hipMemsetAsync(a.sites, 0, sizeof(unsigned long long), s));
  q.timer.mark(0, s);
  if (flags & WS_DISTANCE_COLUMNS)
    hipLaunchKernelGGL((dist_classify_kernel<true>), dim3((a.box.n_cols + 3u) / 4u), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((dist_classify_kernel<false>), dim3((a.box.n_cols + 3u) / 4u), dim3(256), 0, s, a);
  q.timer.mark(1, s);
  return WS_OK;
}

// the row pass over `lines` lines; a launch holds at most 2^23 of them (its threads are counted in 32 bits), the next one goes on
// behind them
static void dist_rows(hipStream_t s, const uint16_t *in, uint32_t *rec, uint32_t lines, uint32_t len, int32_t R)
{
  DistRowArgs r;
  r.len = len;
  r.R = R;
  for (uint32_t l0 = 0; l0 < lines; l0 += 1u << 23)
  {
    r.in = in + (uint64_t)l0 * len;
    r.rec = rec + (uint64_t)l0 * len;
    hipLaunchKernelGGL(dist_row_kernel, dim3(std::min(lines - l0, 1u << 23), (len + DIST_ROW - 1) / DIST_ROW), dim3(DIST_ROW), 0, s, r);
  }
}

// The x, y and z passes (events 1 .. 4) behind a pass 0 that has written the class bits into `rec` and g0 into the first of the two
// planes of `plane`; under WS_DISTANCE_COLUMNS the x and the y pass (events 3, 4 coincide).  Both sources of a distance field come
// here: the window of a map (launch_dist_classify) and the chunks of the store (store_distance.hip).
int dist_passes(hipStream_t s, QueryTimer &t, uint32_t *rec, uint16_t *plane, const uint32_t ext[3], int32_t R, uint32_t flags)
{
  static_assert(DIST_MAX_LINE == 65535u * (uint32_t)DIST_ROW, "a line of the row pass: 65 535 workgroups of DIST_ROW outputs");
  const uint32_t nx = ext[0], ny = ext[1];
  if (flags & WS_DISTANCE_COLUMNS)
  {
    uint16_t *p0 = plane, *p1 = p0 + (uint64_t)nx * ny;
    dist_line(s, p0, p1, 1u, nx, ny, R);
    t.mark(2, s);
    dist_rows(s, p1, rec, nx, ny, R);
    t.mark(3, s);
  }
  else
  {
    const uint32_t nz = ext[2];
    uint16_t *p0 = plane, *p1 = p0 + (uint64_t)nx * ny * nz;
    dist_line(s, p0, p1, 1u, nx, ny * nz, R); // ny nz < 2^32: the records are counted in 32 bits
    t.mark(2, s);
    dist_line(s, p1, p0, nx, ny, nz, R);
    t.mark(3, s);
    dist_rows(s, p0, rec, nx * ny, nz, R);
  }
  t.mark(4, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
