// map_raycast.hip — ray cast of a device map (gfx950): the range image the sensor would see from a pose, with the hit points and,
// on request, the TSDF gradient at them.  The rules are stated in warpsense_hip.h at ws_map_raycast; this file walks them exactly,
// shortened only where the records provably stay the same:
//
//   raycast_kernel     one lane per ray: the march, the crossing, the record
//   raycast_grad_kernel  one lane per ray: six voxels around the hit
//
// What the march does not do per sample:
//   * divide.  p_k = o + trunc(d k step / L) per axis is carried as quotient and remainder of |d| step k by L: adding the
//     quotient and remainder of |d| step by L and one conditional carry gives the next sample exactly (|d| <= L, so the
//     quotient is at most k step <= max_range and the remainder stays below L < 2^31; all of it 32-bit).  trunc is odd, so the sign
//     of d goes on afterwards.  The base voxel floor((p - h) / res) is a multiply-shift (FastDiv, prepared on the host).
//   * gather a cell twice.  step = res / 2: the base voxel often stays; the 8 corner values and the cell's validity are kept
//     while it does.
//   * evaluate T where its sign is known.  The weights are >= 0 and sum to res^3 > 0: 8 positive corners give T > 0, 8
//     corners <= 0 give T <= 0.  Only a mixed cell is interpolated.  At a crossing both T are computed in full (T_{k-1} from a
//     fresh gather of its cell: once per ray).
//   * go on when nothing can follow.  Each axis of p_k is monotone in k, so the base voxel is too: once it has passed the last
//     cell of the window along an axis it moves away on (or stands still beside it), every later cell is invalid and no later
//     sample can be part of a hit.  The ray ends there, and at its hit.
//
// The corners are 4 pairs of z neighbours; a pair is one 8-byte load unless the ring's seam in z lies between the two.
// Plain launches on the context's stream; the output is indexed by ray: no compaction.  The one atomic is the hit counter
// (an integer sum, one add per wave).
#include "ws_device.h"

namespace ws
{
typedef int32_t ri32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t ru32x2_a4 __attribute__((ext_vector_type(2), aligned(4))); // two neighbouring entries, 4-byte aligned

struct RayArgs
{
  const uint32_t *data;
  MapParams mp;
  int32_t wlo[3], whi[3]; // the window in world voxels, inclusive
  int32_t origin[3];
  const int32_t *dirs; // n x 3: directions, or map-frame points under WS_RAYCAST_TARGETS
  uint32_t n;
  int32_t res, half, step;
  uint32_t K; // samples 0 .. K
  FastDiv rdiv; // division by res
  uint32_t flags;
  ri32x4 *rec;
  int32_t *grad;
  unsigned long long *hits;
};

__device__ __forceinline__ bool ray_valid(uint32_t raw, bool any_weight)
{
  const int32_t w = entry_weight(raw);
  return any_weight ? w != 0 : w > 0;
}

// floor(x / res) and the remainder, 0 <= f < res, for any int32 x
__device__ __forceinline__ int32_t floor_div(int32_t x, const FastDiv &d, int32_t &f)
{
  int32_t q = div_trunc(x, d);
  f = x - q * d.d;
  if (f < 0)
  {
    f += d.d;
    q -= 1;
  }
  return q;
}

// floor(sqrt(s)) exactly for 0 <= s < 2^62: the double root is off by a few units at most, the two loops settle it
__device__ __forceinline__ uint32_t isqrt_u64(uint64_t s)
{
  uint64_t r = (uint64_t)sqrt((double)s);
  while (r * r > s) --r;
  while ((r + 1) * (r + 1) <= s) ++r;
  return (uint32_t)r;
}

struct RayCell
{
  int32_t v[8]; // index cx * 4 + cy * 2 + cz
  bool valid;
};

// the 8 corners of the cell with base voxel b; invalid (values untouched) if a corner is outside the window or unobserved
__device__ __forceinline__ void ray_cell_load(const RayArgs &a, const int32_t b[3], bool any_weight, RayCell &c)
{
  c.valid = false;
  if (b[0] < a.wlo[0] || b[0] >= a.whi[0] || b[1] < a.wlo[1] || b[1] >= a.whi[1] || b[2] < a.wlo[2] || b[2] >= a.whi[2]) return;
  const int32_t sx = a.mp.size[0], sy = a.mp.size[1], sz = a.mp.size[2];
  const int32_t x0 = ring(b[0] - a.mp.pos[0] + a.mp.offset[0] + sx, sx), y0 = ring(b[1] - a.mp.pos[1] + a.mp.offset[1] + sy, sy);
  const int32_t z0 = ring(b[2] - a.mp.pos[2] + a.mp.offset[2] + sz, sz);
  const int32_t x1 = x0 + 1 == sx ? 0 : x0 + 1, y1 = y0 + 1 == sy ? 0 : y0 + 1;
  const bool seam = z0 + 1 == sz;
  uint32_t raw[8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    const int32_t xi = (j & 2) ? x1 : x0, yi = (j & 1) ? y1 : y0;
    const int64_t col = (int64_t)(xi * sy + yi) * (int64_t)sz; // size[0] * size[1] < 2^31 (ws_map_create)
    if (!seam)
    {
      const ru32x2_a4 p = *reinterpret_cast<const ru32x2_a4 *>(a.data + col + z0);
      raw[2 * j] = p.x;
      raw[2 * j + 1] = p.y;
    }
    else
    {
      raw[2 * j] = a.data[col + z0];
      raw[2 * j + 1] = a.data[col];
    }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 8; ++j)
  {
    ok = ok && ray_valid(raw[j], any_weight);
    c.v[j] = entry_value(raw[j]);
  }
  c.valid = ok;
}

// the trilinear interpolant times res^3: |T| <= 2^15 res^3 < 2^46
__device__ __forceinline__ int64_t ray_cell_T(const RayCell &c, const int32_t f[3], int32_t res)
{
  const int32_t wx[2] = {res - f[0], f[0]}, wy[2] = {res - f[1], f[1]}, wz[2] = {res - f[2], f[2]};
  int64_t T = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) T += (int64_t)c.v[j] * (int64_t)(wx[j >> 2] * wy[(j >> 1) & 1] * wz[j & 1]); // w <= res^3 <= 2^30
  return T;
}

__global__ __launch_bounds__(64) void raycast_kernel(RayArgs a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  const bool any_weight = (a.flags & WS_RAYCAST_ANY_WEIGHT) != 0;
  ri32x4 out = {0, 0, 0, -1};
  if (i < a.n)
  {
    int64_t d[3];
    bool live = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      d[k] = (int64_t)a.dirs[3 * (size_t)i + k];
      if (a.flags & WS_RAYCAST_TARGETS) d[k] -= (int64_t)a.origin[k];
      if (d[k] <= -(1ll << 30) || d[k] >= (1ll << 30)) live = false;
    }
    const uint32_t L = live ? isqrt_u64((uint64_t)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) : 0u;
    if (L != 0u)
    {
      // per axis: |d| step = qd L + rd; the sample's offset from the origin is q (remainder r), sign of d
      uint32_t qd[3], rd[3], q[3] = {0u, 0u, 0u}, r[3] = {0u, 0u, 0u};
      int32_t sgn[3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
      {
        const uint64_t m = (uint64_t)(d[k] < 0 ? -d[k] : d[k]) * (uint64_t)a.step; // < 2^39
        const uint64_t qq = (uint64_t)div_trunc_i64((int64_t)m, (int64_t)L);
        qd[k] = (uint32_t)qq; // <= step
        rd[k] = (uint32_t)(m - qq * (uint64_t)L);
        sgn[k] = d[k] < 0 ? -1 : (d[k] > 0 ? 1 : 0);
      }
      RayCell cell;
      cell.valid = false;
      int32_t cb[3] = {INT32_MIN, INT32_MIN, INT32_MIN}; // base voxel of `cell` (no sample has this one: (p - h) / res > INT32_MIN)
      bool all_pos = false, all_nonpos = false;
      // state of the sample before: 0 not (valid and T > 0), 1 valid and T > 0
      bool prev_front = false;
      int32_t pp[3] = {0, 0, 0}; // p_{k-1}
      for (uint32_t k = 0; k <= a.K; ++k)
      {
        int32_t p[3], b[3], f[3];
#pragma unroll
        for (int x = 0; x < 3; ++x)
        {
          p[x] = a.origin[x] + sgn[x] * (int32_t)q[x];
          b[x] = floor_div(p[x] - a.half, a.rdiv, f[x]);
        }
        // beyond the window for good (b is monotone along sgn): nothing valid can follow
        bool gone = false;
#pragma unroll
        for (int x = 0; x < 3; ++x) gone = gone || (sgn[x] >= 0 && b[x] >= a.whi[x]) || (sgn[x] <= 0 && b[x] < a.wlo[x]);
        if (gone) break;
        if (b[0] != cb[0] || b[1] != cb[1] || b[2] != cb[2])
        {
          ray_cell_load(a, b, any_weight, cell);
          cb[0] = b[0], cb[1] = b[1], cb[2] = b[2];
          if (cell.valid)
          {
            all_pos = all_nonpos = true;
#pragma unroll
            for (int j = 0; j < 8; ++j)
            {
              all_pos = all_pos && cell.v[j] > 0;
              all_nonpos = all_nonpos && cell.v[j] <= 0;
            }
          }
        }
        bool front = false, back = false; // valid and T > 0 / valid and T <= 0
        int64_t T = 0;
        bool have_T = false;
        if (cell.valid)
        {
          if (all_pos)
            front = true;
          else if (all_nonpos)
            back = true;
          else
          {
            T = ray_cell_T(cell, f, a.res);
            have_T = true;
            front = T > 0;
            back = !front;
          }
        }
        if (prev_front && back)
        {
          if (!have_T) T = ray_cell_T(cell, f, a.res);
          RayCell c0;
          int32_t b0[3], f0[3];
#pragma unroll
          for (int x = 0; x < 3; ++x) b0[x] = floor_div(pp[x] - a.half, a.rdiv, f0[x]);
          ray_cell_load(a, b0, any_weight, c0); // (valid: it was when the sample before was classified)
          const int64_t T0 = ray_cell_T(c0, f0, a.res);
          // T0 > 0 >= T: step T0 < 2^56, the divisor in (0, 2^47)
          const uint64_t t = (uint64_t)(k - 1u) * (uint64_t)a.step + ((uint64_t)a.step * (uint64_t)T0) / (uint64_t)(T0 - T);
#pragma unroll
          for (int x = 0; x < 3; ++x)
          {
            const int64_t h = div_trunc_i64(d[x] * (int64_t)t, (int64_t)L); // |d t| < 2^61
            if (x == 0) out.x = a.origin[0] + (int32_t)h;
            if (x == 1) out.y = a.origin[1] + (int32_t)h;
            if (x == 2) out.z = a.origin[2] + (int32_t)h;
          }
          out.w = (int32_t)t;
          break;
        }
        prev_front = front;
#pragma unroll
        for (int x = 0; x < 3; ++x)
        {
          pp[x] = p[x];
          q[x] += qd[x];
          r[x] += rd[x]; // < 2 L < 2^32
          if (r[x] >= L)
          {
            r[x] -= L;
            q[x] += 1u;
          }
        }
      }
    }
    a.rec[i] = out;
  }
  const unsigned long long hit = __ballot(out.w >= 0);
  if (threadIdx.x == 0 && hit) atomicAdd(a.hits, (unsigned long long)__popcll(hit));
}

__global__ __launch_bounds__(64) void raycast_grad_kernel(RayArgs a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.n) return;
  const bool any_weight = (a.flags & WS_RAYCAST_ANY_WEIGHT) != 0;
  const ri32x4 rec = a.rec[i];
  int32_t g[3] = {0, 0, 0};
  if (rec.w >= 0)
  {
    const int32_t hp[3] = {rec.x, rec.y, rec.z};
    int32_t c[3], f;
    bool ok = true; // the six neighbours lie in the window: c - 1 and c + 1 do on every axis
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      c[k] = floor_div(hp[k], a.rdiv, f);
      ok = ok && c[k] > a.wlo[k] && c[k] < a.whi[k];
    }
    if (ok)
    {
      int32_t diff[3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
      {
        int32_t v[3] = {c[0], c[1], c[2]};
        v[k] = c[k] + 1;
        const uint32_t hi = a.data[get_index(a.mp, v[0], v[1], v[2])];
        v[k] = c[k] - 1;
        const uint32_t lo = a.data[get_index(a.mp, v[0], v[1], v[2])];
        ok = ok && ray_valid(hi, any_weight) && ray_valid(lo, any_weight);
        diff[k] = entry_value(hi) - entry_value(lo);
      }
      if (ok) g[0] = diff[0], g[1] = diff[1], g[2] = diff[2];
    }
  }
  a.grad[3 * (size_t)i + 0] = g[0];
  a.grad[3 * (size_t)i + 1] = g[1];
  a.grad[3 * (size_t)i + 2] = g[2];
}

// the march (events 1, 2), then the gradient if asked for (events 2, 3); the hit count arrives in m->ray.hits.host (pinned)
// once the stream has been synchronised
int launch_raycast(ws_map *m, int which, const int32_t origin[3], const int32_t *dirs_dev, size_t n, int32_t max_range, uint32_t flags)
{
  RayArgs a;
  a.data = m->data[which].as<uint32_t>();
  a.mp = m->par[which];
  for (int k = 0; k < 3; ++k)
  {
    a.wlo[k] = a.mp.pos[k] - a.mp.size[k] / 2;
    a.whi[k] = a.wlo[k] + a.mp.size[k] - 1;
    a.origin[k] = origin[k];
  }
  a.dirs = dirs_dev;
  a.n = (uint32_t)n;
  a.res = m->res;
  a.half = m->res / 2;
  a.step = std::max(m->res / 2, 1);
  a.K = (uint32_t)(max_range / a.step);
  a.rdiv = make_fastdiv(m->res);
  a.flags = flags;
  a.rec = static_cast<ri32x4 *>(m->ray.rec.p);
  a.grad = static_cast<int32_t *>(m->ray.grad.p);
  a.hits = m->ray.hits.dev;
  hipStream_t s = m->ctx->stream;
  const uint32_t blocks = (uint32_t)((n + 63) / 64);
  WS_HIP(hipMemsetAsync(a.hits, 0, sizeof(unsigned long long), s));
  m->ray.timer.mark(1, s);
  hipLaunchKernelGGL(raycast_kernel, dim3(blocks), dim3(64), 0, s, a);
  m->ray.timer.mark(2, s);
  if (flags & WS_RAYCAST_GRADIENT) hipLaunchKernelGGL(raycast_grad_kernel, dim3(blocks), dim3(64), 0, s, a);
  m->ray.timer.mark(3, s);
  WS_HIP(hipGetLastError());
  return m->ray.hits.fetch(s);
}

} // namespace ws
