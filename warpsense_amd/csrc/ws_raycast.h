// ws_raycast.h — the record rules of the ray cast (stated in include/warpsense_hip.h at ws_map_raycast), shared by the ray cast of a
// window (map_raycast.hip) and the ray cast of the chunk store (store_raycast.hip).  Both walk the samples p_k of a ray, gather the 8
// corner entries of the cell of a sample, classify it and place the crossing; what differs is WHERE the entries lie (a ring buffer,
// 64^3 chunks behind a lookup) and which samples may be passed over because nothing valid can be there.  Everything that decides a
// byte of a record or of the gradient is here, once, as functions of corner entries and integers: ray_march and ray_gradient take a
// FIELD, an object of the including file with
//
//   bool gone(b, sgn)                 the base voxel b has passed, for good, everything that can be valid (b is monotone along sgn)
//   void load(b, any_weight, cell)    the 8 corners of the cell with base voxel b through ray_cell_fill, or cell.valid = false
//   static constexpr bool JUMPS       the field can name samples whose cells are invalid without loading them:
//   uint32_t resume(ray, a, b, k)       after load(b) left an invalid cell at sample k: the first k' > k whose cell may be valid
//   bool grad_inside(c)               the six neighbours c +- e_k of voxel c can be valid at all
//   bool entry(v, raw)                the raw entry of voxel v; false: there is no such voxel (not valid)
#pragma once

#include "ws_device.h"

namespace ws
{
typedef int32_t ri32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t ru32x2_a4 __attribute__((ext_vector_type(2), aligned(4))); // two neighbouring entries, 4-byte aligned

// what a ray cast is asked, whatever the field
struct RayCommon
{
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
// ... into the buffers of a result holder
inline RayCommon ray_common(const RayResult &q, const int32_t origin[3], const int32_t *dirs_dev, size_t n, int32_t res, int32_t max_range, uint32_t flags)
{
  RayCommon a;
  for (int k = 0; k < 3; ++k) a.origin[k] = origin[k];
  a.dirs = dirs_dev;
  a.n = (uint32_t)n;
  a.res = res;
  a.half = res / 2;
  a.step = res / 2 > 1 ? res / 2 : 1;
  a.K = (uint32_t)(max_range / a.step);
  a.rdiv = make_fastdiv(res);
  a.flags = flags;
  a.rec = static_cast<ri32x4 *>(q.rec.p);
  a.grad = static_cast<int32_t *>(q.grad.p);
  a.hits = q.hits.dev;
  return a;
}
// The launch sequence, whatever the field: `Args` is the including file's, with the RayCommon `c`.  The march (events 1, 2), then the
// gradient if asked for (events 2, 3); the hit count arrives in q.hits.host (pinned) once the stream has been synchronised
template <typename Args> int ray_launch(RayResult &q, hipStream_t s, const Args &a, void (*march)(Args), void (*gradient)(Args))
{
  const uint32_t blocks = (a.c.n + 63u) / 64u;
  WS_HIP(hipMemsetAsync(a.c.hits, 0, sizeof(unsigned long long), s));
  q.timer.mark(1, s);
  hipLaunchKernelGGL(march, dim3(blocks), dim3(64), 0, s, a);
  q.timer.mark(2, s);
  if (a.c.flags & WS_RAYCAST_GRADIENT) hipLaunchKernelGGL(gradient, dim3(blocks), dim3(64), 0, s, a);
  q.timer.mark(3, s);
  WS_HIP(hipGetLastError());
  return q.hits.fetch(s);
}

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

// a cell from its 8 corner entries: valid iff all 8 are observed under the weight rule
__device__ __forceinline__ void ray_cell_fill(const uint32_t raw[8], bool any_weight, RayCell &c)
{
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 8; ++j)
  {
    ok = ok && ray_valid(raw[j], any_weight);
    c.v[j] = entry_value(raw[j]);
  }
  c.valid = ok;
}

// The weights of T are >= 0 and sum to res^3 > 0: 8 positive corners give T > 0, 8 corners <= 0 give T <= 0.  Only a mixed cell is
// interpolated.
__device__ __forceinline__ void ray_cell_signs(const RayCell &c, bool &all_pos, bool &all_nonpos)
{
  all_pos = all_nonpos = true;
#pragma unroll
  for (int j = 0; j < 8; ++j)
  {
    all_pos = all_pos && c.v[j] > 0;
    all_nonpos = all_nonpos && c.v[j] <= 0;
  }
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

// A ray and its sample.  p_k = o + trunc(d k step / L) per axis is carried as quotient and remainder of |d| step k by L: adding the
// quotient and remainder of |d| step by L and one conditional carry gives the next sample exactly (|d| <= L, so the quotient is at
// most k step <= max_range and the remainder stays below L < 2^31; all of it 32-bit).  trunc is odd, so the sign of d goes on
// afterwards.
struct RayWalk
{
  int64_t d[3];
  uint32_t L;
  uint32_t qd[3], rd[3], q[3], r[3]; // |d| step = qd L + rd; the sample's offset from the origin is q (remainder r), sign of d
  int32_t sgn[3];

  // ray i of the call; false: a dead ray (a component beyond 2^30, or L == 0)
  __device__ __forceinline__ bool start(const RayCommon &a, uint32_t i)
  {
    bool live = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      d[k] = (int64_t)a.dirs[3 * (size_t)i + k];
      if (a.flags & WS_RAYCAST_TARGETS) d[k] -= (int64_t)a.origin[k];
      if (d[k] <= -(1ll << 30) || d[k] >= (1ll << 30)) live = false;
    }
    L = live ? isqrt_u64((uint64_t)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) : 0u;
    if (L == 0u) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      const uint64_t m = (uint64_t)(d[k] < 0 ? -d[k] : d[k]) * (uint64_t)a.step; // < 2^39
      const uint64_t qq = (uint64_t)div_trunc_i64((int64_t)m, (int64_t)L);
      qd[k] = (uint32_t)qq; // <= step
      rd[k] = (uint32_t)(m - qq * (uint64_t)L);
      sgn[k] = d[k] < 0 ? -1 : (d[k] > 0 ? 1 : 0);
      q[k] = r[k] = 0u;
    }
    return true;
  }
  // p_k, its base voxel and the fractions, from q
  __device__ __forceinline__ void sample(const RayCommon &a, int32_t p[3], int32_t b[3], int32_t f[3]) const
  {
#pragma unroll
    for (int x = 0; x < 3; ++x)
    {
      p[x] = a.origin[x] + sgn[x] * (int32_t)q[x];
      b[x] = floor_div(p[x] - a.half, a.rdiv, f[x]);
    }
  }
  // k -> k + 1
  __device__ __forceinline__ void advance()
  {
#pragma unroll
    for (int x = 0; x < 3; ++x)
    {
      q[x] += qd[x];
      r[x] += rd[x]; // < 2 L < 2^32
      if (r[x] >= L)
      {
        r[x] -= L;
        q[x] += 1u;
      }
    }
  }
  // quotient and remainder of sample k, k step <= max_range < 2^31: |d| step k < 2^61, one multiply and one division per axis
  __device__ __forceinline__ void seed(const RayCommon &a, uint32_t k)
  {
#pragma unroll
    for (int x = 0; x < 3; ++x)
    {
      const uint64_t m = (uint64_t)(d[x] < 0 ? -d[x] : d[x]) * ((uint64_t)a.step * (uint64_t)k);
      const uint64_t qq = (uint64_t)div_trunc_i64((int64_t)m, (int64_t)L);
      q[x] = (uint32_t)qq;
      r[x] = (uint32_t)(m - qq * (uint64_t)L);
    }
  }
  // The first sample k with  sgn (p_k - o) >= Q  on axis x, i.e. floor(|d| step k / L) >= Q: k = ceil(Q L / (|d| step)).  Q >= 1;
  // a Q beyond max_range is never reached (the offset is at most k step <= max_range): UINT32_MAX.  Q L < 2^31 2^31: 64 bits hold it.
  __device__ __forceinline__ uint32_t first_at(const RayCommon &a, int x, int64_t Q) const
  {
    if (sgn[x] == 0 || Q > (int64_t)a.K * (int64_t)a.step) return 0xffffffffu;
    if (Q <= 0) return 0u;
    const uint64_t m = (uint64_t)(d[x] < 0 ? -d[x] : d[x]) * (uint64_t)a.step, num = (uint64_t)Q * (uint64_t)L;
    uint64_t k = (uint64_t)div_trunc_i64((int64_t)num, (int64_t)m);
    if (k * m < num) ++k;
    return k > 0xfffffffeull ? 0xffffffffu : (uint32_t)k;
  }
  // the first sample whose base voxel on axis x is >= v (sgn > 0) / <= v (sgn < 0):  b >= v  iff  p - half >= v res,
  // b <= v  iff  p - half <= v res + res - 1.  v is 64-bit: the voxel behind the last chunk of int32 voxel space is 2^31
  __device__ __forceinline__ uint32_t first_voxel(const RayCommon &a, int x, int64_t v) const
  {
    const int64_t edge = v * (int64_t)a.res + (int64_t)a.half - (int64_t)a.origin[x];
    return first_at(a, x, sgn[x] > 0 ? edge : -(edge + (int64_t)a.res - 1));
  }
};

// the crossing between sample k - 1 (T0 > 0) and sample k (T <= 0): the range t and the hit point
__device__ __forceinline__ ri32x4 ray_crossing(const RayCommon &a, const RayWalk &w, uint32_t k, int64_t T0, int64_t T)
{
  // step T0 < 2^56, the divisor in (0, 2^47)
  const uint64_t t = (uint64_t)(k - 1u) * (uint64_t)a.step + ((uint64_t)a.step * (uint64_t)T0) / (uint64_t)(T0 - T);
  ri32x4 out;
  out.x = a.origin[0] + (int32_t)div_trunc_i64(w.d[0] * (int64_t)t, (int64_t)w.L); // |d t| < 2^61
  out.y = a.origin[1] + (int32_t)div_trunc_i64(w.d[1] * (int64_t)t, (int64_t)w.L);
  out.z = a.origin[2] + (int32_t)div_trunc_i64(w.d[2] * (int64_t)t, (int64_t)w.L);
  out.w = (int32_t)t;
  return out;
}

// The march of ray i: its record.  What it does not do per sample:
//   * divide (RayWalk); the base voxel floor((p - h) / res) is a multiply-shift (FastDiv, prepared on the host).
//   * gather a cell twice.  step = res / 2: the base voxel often stays; the 8 corner values and the cell's validity are kept
//     while it does.
//   * evaluate T where its sign is known (ray_cell_signs).  At a crossing both T are computed in full (T_{k-1} from a fresh gather
//     of its cell: once per ray).
//   * go on when nothing can follow: the ray ends at its hit, and where the field says it is gone.
//   * walk through what the field knows to be empty (Field::JUMPS): the samples up to resume() have invalid cells, so the state
//     after the jump is "previous sample not in front".
template <class Field> __device__ __forceinline__ ri32x4 ray_march(const RayCommon &a, Field &fld, uint32_t i)
{
  const bool any_weight = (a.flags & WS_RAYCAST_ANY_WEIGHT) != 0;
  ri32x4 out = {0, 0, 0, -1};
  RayWalk w;
  if (!w.start(a, i)) return out;
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
    w.sample(a, p, b, f);
    if (fld.gone(b, w.sgn)) break;
    if (b[0] != cb[0] || b[1] != cb[1] || b[2] != cb[2])
    {
      fld.load(b, any_weight, cell);
      cb[0] = b[0], cb[1] = b[1], cb[2] = b[2];
      if (cell.valid) ray_cell_signs(cell, all_pos, all_nonpos);
      if (Field::JUMPS && !cell.valid)
      {
        const uint32_t kn = fld.resume(w, a, b, k);
        if (kn > k + 1u)
        {
          if (kn > a.K) break;
          w.seed(a, kn);
          prev_front = false;
          k = kn - 1u;
          continue;
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
      fld.load(b0, any_weight, c0); // (valid: it was when the sample before was classified)
      out = ray_crossing(a, w, k, ray_cell_T(c0, f0, a.res), T);
      break;
    }
    prev_front = front;
#pragma unroll
    for (int x = 0; x < 3; ++x) pp[x] = p[x];
    w.advance();
  }
  return out;
}

// the hit counter: an integer sum, one add per wave (every lane of the wave calls this)
__device__ __forceinline__ void ray_count_hits(const ri32x4 &out, unsigned long long *hits)
{
  const unsigned long long hit = __ballot(out.w >= 0);
  if ((threadIdx.x & 63u) == 0 && hit) atomicAdd(hits, (unsigned long long)__popcll(hit));
}

// the central differences at voxel c, if all six neighbours are valid; else 0, 0, 0
template <class Field> __device__ __forceinline__ void ray_gradient_at(const Field &fld, const int32_t c[3], bool any_weight, int32_t g[3])
{
  g[0] = g[1] = g[2] = 0;
  if (!fld.grad_inside(c)) return;
  bool ok = true;
  int32_t diff[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    int32_t v[3] = {c[0], c[1], c[2]};
    uint32_t hi = 0u, lo = 0u;
    v[k] = c[k] + 1;
    ok = fld.entry(v, hi) && ok;
    v[k] = c[k] - 1;
    ok = fld.entry(v, lo) && ok;
    ok = ok && ray_valid(hi, any_weight) && ray_valid(lo, any_weight);
    diff[k] = entry_value(hi) - entry_value(lo);
  }
  if (ok) g[0] = diff[0], g[1] = diff[1], g[2] = diff[2];
}

// the gradient of ray i from its record: at g = floor(hit / res) the central differences, if all six neighbours are valid
template <class Field> __device__ __forceinline__ void ray_gradient(const RayCommon &a, const Field &fld, uint32_t i)
{
  const bool any_weight = (a.flags & WS_RAYCAST_ANY_WEIGHT) != 0;
  const ri32x4 rec = a.rec[i];
  int32_t g[3] = {0, 0, 0};
  if (rec.w >= 0)
  {
    const int32_t hp[3] = {rec.x, rec.y, rec.z};
    int32_t c[3], f;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = floor_div(hp[k], a.rdiv, f);
    ray_gradient_at(fld, c, any_weight, g);
  }
  a.grad[3 * (size_t)i + 0] = g[0];
  a.grad[3 * (size_t)i + 1] = g[1];
  a.grad[3 * (size_t)i + 2] = g[2];
}

} // namespace ws
