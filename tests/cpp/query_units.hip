// query_units.hip — the integer helpers of the map queries (ws_raycast.h, ws_sample.h, ws_mesh.h and the scan of ws_device.h), evaluated
// ON THE DEVICE and held to a plain restatement of the same operation over the domain each helper's exactness comment claims.  The
// restatement is computed in the same thread with int64 / uint64 and the built-in / and %, and with unsigned __int128 PRODUCTS where
// 64 bits do not hold an intermediate: it never calls div_trunc_i64, FastDiv or isqrt_u64, and it divides nothing wider than 64 bits
// (a quotient that needs 128 bits is stated as a product: floor(m k / L) >= Q  <=>  m k >= Q L).  Every mismatch is counted; the first
// few are recorded with their inputs.  Prints one line per helper, exits 1 on any mismatch.
//
// Where a comment claims more than a caller can send, the host-reachable domain is tested: raycast_check (ws_api.h) admits
// max_range >= 1, res <= 1024 and |origin| + max_range + 2 res <= INT32_MAX per axis; mesh_corners_fit (api_query.hip) admits box
// corners c with (|c| + 1) res <= INT32_MAX.
#include <cstdint>
#include <vector>

#include "ws_raycast.h"
#include "ws_sample.h"
#include "ws_mesh.h"

#include "unit_report.hpp"

using namespace ws;
typedef unsigned __int128 u128;

// RESLIST: 1 is admitted by the store only (half = 0); 1024 is the largest admitted (res^3 = 2^30: the int32 weight product of
// ray_cell_T at its limit)
constexpr int N_RESLIST = 7;
__constant__ int32_t c_reslist[N_RESLIST] = {1, 2, 3, 50, 64, 1023, 1024};
static const int32_t h_reslist[N_RESLIST] = {1, 2, 3, 50, 64, 1023, 1024};
__constant__ int32_t c_extreme[5] = {-32768, -1, 0, 1, 32767};

__host__ __device__ inline int64_t floor_i64(int64_t x, int64_t d, int64_t &f) // d > 0
{
  int64_t q = x / d;
  f = x % d;
  if (f < 0)
  {
    f += d;
    q -= 1;
  }
  return q;
}

// ---- floor_div(x, make_fastdiv(res), f): fd[r] is make_fastdiv(r), prepared on the host as ray_common / sample_common do.
// i < 7 2^32: every int32 x for the resolutions of RESLIST; then 2^24 random x for each other resolution of 1 .. 1024 (`others`)
constexpr uint64_t FLOOR_ALL = (uint64_t)N_RESLIST << 32, FLOOR_RANDOM = (uint64_t)(1024 - N_RESLIST) << 24;
__global__ void k_floor_div(const FastDiv *fd, const int32_t *others, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    int32_t res, x;
    if (i < FLOOR_ALL)
      res = c_reslist[i >> 32], x = (int32_t)(uint32_t)i;
    else
      res = others[(i - FLOOR_ALL) >> 24], x = (int32_t)(uint32_t)mix64(i);
    int32_t f;
    const int32_t q = floor_div(x, fd[res], f);
    if ((int64_t)q * res + f != (int64_t)x || f < 0 || f >= res) fail(rep, x, res, f, 0, q, (long long)x / res);
    ++c;
  }
  count(rep, c);
}

// ---- isqrt_u64(s): k^2 - 1, k^2, k^2 + 1 for every k in [1, 2^31) (the largest: (2^31 - 1)^2 + 1 < 2^62), then s = 0, the largest
// L^2 a live ray has, 3 (2^30 - 1)^2, and 2^28 random s of every magnitude below 2^62
constexpr uint64_t ISQRT_SQUARES = 3 * ((1ull << 31) - 1), ISQRT_CASES = ISQRT_SQUARES + 2 + (1ull << 28);
__global__ void k_isqrt(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    uint64_t s;
    if (i < ISQRT_SQUARES)
    {
      const uint64_t k = i / 3 + 1;
      s = k * k + (i % 3) - 1;
    }
    else if (i == ISQRT_SQUARES)
      s = 0;
    else if (i == ISQRT_SQUARES + 1)
      s = 3 * ((1ull << 30) - 1) * ((1ull << 30) - 1);
    else
    {
      const uint64_t h = mix64(i);
      s = h >> (2 + mix64(h) % 62);
    }
    const uint64_t r = isqrt_u64(s);
    if (!(r * r <= s && s < (r + 1) * (r + 1))) fail(rep, (long long)s, 0, 0, 0, (long long)r, 0);
    ++c;
  }
  count(rep, c);
}

// ---- ray_cell_fill + ray_cell_T + ray_cell_signs.  Enumerated: res of RESLIST, f per axis from {0, 1, res / 2, res - 1} (held to
// f <= res - 1, the helper's domain: at res 1 and 2 values of the list coincide), the corner values all 5^8 combinations of the
// extremes; then 2^26 random raw entries with random res in 1 .. 1024 and f in [0, res).  The weights are random everywhere.
constexpr uint64_t CELL_ENUM = (uint64_t)N_RESLIST * 64 * 390625, CELL_CASES = CELL_ENUM + (1ull << 26);
__global__ void k_cell_T(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    uint32_t raw[8];
    int32_t f[3], res;
    const uint64_t h = mix64(i), g = mix64(h), e = mix64(g), d = mix64(e);
    const uint64_t wsrc[4] = {h, g, e, d};
    const bool any_weight = (h >> 63) != 0;
    if (i < CELL_ENUM)
    {
      uint64_t t = i;
      for (int j = 0; j < 8; ++j)
      {
        // three corners in four with a positive weight, so that whole cells are valid often enough
        uint32_t w = (uint32_t)(wsrc[j >> 1] >> (32 * (j & 1)));
        if (w & 0x30000u) w = (w & 0x7fffu) | 1u;
        raw[j] = pack_entry(c_extreme[t % 5], (int32_t)(int16_t)w);
        t /= 5;
      }
      res = c_reslist[t / 64];
      for (int k = 0; k < 3; ++k)
      {
        const int32_t pick[4] = {0, 1, res / 2, res - 1};
        f[k] = min(pick[(t >> (2 * k)) & 3], res - 1);
      }
    }
    else
    {
      for (int j = 0; j < 8; ++j) raw[j] = (uint32_t)(wsrc[j >> 1] >> (32 * (j & 1)));
      const uint64_t u = mix64(d);
      res = 1 + (int32_t)(u % 1024);
      for (int k = 0; k < 3; ++k) f[k] = (int32_t)((u >> (10 + 16 * k)) & 0xffffu) % res;
    }
    RayCell cell;
    ray_cell_fill(raw, any_weight, cell);
    bool all_pos, all_nonpos;
    ray_cell_signs(cell, all_pos, all_nonpos);
    const int64_t T = ray_cell_T(cell, f, res);
    // the restatement: the eight products in int64 throughout
    int64_t want = 0;
    bool valid = true, pos = true, nonpos = true;
    for (int j = 0; j < 8; ++j)
    {
      const int64_t v = (int16_t)(raw[j] & 0xffffu), wt = (int16_t)(raw[j] >> 16);
      const int64_t wx = (j & 4) ? f[0] : res - f[0], wy = (j & 2) ? f[1] : res - f[1], wz = (j & 1) ? f[2] : res - f[2];
      want += v * (wx * wy * wz);
      valid = valid && (any_weight ? wt != 0 : wt > 0);
      pos = pos && v > 0;
      nonpos = nonpos && v <= 0;
      if (cell.v[j] != v) fail(rep, raw[j], j, 0, 1, cell.v[j], v);
    }
    const int64_t res3 = (int64_t)res * res * res, lim = 32768 * res3;
    if (T != want) fail(rep, (long long)i, res, f[0] | (f[1] << 10) | (f[2] << 20), 0, T, want);
    if (want > lim || want < -lim) fail(rep, (long long)i, res, 0, 2, want, lim);
    if (cell.valid != valid || all_pos != pos || all_nonpos != nonpos) fail(rep, (long long)i, res, 0, 3, cell.valid | (all_pos << 1) | (all_nonpos << 2), valid | (pos << 1) | (nonpos << 2));
    if ((all_pos && !(T > 0)) || (all_nonpos && !(T <= 0))) fail(rep, (long long)i, res, 0, 4, T, want);
    ++c;
  }
  count(rep, c);
}

// ---- sample_floor_T(T, res^3) and sample_class.  Enumerated: every res in 1 .. 1024, T = q res^3 + {-1, 0, 1} for every q in
// [-32768, 32767] (the largest |T|: 2^45 + 1); then 2^26 random T.  The comment claims |T| < 2^46, but the int32 result holds the
// floor only for what ray_cell_T can give, |T| <= 2^15 res^3: the random T are drawn from [-2^15 res^3, 2^15 res^3).  Four checks per
// T: the floor, and the class at band 1, tau (1000, the suite's) and 32767.
constexpr uint64_t FLOORT_ENUM = 1024ull * 65536 * 3, FLOORT_T = FLOORT_ENUM + (1ull << 26);
__global__ void k_floor_T(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    int64_t res, T;
    if (i < FLOORT_ENUM)
    {
      res = 1 + (int64_t)(i / (65536 * 3));
      const uint64_t t = i % (65536 * 3);
      T = ((int64_t)(t / 3) - 32768) * (res * res * res) + (int64_t)(t % 3) - 1;
    }
    else
    {
      const uint64_t h = mix64(i);
      res = 1 + (int64_t)(h % 1024);
      T = (int64_t)(mix64(h) % (uint64_t)(65536 * res * res * res)) - 32768 * res * res * res;
    }
    const int64_t res3 = res * res * res;
    const int32_t got = sample_floor_T(T, res3);
    int64_t want = T / res3;
    if (T % res3 != 0 && T < 0) want -= 1;
    if ((int64_t)got != want) fail(rep, T, res, 0, 0, got, want);
    const int32_t bands[3] = {1, 1000, 32767};
    for (int b = 0; b < 3; ++b)
    {
      const int64_t band = bands[b];
      // FREE d >= band, SURFACE -band < d < band, INSIDE d <= -band (warpsense_hip.h at ws_map_sample)
      const uint32_t cls = (-band < want && want < band) ? 2u : (want >= band ? 1u : 3u);
      const uint32_t gc = sample_class((int32_t)want, bands[b]);
      if (gc != cls) fail(rep, T, res, band, 1, gc, cls);
    }
    c += 4;
  }
  count(rep, c);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The rays of the three RayWalk lines.  A ray is what a caller passes: origin, three int32 (a direction, or a target point under
// WS_RAYCAST_TARGETS), the resolution and max_range.  gen_ray is host and device code: the host walks the same rays to state the
// number of cases.
struct RaySpec
{
  int32_t in[3], origin[3];
  uint32_t flags;
  int32_t res, max_range;
};
constexpr int64_t DMAX = (1ll << 30) - 1; // the largest live component (RayWalk::start; warpsense_hip.h: |component| < 2^30)
struct Rng
{
  uint64_t s;
  __host__ __device__ uint64_t next() { return s = mix64(s); }
  // a signed value of every magnitude up to +-DMAX
  __host__ __device__ int64_t component()
  {
    const uint64_t h = next();
    const int64_t m = (int64_t)((h >> 34) >> (mix64(h) % 30)); // 0 .. 2^30 - 1
    return (h & 1) ? -m : m;
  }
};
__host__ __device__ inline int64_t clamp_i32(int64_t v) { return v < INT32_MIN ? INT32_MIN : (v > INT32_MAX ? INT32_MAX : v); }

__host__ __device__ inline void gen_ray(uint64_t id, RaySpec &s)
{
  Rng r = {mix64(id ^ 0xA5A5A5A5F00DULL)};
  // step 1 (res 1, 2, 3), 25 (res 50, 51), 512 (res 1024): step = max(res / 2, 1), ray_common (ws_raycast.h)
  const uint32_t sk = (uint32_t)(id % 3), rk = (uint32_t)((id / 3) % 3);
  s.res = sk == 0 ? 1 + (int32_t)rk : (sk == 1 ? 50 + (int32_t)(rk & 1) : 1024);
  const int64_t step = s.res / 2 > 1 ? s.res / 2 : 1;
  const int64_t room = (int64_t)INT32_MAX - 2 * s.res; // |origin| + max_range <= room: raycast_check, ws_api.h "|origin| + max_range + 2 res does not fit int32"
  const uint32_t mode = (uint32_t)((id / 9) % 4);
  int64_t o[3] = {0, 0, 0}, mr;
  if (mode == 0)
    mr = room; // origin 0: the largest max_range that check admits, K step up to 2^31 - 1 - 2 res
  else if (mode == 1)
  {
    // origins near the int32 ends: max_range small, |origin| the largest the check admits on one axis at least
    mr = 1 + (int64_t)(r.next() % (1u << 20));
    const uint64_t h = r.next();
    for (int k = 0; k < 3; ++k)
    {
      const int64_t a = room - mr - (((h >> (8 * k)) & 3) ? (int64_t)((h >> (8 * k + 2)) & 63) : 0);
      o[k] = ((h >> (40 + k)) & 1) ? -a : a;
    }
    o[h % 3] = ((h >> 50) & 1) ? -(room - mr) : room - mr;
  }
  else
  {
    for (int k = 0; k < 3; ++k) o[k] = r.component();
    // any range the check admits beside such an origin, of every magnitude; or (mode 3) a range of a few steps: K = 0, 1, 2, 3
    mr = mode == 2 ? 1 + (int64_t)((r.next() % (uint64_t)(room - DMAX)) >> (r.next() % 31)) : 1 + (int64_t)(r.next() % (uint64_t)(4 * step - 1));
  }
  s.max_range = (int32_t)mr;
  for (int k = 0; k < 3; ++k) s.origin[k] = (int32_t)o[k];
  s.flags = 0;
  int64_t d[3] = {0, 0, 0};
  const uint32_t cat = (uint32_t)((id / 36) % 16);
  const uint64_t h = r.next();
  const int ax = (int)(h % 3);
  const int64_t sa = (h & 8) ? -1 : 1, sb = (h & 16) ? -1 : 1, sc = (h & 32) ? -1 : 1;
  switch (cat)
  {
  case 6: // axis-aligned, every magnitude; 1 and DMAX among them
    d[ax] = ((h >> 8) & 7) == 0 ? sa : (((h >> 8) & 7) == 1 ? sa * DMAX : r.component());
    break;
  case 7: // one component +-1 beside two of +-DMAX: L just below 2^30 sqrt(2)
    d[ax] = sa, d[(ax + 1) % 3] = sb * DMAX, d[(ax + 2) % 3] = sc * DMAX;
    break;
  case 8: // exact Pythagorean multiples (3, 4, 0) j and (2, 3, 6) j: L^2 is the perfect square (5 j)^2 / (7 j)^2
  {
    const bool two = (h >> 8) & 1;
    const int64_t jmax = two ? DMAX / 6 : DMAX / 4;
    const int64_t j = ((h >> 9) & 3) == 0 ? jmax : 1 + (int64_t)((r.next() % (uint64_t)jmax) >> (r.next() % 28));
    d[ax] = sa * (two ? 2 : 3) * j, d[(ax + 1) % 3] = sb * (two ? 3 : 4) * j, d[(ax + 2) % 3] = two ? sc * 6 * j : 0;
    break;
  }
  case 9: // L^2 one below a perfect square: x = (y^2 + z^2) / 2 with y, z of one parity gives x^2 + y^2 + z^2 = (x + 1)^2 - 1
  {
    int64_t y = 1 + (int64_t)((r.next() % 32767) >> (r.next() % 15)), z = (int64_t)((r.next() % 32767) >> (r.next() % 15));
    if ((y ^ z) & 1) z += 1; // y, z <= 32767: x < 2^30
    d[ax] = sa * ((y * y + z * z) / 2), d[(ax + 1) % 3] = sb * y, d[(ax + 2) % 3] = sc * z;
    break;
  }
  case 10: // (0, 0, 0): L == 0, dead
    break;
  case 11: // a component of exactly +-2^30: dead
    for (int k = 0; k < 3; ++k) d[k] = r.component();
    d[ax] = sa * (1ll << 30);
    break;
  case 14:
  case 15: // short directions, as the suite's
    for (int k = 0; k < 3; ++k) d[k] = (int64_t)(r.next() % 65537) - 32768;
    break;
  default: // 0 .. 5 random directions of every magnitude; 12, 13 targets
    for (int k = 0; k < 3; ++k) d[k] = r.component();
  }
  if (cat == 12 || cat == 13)
  {
    // WS_RAYCAST_TARGETS: the three int32 are points, d = point - origin in int64 (RayWalk::start).  12: points around the origin
    // (held to int32); 13: any int32 point (|d| up to 2^32 beside an origin at an int32 end: mostly dead)
    s.flags = WS_RAYCAST_TARGETS;
    for (int k = 0; k < 3; ++k) d[k] = cat == 12 ? clamp_i32(o[k] + d[k]) : (int64_t)(int32_t)(uint32_t)r.next();
  }
  for (int k = 0; k < 3; ++k) s.in[k] = (int32_t)d[k];
}
// d of the rule, and whether the ray is live: every |component| < 2^30 and L != 0 (L = 0 only for d = 0: floor(sqrt(s)) >= 1 for s >= 1)
__host__ __device__ inline bool ray_dir(const RaySpec &s, int64_t d[3])
{
  bool live = true, any = false;
  for (int k = 0; k < 3; ++k)
  {
    d[k] = (int64_t)s.in[k] - ((s.flags & WS_RAYCAST_TARGETS) ? (int64_t)s.origin[k] : 0);
    live = live && d[k] >= -DMAX && d[k] <= DMAX;
    any = any || d[k] != 0;
  }
  return live && any;
}
__host__ __device__ inline int64_t ray_step(const RaySpec &s) { return s.res / 2 > 1 ? s.res / 2 : 1; }
__host__ __device__ inline int64_t ray_K(const RaySpec &s) { return s.max_range / ray_step(s); }
// the call's constants as ray_common (ws_raycast.h) sets them, without a result holder
__device__ inline RayCommon common_of(const RaySpec &s, const int32_t *dirs)
{
  RayCommon a;
  for (int k = 0; k < 3; ++k) a.origin[k] = s.origin[k];
  a.dirs = dirs;
  a.n = 1;
  a.res = s.res;
  a.half = s.res / 2;
  a.step = s.res / 2 > 1 ? s.res / 2 : 1;
  a.K = (uint32_t)(s.max_range / a.step);
  a.rdiv = make_fastdiv(s.res);
  a.flags = s.flags;
  a.rec = nullptr;
  a.grad = nullptr;
  a.hits = nullptr;
  return a;
}
constexpr uint64_t N_RAYS = 1ull << 22;

// the states the steps line looks at: min(K, 64) advances from 0, then twice a seed followed by up to 8 advances
__host__ __device__ inline uint64_t walk_k0(const RaySpec &s, uint64_t id, int which)
{
  const uint64_t K = (uint64_t)ray_K(s);
  if (K <= 8) return 0;
  return which == 0 ? mix64(id ^ 0x5EEDull) % (K - 8 + 1) : K - 8; // random in [0, K - 8]; and the one whose 8 advances end at K
}
__host__ __device__ inline uint64_t walk_cases(const RaySpec &s)
{
  const uint64_t K = (uint64_t)ray_K(s), nadv = K < 64 ? K : 64, na = K < 8 ? K : 8;
  return 1 + (nadv + 1) + 2 * (na + 1);
}

// state of sample k: q L + r == |d| step k with r < L per axis (below 2^61: |d| < 2^30, step k <= max_range < 2^31), and p, b, f of
// sample() against the int64 floor
__device__ void check_state(const RayCommon &a, const RayWalk &w, const int64_t d[3], uint64_t k, uint64_t id, Report *rep)
{
  int32_t p[3], b[3], f[3];
  w.sample(a, p, b, f);
  for (int x = 0; x < 3; ++x)
  {
    const uint64_t ad = (uint64_t)(d[x] < 0 ? -d[x] : d[x]), m = ad * (uint64_t)a.step * k;
    if ((uint64_t)w.q[x] * (uint64_t)w.L + (uint64_t)w.r[x] != m || w.r[x] >= w.L) fail(rep, (long long)id, (long long)k, x, 0, ((long long)w.q[x] << 32) | w.r[x], (long long)(m / w.L));
    const int64_t pw = (int64_t)a.origin[x] + (d[x] < 0 ? -1 : 1) * (int64_t)(m / (uint64_t)w.L);
    int64_t fw;
    const int64_t bw = floor_i64(pw - a.half, a.res, fw);
    if (p[x] != pw || b[x] != bw || f[x] != fw) fail(rep, (long long)id, (long long)k, x, 1, p[x], pw);
  }
}

__global__ void k_walk_steps(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(id, base, n)
  {
    RaySpec s;
    gen_ray(id, s);
    int64_t d[3];
    const bool want_live = ray_dir(s, d);
    const RayCommon a = common_of(s, s.in);
    RayWalk w;
    const bool live = w.start(a, 0);
    if (live != want_live) fail(rep, (long long)id, d[0], d[1], d[2], live, want_live);
    ++c;
    if (!live || !want_live) continue;
    const uint64_t ss = (uint64_t)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), L = w.L;
    if (!(L * L <= ss && ss < (L + 1) * (L + 1))) fail(rep, (long long)id, d[0], d[1], d[2], (long long)L, 0);
    for (int x = 0; x < 3; ++x)
    {
      const uint64_t m = (uint64_t)(d[x] < 0 ? -d[x] : d[x]) * (uint64_t)a.step; // < 2^39
      const int32_t sg = d[x] < 0 ? -1 : (d[x] > 0 ? 1 : 0);
      if ((uint64_t)w.qd[x] * L + w.rd[x] != m || w.rd[x] >= L || w.sgn[x] != sg || w.d[x] != d[x]) fail(rep, (long long)id, d[x], x, 2, ((long long)w.qd[x] << 32) | w.rd[x], (long long)(m / L));
    }
    const uint64_t K = a.K, nadv = K < 64 ? K : 64, na = K < 8 ? K : 8;
    for (uint64_t k = 0; k <= nadv; ++k)
    {
      check_state(a, w, d, k, id, rep);
      if (k < nadv) w.advance();
    }
    for (int t = 0; t < 2; ++t)
    {
      const uint64_t k0 = walk_k0(s, id, t);
      w.seed(a, (uint32_t)k0);
      for (uint64_t j = 0; j <= na; ++j)
      {
        check_state(a, w, d, k0 + j, id, rep);
        if (j < na) w.advance();
      }
    }
    c += (nadv + 1) + 2 * (na + 1);
  }
  count(rep, c);
}

// first_at's answer for Q on axis x.  UINT32_MAX iff the axis does not move, or Q > K step, or the ceiling exceeds 0xfffffffe;
// otherwise the first k with m k >= Q L, as 128-bit products (m < 2^39, k < 2^32, Q L < 2^62)
__device__ bool first_at_ok(const RayCommon &a, const RayWalk &w, const int64_t d[3], int x, int64_t Q, uint32_t k)
{
  const uint64_t m = (uint64_t)(d[x] < 0 ? -d[x] : d[x]) * (uint64_t)a.step;
  const int64_t KS = (int64_t)a.K * (int64_t)a.step;
  if (d[x] == 0 || Q > KS) return k == 0xffffffffu;
  if (Q <= 0) return k == 0u; // m 0 >= Q L, and no k - 1 >= 0 has m (k - 1) < Q L <= 0
  const u128 QL = (u128)(uint64_t)Q * (u128)w.L;
  if ((u128)m * (u128)0xfffffffeull < QL) return k == 0xffffffffu;
  return k != 0xffffffffu && (u128)m * (u128)k >= QL && (k == 0u || (u128)m * (u128)(k - 1u) < QL);
}
constexpr uint64_t FIRST_Q = 9, FIRST_V = 12, FIRST_PER_RAY = 3 * (FIRST_Q + FIRST_V);
__global__ void k_first_at(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(id, base, n)
  {
    RaySpec s;
    gen_ray(id, s);
    int64_t d[3];
    if (!ray_dir(s, d)) continue; // (dead rays: the steps line)
    const RayCommon a = common_of(s, s.in);
    RayWalk w;
    if (!w.start(a, 0)) continue; // (counted short: the line fails)
    Rng r = {mix64(id ^ 0xF125ull)};
    const int64_t KS = (int64_t)a.K * (int64_t)a.step;
    for (int x = 0; x < 3; ++x)
    {
      const int64_t Qs[FIRST_Q] = {0, -(int64_t)(r.next() >> (1 + r.next() % 63)), 1, 2, 1 + (int64_t)(r.next() % (uint64_t)(KS > 0 ? KS : 1)), KS - 1, KS, KS + 1, 1ll << 31};
      for (uint64_t j = 0; j < FIRST_Q; ++j)
      {
        const uint32_t k = w.first_at(a, x, Qs[j]);
        if (!first_at_ok(a, w, d, x, Qs[j], k)) fail(rep, (long long)id, x, Qs[j], 0, k, 0);
      }
      // voxels: around the origin's, one within reach, the last sample's and the one behind it, and up to the int32 voxel edges
      // (v is 64-bit: the voxel behind the last chunk of int32 voxel space is 2^31)
      const int64_t sg = d[x] < 0 ? -1 : 1, o = a.origin[x];
      int64_t ff;
      const int64_t v0 = floor_i64(o - a.half, a.res, ff), vK = floor_i64(o + sg * KS - a.half, a.res, ff);
      const int64_t vs[FIRST_V] = {v0 - 2, v0 - 1, v0, v0 + 1, v0 + 2, v0 + sg * (int64_t)(r.next() % (uint64_t)(KS / a.res + 2)), vK, vK + sg,
                                   floor_i64(INT32_MIN, a.res, ff), floor_i64(INT32_MAX, a.res, ff) + 1, -(1ll << 31), 1ll << 31};
      for (uint64_t j = 0; j < FIRST_V; ++j)
      {
        const int64_t v = vs[j];
        const uint32_t k = w.first_voxel(a, x, v);
        // b >= v  <=>  p - half >= v res  <=>  sgn (p - o) >= v res + half - o;   b <= v  <=>  p - half <= v res + res - 1
        const int64_t edge = v * a.res + a.half - o, Q = d[x] > 0 ? edge : -(edge + a.res - 1);
        bool ok = first_at_ok(a, w, d, x, Q, k);
        if (ok && k <= a.K)
        {
          // ... and through the walk itself: the base voxel of sample k has reached v, that of sample k - 1 has not
          RayWalk u = w;
          int32_t p[3], b[3], f[3];
          u.seed(a, k);
          u.sample(a, p, b, f);
          ok = d[x] > 0 ? (int64_t)b[x] >= v : (int64_t)b[x] <= v;
          if (k > 0)
          {
            u.seed(a, k - 1u);
            u.sample(a, p, b, f);
            ok = ok && (d[x] > 0 ? (int64_t)b[x] < v : (int64_t)b[x] > v);
          }
        }
        if (!ok) fail(rep, (long long)id, x, v, 1, k, Q);
      }
    }
    c += FIRST_PER_RAY;
  }
  count(rep, c);
}

// ---- ray_crossing(a, w, k, T0, T): T0 in (0, 2^45], T in [-2^45, 0] (|T| <= 2^15 res^3, res <= 1024), at their ends and random of
// every magnitude; k = 1, random, K.  Rays with K = 0 have no crossing.
constexpr uint64_t CROSS_PER_RAY = 6 * 3;
__global__ void k_crossing(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(id, base, n)
  {
    RaySpec s;
    gen_ray(id, s);
    int64_t d[3];
    if (!ray_dir(s, d) || ray_K(s) < 1) continue;
    const RayCommon a = common_of(s, s.in);
    RayWalk w;
    if (!w.start(a, 0)) continue; // (counted short: the line fails)
    Rng r = {mix64(id ^ 0xC055ull)};
    const int64_t TOP = 1ll << 45;
    const int64_t T0s[6] = {1, TOP, 1, TOP, 1 + (int64_t)(r.next() % (uint64_t)TOP), 1 + (int64_t)((r.next() % (uint64_t)TOP) >> (r.next() % 45))};
    const int64_t Ts[6] = {0, -TOP, -TOP, 0, -(int64_t)(r.next() % (uint64_t)(TOP + 1)), -(int64_t)((r.next() % (uint64_t)(TOP + 1)) >> (r.next() % 46))};
    const uint32_t ks[3] = {1u, 1u + (uint32_t)(r.next() % a.K), a.K};
    for (int j = 0; j < 6; ++j)
      for (int kk = 0; kk < 3; ++kk)
      {
        const uint32_t k = ks[kk];
        const ri32x4 got = ray_crossing(a, w, k, T0s[j], Ts[j]);
        // t = s_{k-1} + floor(step T0 / (T0 - T)), hit = o + trunc(d t / L) (warpsense_hip.h at ws_map_raycast)
        const int64_t t = (int64_t)(k - 1u) * a.step + (a.step * T0s[j]) / (T0s[j] - Ts[j]);
        const int64_t hx = a.origin[0] + (d[0] * t) / (int64_t)w.L, hy = a.origin[1] + (d[1] * t) / (int64_t)w.L, hz = a.origin[2] + (d[2] * t) / (int64_t)w.L;
        if (got.x != hx || got.y != hy || got.z != hz || got.w != t) fail(rep, (long long)id, k, T0s[j], Ts[j], got.w, t);
      }
    c += CROSS_PER_RAY;
  }
  count(rep, c);
}

// ---- crossing(va, vb, res) of the mesh: every pair of int16 values of which exactly one is negative, for each res of RESLIST
constexpr uint64_t MESHX_CASES = (uint64_t)N_RESLIST << 31;
__global__ void k_mesh_crossing(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const int32_t res = c_reslist[i >> 31];
    const int32_t neg = -1 - (int32_t)(i & 0x7fffu), pos = (int32_t)((i >> 15) & 0x7fffu);
    const int32_t va = ((i >> 30) & 1) ? pos : neg, vb = ((i >> 30) & 1) ? neg : pos;
    const int64_t ua = va < 0 ? -(int64_t)va : va, ub = vb < 0 ? -(int64_t)vb : vb, m = ua + ub;
    const int64_t want = (2 * ua * res + m) / (2 * m), got = crossing(va, vb, res);
    if (got != want || got < 0 || got > res) fail(rep, va, vb, res, 0, got, want);
    ++c;
  }
  count(rep, c);
}

// ---- mesh_vertex(raw, c3, res): 2^26 corner sets, random raw entries (negative weights among them: WS_MESH_ANY_WEIGHT) with the
// extreme values mixed in; res of RESLIST or random in 1 .. 1024; c3 per axis at 0, +-1, random, and at the ends of what the box check
// admits: mesh_corners_fit (api_query.hip) takes corners c with (|c| + 1) res <= INT32_MAX, and the cells of a box [lo, hi] are
// lo <= c3 <= hi - 1, so with M = INT32_MAX / res:  -(M - 1) <= c3 <= M - 2.  A cell without a crossing edge has no vertex under the
// rule (it is not active); the helper leaves it at the cell's corner c3 res + res / 2, which is what is asked of it here.
constexpr uint64_t VERTEX_CASES = 1ull << 26;
__global__ void k_mesh_vertex(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const uint64_t hs[5] = {mix64(i), mix64(i ^ (1ull << 40)), mix64(i ^ (2ull << 40)), mix64(i ^ (3ull << 40)), mix64(i ^ (4ull << 40))};
    uint32_t raw[8];
    for (int j = 0; j < 8; ++j)
    {
      raw[j] = (uint32_t)(hs[j >> 1] >> (32 * (j & 1)));
      const uint32_t pick = (uint32_t)((hs[4] >> (4 * j)) & 15u); // one corner in three at an extreme value
      if (pick < 5) raw[j] = (raw[j] & 0xffff0000u) | ((uint32_t)c_extreme[pick] & 0xffffu);
    }
    const uint64_t u = mix64(hs[4]);
    const int32_t res = (u & 1) ? c_reslist[(u >> 1) % N_RESLIST] : 1 + (int32_t)((u >> 1) % 1024);
    const int64_t M = INT32_MAX / res;
    int32_t c3[3];
    for (int k = 0; k < 3; ++k)
    {
      const uint64_t t = mix64(u + k);
      const int64_t pick[6] = {0, 1, -1, M - 2, -(M - 1), (int64_t)(t >> 8) % (2 * M - 2) - (M - 1)};
      c3[k] = (int32_t)pick[t % 6];
    }
    const mi32x4 got = mesh_vertex(raw, c3, res);
    // the rule (warpsense_hip.h at ws_map_mesh) in int64
    int64_t v[8], wmin = INT64_MAX, sum[3] = {0, 0, 0}, nx = 0;
    for (int k = 0; k < 8; ++k)
    {
      v[k] = (int16_t)(raw[k] & 0xffffu);
      const int64_t wt = (int16_t)(raw[k] >> 16);
      wmin = wt < 0 ? (-wt < wmin ? -wt : wmin) : (wt < wmin ? wt : wmin);
    }
    for (int ax = 0; ax < 3; ++ax)
      for (int k = 0; k < 8; ++k)
      {
        const int bit = 4 >> ax;
        if ((k & bit) || (v[k] < 0) == (v[k | bit] < 0)) continue;
        const int64_t ua = v[k] < 0 ? -v[k] : v[k], ub = v[k | bit] < 0 ? -v[k | bit] : v[k | bit], m = ua + ub;
        ++nx;
        for (int dd = 0; dd < 3; ++dd) sum[dd] += dd == ax ? (2 * ua * res + m) / (2 * m) : ((k & (4 >> dd)) ? res : 0);
      }
    const int32_t g[3] = {got.x, got.y, got.z};
    for (int dd = 0; dd < 3; ++dd)
    {
      const int64_t want = (int64_t)c3[dd] * res + res / 2 + (nx ? sum[dd] / nx : 0);
      if ((int64_t)g[dd] != want || want > INT32_MAX || want < INT32_MIN) fail(rep, (long long)i, res, c3[dd], dd, g[dd], want);
    }
    if ((int64_t)(uint32_t)got.w != wmin) fail(rep, (long long)i, res, 0, 3, (uint32_t)got.w, wmin);
    ++c;
  }
  count(rep, c);
}

// ---- block_scan_256: one value per thread; every fourth workgroup all 0xffffff (256 of them stay below 2^32), else random 24-bit counts
constexpr uint32_t SCAN_WGS = 1u << 12;
__global__ void k_block_scan(uint32_t *in, uint32_t *out)
{
  __shared__ uint32_t wsum[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cnt = (blockIdx.x & 3u) == 3u ? 0xffffffu : (uint32_t)mix64(i) & 0xffffffu;
  in[i] = cnt;
  out[i] = block_scan_256(cnt, wsum);
}

// ---- scan_block_totals (ws_device.h): one workgroup of 1024 threads, as the five kernels that share it launch it
__global__ void k_scan_totals(const uint32_t *tot, unsigned long long *off, uint32_t n, unsigned long long *total) { scan_block_totals(tot, off, n, total); }

int main()
{
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  const dim3 G(GRID), B(BLOCK);

  {
    std::vector<FastDiv> fd(1025);
    std::vector<int32_t> others;
    for (int32_t r = 1; r <= 1024; ++r)
    {
      fd[r] = make_fastdiv(r);
      bool listed = false;
      for (int32_t l : h_reslist) listed = listed || l == r;
      if (!listed) others.push_back(r);
    }
    fd[0] = fd[1];
    FastDiv *d_fd;
    int32_t *d_others;
    CHECK_HIP(hipMalloc((void **)&d_fd, fd.size() * sizeof(FastDiv)));
    CHECK_HIP(hipMalloc((void **)&d_others, others.size() * sizeof(int32_t)));
    CHECK_HIP(hipMemcpy(d_fd, fd.data(), fd.size() * sizeof(FastDiv), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_others, others.data(), others.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    begin();
    chunked(FLOOR_ALL + FLOOR_RANDOM, [&](uint64_t b, uint64_t n) { k_floor_div<<<G, B>>>(d_fd, d_others, b, n, g_rep); });
    finish("floor_div", FLOOR_ALL + ((uint64_t)others.size() << 24)); // 7 2^32 + 1017 2^24
    CHECK_HIP(hipFree(d_fd));
    CHECK_HIP(hipFree(d_others));
  }

  begin();
  chunked(ISQRT_CASES, [&](uint64_t b, uint64_t n) { k_isqrt<<<G, B>>>(b, n, g_rep); });
  finish("isqrt_u64", ISQRT_CASES);

  begin();
  k_cell_T<<<G, B>>>(0, CELL_CASES, g_rep);
  finish("ray_cell_T", CELL_CASES);

  begin();
  k_floor_T<<<G, B>>>(0, FLOORT_T, g_rep);
  finish("sample_floor_T", 4 * FLOORT_T);

  {
    // the same rays on the host: how many cases each line has to report
    unsigned long long walk = 0, first = 0, cross = 0, live = 0, dead_big = 0, dead_zero = 0;
    for (uint64_t id = 0; id < N_RAYS; ++id)
    {
      RaySpec s;
      gen_ray(id, s);
      int64_t d[3];
      const bool alive = ray_dir(s, d);
      walk += alive ? walk_cases(s) : 1;
      first += alive ? FIRST_PER_RAY : 0;
      cross += alive && ray_K(s) >= 1 ? CROSS_PER_RAY : 0;
      live += alive;
      if (!alive) (d[0] == 0 && d[1] == 0 && d[2] == 0 ? dead_zero : dead_big) += 1;
      // every ray is one raycast_check admits
      for (int k = 0; k < 3; ++k)
        if (s.max_range < 1 || (int64_t)(s.origin[k] < 0 ? -(int64_t)s.origin[k] : s.origin[k]) + s.max_range + 2 * (int64_t)s.res > (int64_t)INT32_MAX)
        {
          printf("RayWalk: ray %llu is not one the host check admits\n", (unsigned long long)id);
          g_bad = 1;
        }
    }
    if (live < N_RAYS / 2 || dead_big < N_RAYS / 32 || dead_zero < N_RAYS / 32)
    {
      printf("RayWalk: %llu live, %llu dead by a component, %llu dead by L == 0 of %llu rays\n", live, dead_big, dead_zero, (unsigned long long)N_RAYS);
      g_bad = 1;
    }
    begin();
    k_walk_steps<<<G, B>>>(0, N_RAYS, g_rep);
    finish("RayWalk steps", walk);
    begin();
    k_first_at<<<G, B>>>(0, N_RAYS, g_rep);
    finish("RayWalk first_at", first);
    begin();
    k_crossing<<<G, B>>>(0, N_RAYS, g_rep);
    finish("ray_crossing", cross);
  }

  begin();
  k_mesh_crossing<<<G, B>>>(0, MESHX_CASES, g_rep);
  finish("mesh crossing", MESHX_CASES);

  begin();
  k_mesh_vertex<<<G, B>>>(0, VERTEX_CASES, g_rep);
  finish("mesh_vertex", VERTEX_CASES);

  {
    const size_t n = (size_t)SCAN_WGS * 256;
    uint32_t *d_in, *d_out;
    CHECK_HIP(hipMalloc((void **)&d_in, n * 4));
    CHECK_HIP(hipMalloc((void **)&d_out, n * 4));
    CHECK_HIP(hipMemset(d_out, 0xff, n * 4));
    k_block_scan<<<dim3(SCAN_WGS), dim3(256)>>>(d_in, d_out);
    CHECK_HIP(hipGetLastError());
    std::vector<uint32_t> in(n), out(n);
    CHECK_HIP(hipMemcpy(in.data(), d_in, n * 4, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(out.data(), d_out, n * 4, hipMemcpyDeviceToHost));
    Report r = {};
    for (size_t b = 0; b < SCAN_WGS; ++b)
    {
      uint32_t run = 0;
      for (size_t t = 0; t < 256; ++t)
      {
        const size_t i = b * 256 + t;
        const uint32_t want_in = (b & 3) == 3 ? 0xffffffu : (uint32_t)mix64(i) & 0xffffffu;
        if (in[i] != want_in) host_fail(r, (long long)b, (long long)t, 0, 1, in[i], want_in);
        if (out[i] != run) host_fail(r, (long long)b, (long long)t, 0, 0, out[i], run);
        run += in[i];
        ++r.checked;
      }
    }
    finish_host("block_scan_256", r, n);
    CHECK_HIP(hipFree(d_in));
    CHECK_HIP(hipFree(d_out));
  }

  {
    // around one piece per thread (n <= 1024), two (the seg > 1 branch starts at 1025), three, five, and 257 with a ragged end
    const uint32_t ns[10] = {1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 262149};
    const uint32_t nmax = 262149;
    uint32_t *d_tot;
    unsigned long long *d_off, *d_total;
    CHECK_HIP(hipMalloc((void **)&d_tot, nmax * 4));
    CHECK_HIP(hipMalloc((void **)&d_off, (nmax + 1) * 8));
    d_total = d_off + nmax;
    Report r = {};
    unsigned long long expect = 0;
    std::vector<uint32_t> tot(nmax);
    std::vector<unsigned long long> off(nmax + 1);
    for (uint32_t n : ns)
      for (int fill = 0; fill < 2; ++fill)
      {
        for (uint32_t i = 0; i < n; ++i) tot[i] = fill ? 0xffffffffu : (uint32_t)mix64(((uint64_t)n << 32) | i); // all-ones: the sum passes 2^32
        CHECK_HIP(hipMemcpy(d_tot, tot.data(), n * 4, hipMemcpyHostToDevice));
        CHECK_HIP(hipMemset(d_off, 0xff, (nmax + 1) * 8));
        k_scan_totals<<<dim3(1), dim3(1024)>>>(d_tot, d_off, n, d_total);
        CHECK_HIP(hipGetLastError());
        CHECK_HIP(hipMemcpy(off.data(), d_off, (nmax + 1) * 8, hipMemcpyDeviceToHost));
        uint64_t run = 0;
        for (uint32_t i = 0; i < n; ++i)
        {
          if (off[i] != run) host_fail(r, n, i, fill, 0, (long long)off[i], (long long)run);
          run += tot[i];
        }
        if (off[nmax] != run) host_fail(r, n, n, fill, 1, (long long)off[nmax], (long long)run);
        // nothing behind the n offsets is written
        if (n < nmax && off[n] != ~0ull) host_fail(r, n, n, fill, 2, (long long)off[n], -1);
        r.checked += n + 1;
        expect += n + 1;
      }
    finish_host("scan_block_totals", r, expect); // 2 (275 465 + 10)
    CHECK_HIP(hipFree(d_tot));
    CHECK_HIP(hipFree(d_off));
  }

  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
