// device_units.hip — the fixed-point helpers of ws_device.h / ws_march.h, evaluated ON THE DEVICE and held to a plain int64 / double
// restatement of the same operation, computed in the same thread, over the domain each helper's exactness argument states.
// Every mismatch is counted; the first few are recorded with their inputs.  Prints one line per helper, exits 1 on any mismatch.
#include <cstdint>
#include <vector>

#include "ws_march.h"

#include "unit_report.hpp"

using namespace ws;

// trunc(x / d) as plain 64-bit arithmetic: q is it iff x - q d lies in [0, d) (x >= 0) or (-d, 0] (x < 0), q d of x's sign or 0
__device__ __forceinline__ bool is_trunc_quotient(int64_t x, int64_t d, int64_t q)
{
  const int64_t r = x - q * d;
  return x >= 0 ? (q >= 0 && r >= 0 && r < d) : (q <= 0 && r <= 0 && r > -d);
}

// ---- make_fastdiv_dev(d) == make_fastdiv(d) for every d in [1, 2^31)
__global__ void k_fastdiv(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const int32_t d = (int32_t)(i + 1);
    const FastDiv a = make_fastdiv_dev(d), b = make_fastdiv(d);
    if (a.M != b.M || a.k != b.k) fail(rep, d, 0, 0, 0, (long long)a.M, (long long)b.M);
    ++c;
  }
  count(rep, c);
}

// ---- div_trunc(x, fd): every int32 x for each divisor of the list
__global__ void k_div_trunc(const int32_t *divs, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const int32_t d = divs[i >> 32];
    const int32_t x = (int32_t)(uint32_t)i;
    const FastDiv f = make_fastdiv_dev(d);
    const int32_t q = div_trunc(x, f);
    if (!is_trunc_quotient(x, d, q)) fail(rep, x, d, 0, 0, q, (long long)x / d);
    ++c;
  }
  count(rep, c);
}

// ---- div_res(x, frame): every int32 x for the listed resolutions
__global__ void k_div_res_all(const MarchFrame *frames, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const MarchFrame &f = frames[i >> 32];
    const int32_t x = (int32_t)(uint32_t)i;
    const int32_t q = div_res(x, f);
    if (!is_trunc_quotient(x, f.res, q)) fail(rep, x, f.res, 0, 0, q, (long long)x / f.res);
    ++c;
  }
  count(rep, c);
}
// ... and for every res in [lo, lo + n_res): x = +-k res + {-1, 0, 1} (k small and k near the int32 limit), then random x.
// The frame is built in the thread (make_march_frame is host and device code).
constexpr int DIVRES_PER = 1 << 16;
__global__ void k_div_res_sampled(int32_t res_lo, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  const int32_t zero[3] = {0, 0, 0};
  const MapParams mp = {{3, 3, 3}, {0, 0, 0}, {0, 0, 0}};
  FOR_RANGE(i, base, n)
  {
    const int32_t res = res_lo + (int32_t)(i / DIVRES_PER);
    const uint32_t j = (uint32_t)(i % DIVRES_PER);
    const MarchFrame f = make_march_frame(zero, res, res, mp);
    int64_t x;
    if (j < DIVRES_PER / 2)
    {
      const int64_t kmax = INT32_MAX / res;
      const uint32_t t = j / 6, v = j % 6;
      const int64_t k = t < 2048 ? t : kmax - (t - 2048);
      x = (v & 1 ? -1 : 1) * k * res + (int64_t)(v >> 1) - 1;
      if (k < 0 || x > INT32_MAX || x < INT32_MIN) continue;
    }
    else
      x = (int32_t)(uint32_t)mix64(i);
    const int32_t q = div_res((int32_t)x, f);
    if (!is_trunc_quotient(x, res, q)) fail(rep, x, res, 0, 0, q, x / res);
    ++c;
  }
  count(rep, c);
}

// ---- div_res_b + ring_b and the mirrored ring_m: every millimetre y whose voxel trunc(y / res) lies in the window of axis 0 of
// the frame, against (trunc(y / res) - pos + offset) mod size
__global__ void k_ring(const MarchFrame *frames, int n_frames, uint64_t base, uint64_t n, const int64_t *first, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    int fi = 0;
    while (fi + 1 < n_frames && first[fi + 1] <= (int64_t)i) ++fi;
    const MarchFrame &f = frames[fi];
    const int32_t res = f.res, size = f.map.size[0], pos = f.map.pos[0], off = f.map.offset[0];
    const int64_t vlo = (int64_t)pos - size / 2, vhi = (int64_t)pos + size / 2;
    const int64_t ylo = vlo * res - (res - 1);
    const int64_t y = ylo + ((int64_t)i - first[fi]);
    const int64_t v = y / res;
    if (v < vlo || v > vhi) continue;
    const int64_t want = (((v - pos + off) % size) + size) % size;
    const int32_t got = ring_b(div_res_b((int32_t)y, f), f.ringB[0], size);
    if (got != want) fail(rep, y, res, pos, size, got, want);
    // mirrored: the walk of the free pass divides s y and puts the sign back in the ring constant (tsdf_free.hip, march_free)
    const uint32_t kc = (uint32_t)f.ringB[0] + 2u * (uint32_t)f.divBq + 1u;
    const int32_t gotm = ring_m(div_res_b((int32_t)-y, f), ~0u, kc, size);
    if (gotm != want) fail(rep, -y, res, pos, size, gotm, want);
    const int32_t gotp = ring_m(div_res_b((int32_t)y, f), 0u, (uint32_t)f.ringB[0], size);
    if (gotp != want) fail(rep, y, res, pos, size + (1ll << 32), gotp, want);
    c += 3;
  }
  count(rep, c);
}

// ---- iv_bias + trunc15_biased: trunc(m iv / 32768) for iv in [-32768, 32768], m in [0, 65536) (the fan offsets of the fast rays:
// m = delta_z <= 141 there; m |iv| < 2^31 and m < 2^23 are what the 24-bit multiply needs)
__global__ void k_trunc15(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const int32_t m = (int32_t)(i / 65537), iv = (int32_t)(i % 65537) - 32768;
    const int32_t got = trunc15_biased(m, iv, iv_bias(iv));
    const int64_t want = (int64_t)m * iv / MATRIX_RESOLUTION;
    if (got != want) fail(rep, m, iv, 0, 0, got, want);
    if (iv != MATRIX_RESOLUTION && trunc_shift15(m * iv) != want) fail(rep, m, iv, 1, 0, trunc_shift15(m * iv), want);
    ++c;
  }
  count(rep, c);
}

// ---- tsdf_weight: every value in [-tau, tau] for every tau in [1, 32767]; the plain form, the prepared division, the resolve's
// v_mul_hi_u32 form (tile_resolve_kernel) and tsdf_weight_is_zero
__global__ void k_weight(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const int32_t tau = 1 + (int32_t)(i / 65535), value = (int32_t)(i % 65535) - 32767;
    if (value < -tau || value > tau) continue;
    const int32_t eps = tau / 10;
    const int64_t want = value < -eps ? (int64_t)WEIGHT_RESOLUTION * (tau + value) / (tau - eps) : WEIGHT_RESOLUTION;
    const FastDiv wd = make_fastdiv(tau - eps);
    const int32_t a = tsdf_weight(value, tau, eps), b = tsdf_weight(value, tau, eps, wd);
    if (a != want) fail(rep, value, tau, 0, 0, a, want);
    if (b != want) fail(rep, value, tau, 1, 0, b, want);
    if (value < -eps)
    {
      const uint32_t wM32 = (uint32_t)wd.M;
      const int32_t wS = wd.k - 32;
      const int32_t r = (int32_t)(__umulhi((uint32_t)(WEIGHT_RESOLUTION * (tau + value)), wM32) >> wS);
      if (r != want) fail(rep, value, tau, 2, 0, r, want);
    }
    if (tsdf_weight_is_zero(value, tau, eps) != (want == 0)) fail(rep, value, tau, 3, 0, tsdf_weight_is_zero(value, tau, eps), want);
    ++c;
  }
  count(rep, c);
}

// ---- integrate_entry against the oracle's rule (wso_update_avg) in int64, then cast to int16
__device__ __forceinline__ uint32_t integrate_ref(uint32_t existing, uint32_t fresh, int32_t max_weight)
{
  const int64_t nv = (int16_t)(fresh & 0xffffu), nw = (int16_t)(fresh >> 16), ev = (int16_t)(existing & 0xffffu), ew = (int16_t)(existing >> 16);
  if (nw > 0 && ew > 0)
  {
    const int64_t v = (ev * ew + nv * nw) / (ew + nw);
    const int64_t w = max_weight < ew + nw ? max_weight : ew + nw;
    return ((uint32_t)(uint16_t)(int16_t)v) | ((uint32_t)(uint16_t)(int16_t)w << 16);
  }
  if (nw != 0 && ew <= 0) return fresh;
  return existing;
}
__constant__ int32_t c_mw[6] = {1, 64, 65, 640, 32767, 40000};
__constant__ int32_t c_edge[10] = {-32768, -32767, -2, -1, 0, 1, 2, 32766, 32767, 640};
__global__ void k_integrate_edges(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    uint64_t t = i;
    const int32_t ev = c_edge[t % 10]; t /= 10;
    const int32_t ew = c_edge[t % 10]; t /= 10;
    const int32_t nv = c_edge[t % 10]; t /= 10;
    const int32_t nw = c_edge[t % 10]; t /= 10;
    const int32_t mw = c_mw[t % 6];
    const uint32_t e = pack_entry(ev, ew), f = pack_entry(nv, nw);
    const uint32_t got = integrate_entry(e, f, mw), want = integrate_ref(e, f, mw);
    if (got != want) fail(rep, e, f, mw, 0, got, want);
    ++c;
  }
  count(rep, c);
}
__global__ void k_integrate_random(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const uint64_t h = mix64(i), g = mix64(i ^ 0x5851F42D4C957F2Dull);
    uint32_t e = (uint32_t)h, f = (uint32_t)(h >> 32);
    // three cases in four: both weights positive (the division), drawn over all of [1, 32767] or small
    const uint32_t mode = (uint32_t)(g & 3);
    if (mode)
    {
      uint32_t ew = (e >> 16) & 0x7fffu, nw = (f >> 16) & 0x7fffu;
      if (mode == 2) ew &= 0xffu;
      if (mode == 3) nw &= 0x3fu;
      e = (e & 0xffffu) | ((ew ? ew : 1u) << 16);
      f = (f & 0xffffu) | ((nw ? nw : 1u) << 16);
    }
    const int32_t mw = c_mw[(g >> 8) % 6];
    const uint32_t got = integrate_entry(e, f, mw), want = integrate_ref(e, f, mw);
    if (got != want) fail(rep, e, f, mw, 0, got, want);
    ++c;
  }
  count(rep, c);
}

// ---- l2norm: sqrt_trunc_i for every int32 sum (the wrapped negative ones give 0), l2norm_i / l2norm_l on random components
__global__ void k_sqrt_all(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const int32_t sq = (int32_t)(uint32_t)i;
    const int32_t want = sq < 0 ? 0 : (int32_t)(float)sqrt((double)(float)sq);
    const int32_t got = sqrt_trunc_i(sq);
    if (got != want) fail(rep, sq, 0, 0, 0, got, want);
    ++c;
  }
  count(rep, c);
}
__global__ void k_l2norm_random(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const uint64_t h = mix64(i), g = mix64(h);
    // components up to 2^17 (sums that stay below 2^31 and ones that wrap), or full int32
    const int sh = (g & 1) ? 15 : 0;
    const int32_t x = (int32_t)(uint32_t)h >> sh, y = (int32_t)(uint32_t)(h >> 32) >> sh, z = (int32_t)(uint32_t)g >> sh;
    const int32_t sq = (int32_t)(uint32_t)((uint64_t)((int64_t)x * x + (int64_t)y * y + (int64_t)z * z));
    const int32_t want = sq < 0 ? 0 : (int32_t)(float)sqrt((double)(float)sq);
    const int32_t got = l2norm_i(x, y, z);
    if (got != want) fail(rep, x, y, z, 0, got, want);
    // 64-bit: components below 2^31.5 (no wrap) or anything (wrapped sums: INT64_MIN, oracle/ws_oracle.c:l2norm_l)
    const int sl = (g & 2) ? 33 : 1;
    const int64_t X = (int64_t)h >> sl, Y = (int64_t)g >> sl, Z = (int64_t)mix64(g) >> sl;
    const uint64_t sqw = (uint64_t)X * (uint64_t)X + (uint64_t)Y * (uint64_t)Y + (uint64_t)Z * (uint64_t)Z;
    const int64_t wantl = (int64_t)sqw < 0 ? INT64_MIN : (int64_t)(float)sqrt((double)(float)(int64_t)sqw);
    const int64_t gotl = l2norm_l(X, Y, Z);
    if (gotl != wantl) fail(rep, X, Y, Z, 1, gotl, wantl);
    c += 2;
  }
  count(rep, c);
}

// ---- div_trunc_i64 (the ray set-up's 64-bit divisions) on random operands of every magnitude
__global__ void k_div_i64(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const uint64_t h = mix64(i), g = mix64(h);
    const int64_t num = (int64_t)h >> (g & 63);
    int64_t den = (int64_t)mix64(g) >> ((g >> 6) & 63);
    if (den == 0 || (num == INT64_MIN && den == -1)) den = 1; // (the one quotient int64 does not hold)
    const int64_t got = div_trunc_i64(num, den), want = num / den;
    if (got != want) fail(rep, num, den, 0, 0, got, want);
    ++c;
  }
  count(rep, c);
}

// ---- div_trunc_i64 on the operands its argument is about: the double division below 2^53 can only go wrong where num / den is
// within a rounding error of an integer, i.e. num = q den + e with e in {-1, 0, 1} and |num| as large as the branch admits; the
// switch to the plain division is at 2^53.  Two families, both signs of each operand:
//   near: for every den of the list, num = +-(2^53 + delta), delta in [-4, 4].  The list: every power of two and every divisor of
//         2^53 - 1 and 2^53 + 1 up to 2^53 - 1 (1 and 2^53 - 1 among them), so every num is q den + e with |e| <= 5, within 4 of 2^53.
//   mult: for EDGE_DENS divisors of every magnitude in [1, 2^53 - 1] and A in {2^53, 2^52, 2^40}: the multiple of den next below A
//         and the one at or next above it, each with e in {-1, 0, 1}.  |num| is within den of A: at A = 2^53 the lower multiple takes
//         the double division, the upper one the plain division (or the double one, where q den - 1 = 2^53 - 1).
constexpr uint64_t EDGE_DENS = 1ull << 20, EDGE_PER_DEN = 3 * 2 * 3 * 4, EDGE_PER_NEAR = 9 * 4;
__host__ __device__ inline int64_t edge_den(uint64_t j)
{
  const int64_t top = (1ll << 53) - 1;
  const int64_t special[8] = {1, 2, 3, top, top - 1, 1ll << 26, (1ll << 26) + 1, 94906266 /* ceil(sqrt(2^53)) */};
  if (j < 8) return special[j];
  const uint64_t h = mix64(j), g = mix64(h);
  const int64_t d = (int64_t)(h >> (11 + g % 53)); // every magnitude up to 2^53 - 1
  return d ? d : 1;
}
__global__ void k_div_i64_edges(const int64_t *near_dens, uint64_t n_near, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    int64_t num, den;
    uint64_t t = i;
    if (i < n_near * EDGE_PER_NEAR)
    {
      const uint32_t sg = (uint32_t)(t % 4); t /= 4;
      const int64_t delta = (int64_t)(t % 9) - 4; t /= 9;
      den = near_dens[t];
      num = (1ll << 53) + delta;
      if (sg & 1) num = -num;
      if (sg & 2) den = -den;
    }
    else
    {
      t -= n_near * EDGE_PER_NEAR;
      const uint32_t sg = (uint32_t)(t % 4); t /= 4;
      const int64_t e = (int64_t)(t % 3) - 1; t /= 3;
      const uint32_t hi = (uint32_t)(t % 2); t /= 2;
      const uint32_t which = (uint32_t)(t % 3); t /= 3;
      den = edge_den(t);
      const int64_t A = which == 0 ? (1ll << 53) : (which == 1 ? (1ll << 52) : (1ll << 40));
      const int64_t q = (A - 1) / den + (int64_t)hi; // q den < A <= (q + 1) den
      num = q * den + e;                             // below 2^54
      if (sg & 1) num = -num;
      if (sg & 2) den = -den;
    }
    const int64_t got = div_trunc_i64(num, den), want = num / den;
    if (got != want) fail(rep, num, den, 0, 0, got, want);
    ++c;
  }
  count(rep, c);
}

// ---------------------------------------------------------------------------------------------------------------------------
int main()
{
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  const dim3 G(GRID), B(BLOCK);

  begin();
  chunked((1ull << 31) - 1, [&](uint64_t b, uint64_t n) { k_fastdiv<<<G, B>>>(b, n, g_rep); });
  finish("make_fastdiv_dev", (1ull << 31) - 1);

  {
    std::vector<int32_t> divs = {1, 2, 3, 5, 6, 7, 9, 10, 25, 50, 641, 1000, 65535, 65536, 65537, 1 << 30, INT32_MAX, INT32_MAX - 1};
    for (int k = 2; k <= 30 && divs.size() < 48; k += 2)
    {
      divs.push_back((1 << k) - 1);
      divs.push_back((1 << k) + 1);
    }
    uint64_t s = 12345;
    while (divs.size() < 64)
    {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      divs.push_back(1 + (int32_t)((s >> 33) % INT32_MAX));
    }
    int32_t *d_divs;
    CHECK_HIP(hipMalloc((void **)&d_divs, divs.size() * sizeof(int32_t)));
    CHECK_HIP(hipMemcpy(d_divs, divs.data(), divs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    begin();
    chunked((uint64_t)divs.size() << 32, [&](uint64_t b, uint64_t n) { k_div_trunc<<<G, B>>>(d_divs, b, n, g_rep); });
    finish("div_trunc", (uint64_t)divs.size() << 32);
    CHECK_HIP(hipFree(d_divs));
  }

  {
    // every res in [2, 256] and the larger ones of the suite and the tools
    std::vector<int32_t> rs;
    for (int32_t r = 2; r <= 256; ++r) rs.push_back(r);
    for (int32_t r : {333, 500, 512, 1000, 1024, 2000, 4096, 10000, 65535}) rs.push_back(r);
    std::vector<MarchFrame> fr;
    const int32_t zero[3] = {0, 0, 0};
    const MapParams mp = {{3, 3, 3}, {0, 0, 0}, {0, 0, 0}};
    for (int32_t r : rs) fr.push_back(make_march_frame(zero, r, r, mp));
    MarchFrame *d_fr;
    CHECK_HIP(hipMalloc((void **)&d_fr, fr.size() * sizeof(MarchFrame)));
    CHECK_HIP(hipMemcpy(d_fr, fr.data(), fr.size() * sizeof(MarchFrame), hipMemcpyHostToDevice));
    begin();
    chunked((uint64_t)fr.size() << 32, [&](uint64_t b, uint64_t n) { k_div_res_all<<<G, B>>>(d_fr, b, n, g_rep); });
    finish("div_res (all x)", (uint64_t)fr.size() << 32);
    CHECK_HIP(hipFree(d_fr));
    begin();
    chunked((uint64_t)(65535 - 257 + 1) * DIVRES_PER, [&](uint64_t b, uint64_t n) { k_div_res_sampled<<<G, B>>>(257, b, n, g_rep); });
    finish("div_res (sampled)", (uint64_t)(65535 - 257 + 1) * DIVRES_PER); // (no x of the list leaves int32 for these res)
  }

  {
    // windows of one axis: odd and even sizes, offsets across the ring, positions on both sides of the origin, and the largest
    // reach make_march_frame still takes the biased route for (|pos| + size / 2 + 4 < 2^22 and times res < 2^30)
    struct W
    {
      int32_t res, size, pos, off;
      bool at_limit; // one more voxel of reach and the frame leaves the biased route
    };
    std::vector<W> ws = {{2, 65, 0, 32},     {3, 101, -7, 0},      {7, 51, 13, 50},   {25, 75, -200, 17},  {51, 333, 1000, 332},
                         {75, 64, -33, 63},  {333, 25, 5, 3},      {50, 128, 0, 0},   {20, 400, 37, 11},   {256, 480, -1367, 401},
                         {1000, 20, -3, 19}, {65, 1001, -500, 999}, {4, 4096, 70000, 2048}};
    for (W &w : ws) w.at_limit = false;
    const int32_t lim = (1 << 22) - 1;
    const int32_t lim1000 = (int32_t)(((1ll << 30) - 1) / 1000); // the largest reach with reach * 1000 < 2^30
    ws.push_back({2, 1001, lim - 500 - 4, 7, true});      // reach 2^22 - 1
    ws.push_back({2, 1001, -(lim - 500 - 4), 993, true}); // ... on the negative side
    ws.push_back({255, 2001, lim - 1000 - 4, 1, true});   // reach 2^22 - 1, and reach * res just below 2^30
    ws.push_back({1000, 501, lim1000 - 250 - 4, 100, true});    // reach * res just below 2^30
    ws.push_back({1000, 501, -(lim1000 - 250 - 4), 400, true}); // ... on the negative side
    std::vector<MarchFrame> fr;
    std::vector<int64_t> first;
    int64_t total = 0;
    unsigned long long ring_cases = 0;
    for (const W &w : ws)
    {
      const int32_t spos[3] = {w.pos, 0, 0};
      const MapParams mp = {{w.size, 3, 3}, {w.pos, 0, 0}, {w.off, 0, 0}};
      const MarchFrame f = make_march_frame(spos, w.res, w.res, mp);
      if (!f.biased_ok)
      {
        printf("ring: frame res %d size %d pos %d is not biased_ok\n", w.res, w.size, w.pos);
        g_bad = 1;
        continue;
      }
      // one more voxel of reach and the frame leaves the biased route
      const MapParams mp2 = {{w.size, 3, 3}, {w.pos + (w.pos < 0 ? -1 : 1), 0, 0}, {w.off, 0, 0}};
      if (w.at_limit && make_march_frame(spos, w.res, w.res, mp2).biased_ok)
      {
        printf("ring: frame res %d size %d pos %d is still biased_ok one voxel further out\n", w.res, w.size, w.pos);
        g_bad = 1;
      }
      fr.push_back(f);
      first.push_back(total);
      total += ((int64_t)w.size / 2 * 2 + 1) * w.res + 2 * (w.res - 1);
      // the millimetres whose voxel trunc(y / res) is in the window: res per voxel, 2 res - 1 for the voxel 0; three checks each
      const int64_t vlo = (int64_t)w.pos - w.size / 2, vhi = (int64_t)w.pos + w.size / 2;
      ring_cases += 3 * ((vhi - vlo + 1) * w.res + (vlo <= 0 && vhi >= 0 ? w.res - 1 : 0));
    }
    MarchFrame *d_fr;
    int64_t *d_first;
    CHECK_HIP(hipMalloc((void **)&d_fr, fr.size() * sizeof(MarchFrame)));
    CHECK_HIP(hipMalloc((void **)&d_first, first.size() * sizeof(int64_t)));
    CHECK_HIP(hipMemcpy(d_fr, fr.data(), fr.size() * sizeof(MarchFrame), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_first, first.data(), first.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    begin();
    k_ring<<<G, B>>>(d_fr, (int)fr.size(), 0, (uint64_t)total, d_first, g_rep);
    finish("div_res_b/ring_b/ring_m", ring_cases);
    CHECK_HIP(hipFree(d_fr));
    CHECK_HIP(hipFree(d_first));
  }

  begin();
  k_trunc15<<<G, B>>>(0, 65536ull * 65537ull, g_rep);
  finish("trunc15_biased", 65536ull * 65537ull);

  begin();
  chunked(32767ull * 65535ull, [&](uint64_t b, uint64_t n) { k_weight<<<G, B>>>(b, n, g_rep); });
  finish("tsdf_weight", 32767ull * 32768ull + 32767ull); // sum over tau of 2 tau + 1

  begin();
  k_integrate_edges<<<G, B>>>(0, 60000, g_rep);
  finish("integrate_entry (edges)", 60000);
  begin();
  chunked(1ull << 32, [&](uint64_t b, uint64_t n) { k_integrate_random<<<G, B>>>(b, n, g_rep); });
  finish("integrate_entry (rand)", 1ull << 32);

  begin();
  chunked(1ull << 32, [&](uint64_t b, uint64_t n) { k_sqrt_all<<<G, B>>>(b, n, g_rep); });
  finish("sqrt_trunc_i (all)", 1ull << 32);
  begin();
  k_l2norm_random<<<G, B>>>(0, 1ull << 28, g_rep);
  finish("l2norm_i / l2norm_l", 1ull << 29);

  begin();
  k_div_i64<<<G, B>>>(0, 1ull << 28, g_rep);
  finish("div_trunc_i64", 1ull << 28);

  {
    // the divisors of the `near` family; each is checked to divide the number it is listed for
    std::vector<int64_t> nd;
    for (int j = 0; j <= 52; ++j) nd.push_back(1ll << j);
    const int64_t top = (1ll << 53) - 1;
    const int64_t pm[3] = {6361, 69431, 20394401};       // 2^53 - 1
    const int64_t pp[3] = {3, 107, 28059810762433ll};    // 2^53 + 1
    for (int m = 1; m < 8; ++m)
    {
      int64_t a = 1, b = 1;
      for (int k = 0; k < 3; ++k)
        if (m & (1 << k)) a *= pm[k], b *= pp[k];
      if (top % a != 0 || (top + 2) % b != 0)
      {
        printf("div_trunc_i64 (edges): %lld or %lld is no divisor\n", (long long)a, (long long)b);
        g_bad = 1;
      }
      nd.push_back(a);
      if (b <= top) nd.push_back(b);
    }
    int64_t *d_nd;
    CHECK_HIP(hipMalloc((void **)&d_nd, nd.size() * sizeof(int64_t)));
    CHECK_HIP(hipMemcpy(d_nd, nd.data(), nd.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    const uint64_t n_edges = nd.size() * EDGE_PER_NEAR + EDGE_DENS * EDGE_PER_DEN; // 66 * 36 + 2^20 * 72 = 75 499 848 >= 2^26
    begin();
    k_div_i64_edges<<<G, B>>>(d_nd, nd.size(), 0, n_edges, g_rep);
    finish("div_trunc_i64 (edges)", n_edges);
    CHECK_HIP(hipFree(d_nd));
  }

  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
