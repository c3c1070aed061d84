// clearance_units.hip — the rules of ws_map_clearance / ws_store_clearance (ws_clearance.h), evaluated ON THE DEVICE and held to a plain
// restatement that runs on the host of this program and never goes through the helpers under test:
//   clear_margin                  every d2 in 0 .. 65025 at res 1, 20, 64, 1000 and 1024, with radius 0 and 65535: the floor square root by
//                                 integer bisection on the host, a float estimate with integer correction on the device
//   clear_centre / clear_voxel    the rotated offset at the ends of its domain: rot_q30 entries, offsets and positions drawn from the ends
//                                 (+-2^30, +-2^20, +-(2^30 - 1)), from the values around +-2^29 where the rounding turns, and at random; the
//                                 host restates the sum, the rounding and the two floor divisions in 128-bit integers
//   clear_penalty, clear_key      over margins and soft ranges at the ends of theirs
// Prints one line per subject, exits 1 on any mismatch.
#include <cstdint>
#include <vector>

#include "ws_clearance.h"

#include "unit_report.hpp"

using namespace ws;

constexpr uint32_t N_RES = 5, N_D2 = 65026, N_RAD = 2;
constexpr uint64_t N_MARGIN = (uint64_t)N_RES * N_D2 * N_RAD, N_CENTRE = 1u << 19, N_SMALL = 64 * 64;
__host__ __device__ inline int32_t unit_res(uint64_t j)
{
  const int32_t r[N_RES] = {1, 20, 64, 1000, 1024};
  return r[j % N_RES];
}

struct CentreCase
{
  int32_t pose[12], off[3], res;
};
__host__ __device__ inline int32_t pick(const int32_t *ends, uint32_t n, uint64_t h, int32_t lo, int32_t hi)
{
  // three of four values come from the ends, the fourth is anywhere in [lo, hi]
  if ((h & 3u) != 3u) return ends[(h >> 2) % n];
  return (int32_t)((int64_t)lo + (int64_t)((h >> 2) % (uint64_t)((int64_t)hi - lo + 1)));
}
__host__ __device__ inline CentreCase centre_case(uint64_t i)
{
  const int32_t Q = 1 << 30, H = 1 << 29, O = 1 << 20;
  const int32_t rot[] = {-Q, -Q + 1, -H - 1, -H, -H + 1, -1, 0, 1, H - 1, H, H + 1, Q - 1, Q};
  const int32_t off[] = {-O, -O + 1, -2, -1, 0, 1, 2, O - 1, O};
  const int32_t pos[] = {-(Q - 1), -(Q - 2), -1025, -1024, -1, 0, 1, 1023, 1024, Q - 2, Q - 1};
  CentreCase c;
  for (int j = 0; j < 9; ++j) c.pose[j] = pick(rot, 13, mix64(16 * i + j), -Q, Q);
  for (int j = 0; j < 3; ++j) c.pose[9 + j] = pick(pos, 11, mix64(16 * i + 9 + j), -(Q - 1), Q - 1);
  for (int j = 0; j < 3; ++j) c.off[j] = pick(off, 9, mix64(16 * i + 12 + j), -O, O);
  c.res = unit_res(mix64(16 * i + 15));
  return c;
}

__global__ void k_margin(int32_t *out, uint64_t n, Report *rep)
{
  unsigned long long cnt = 0;
  FOR_RANGE(i, 0, n)
  {
    const uint32_t d2 = (uint32_t)(i % N_D2);
    const uint64_t j = i / N_D2;
    out[i] = clear_margin(d2, unit_res(j / N_RAD), (j % N_RAD) ? 65535 : 0);
    ++cnt;
  }
  count(rep, cnt);
}

__global__ void k_centre(int64_t *out, uint64_t n, Report *rep)
{
  unsigned long long cnt = 0;
  FOR_RANGE(i, 0, n)
  {
    const CentreCase c = centre_case(i);
    for (int a = 0; a < 3; ++a)
    {
      const int64_t centre = clear_centre(c.pose, c.off, a);
      out[6 * i + a] = centre;
      out[6 * i + 3 + a] = clear_voxel(centre, c.res);
    }
    ++cnt;
  }
  count(rep, cnt);
}

// margins -65535 .. 2^18 and soft 0 .. 65535 from 64 values each, ends included
__host__ __device__ inline int32_t small_margin(uint32_t j) { return j == 0 ? -65535 : j == 63 ? (1 << 18) : j == 1 ? -1 : j == 2 ? 0 : (int32_t)(mix64(j) % 327680u) - 65535; }
__host__ __device__ inline int32_t small_soft(uint32_t j) { return j == 0 ? 0 : j == 63 ? 65535 : (int32_t)(mix64(1000 + j) % 65536u); }
__global__ void k_small(uint64_t *out, Report *rep)
{
  unsigned long long cnt = 0;
  FOR_RANGE(i, 0, N_SMALL)
  {
    const int32_t m = small_margin((uint32_t)(i / 64)), s = small_soft((uint32_t)(i % 64));
    out[2 * i] = clear_penalty(m, s);
    out[2 * i + 1] = clear_key(m, (uint32_t)(i * 1021u));
    ++cnt;
  }
  count(rep, cnt);
}

// ---- the plain restatement, host only
static int64_t plain_isqrt(unsigned __int128 x)
{
  int64_t lo = 0, hi = (int64_t)1 << 20; // lo^2 <= x < hi^2
  while (hi - lo > 1)
  {
    const int64_t mid = (lo + hi) / 2;
    if ((unsigned __int128)mid * (unsigned __int128)mid <= x) lo = mid; else hi = mid;
  }
  return lo;
}
static __int128 plain_floor_div(__int128 a, __int128 b)
{
  __int128 q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
  return q;
}

int main()
{
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  Report r;
  const dim3 G(GRID), B(BLOCK);

  int32_t *d_m = nullptr;
  CHECK_HIP(hipMalloc((void **)&d_m, N_MARGIN * sizeof(int32_t)));
  begin();
  k_margin<<<G, B>>>(d_m, N_MARGIN, g_rep);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  std::vector<int32_t> got_m(N_MARGIN);
  CHECK_HIP(hipMemcpy(got_m.data(), d_m, N_MARGIN * sizeof(int32_t), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
  unsigned long long squares = 0;
  for (uint64_t i = 0; i < N_MARGIN; ++i)
  {
    const uint64_t d2 = i % N_D2, j = i / N_D2;
    const int64_t res = unit_res(j / N_RAD), rad = (j % N_RAD) ? 65535 : 0;
    const int64_t root = plain_isqrt((unsigned __int128)d2 * (unsigned __int128)(res * res));
    squares += (uint64_t)(root * root) == d2 * (uint64_t)(res * res);
    if (got_m[i] != root - rad) host_fail(r, (long long)d2, res, rad, 0, got_m[i], root - rad);
    if (clear_margin((uint32_t)d2, (int32_t)res, (int32_t)rad) != root - rad) host_fail(r, (long long)d2, res, rad, 1, clear_margin((uint32_t)d2, (int32_t)res, (int32_t)rad), root - rad);
  }
  finish_host("clear_margin", r, N_MARGIN);
  printf("clear_margin cases  perfect squares: %llu\n", squares);
  CHECK_HIP(hipFree(d_m));

  int64_t *d_c = nullptr;
  CHECK_HIP(hipMalloc((void **)&d_c, N_CENTRE * 6 * sizeof(int64_t)));
  begin();
  k_centre<<<G, B>>>(d_c, N_CENTRE, g_rep);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  std::vector<int64_t> got_c(N_CENTRE * 6);
  CHECK_HIP(hipMemcpy(got_c.data(), d_c, N_CENTRE * 6 * sizeof(int64_t), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
  unsigned long long halves = 0, negative = 0, widest = 0;
  for (uint64_t i = 0; i < N_CENTRE; ++i)
  {
    const CentreCase c = centre_case(i);
    for (int a = 0; a < 3; ++a)
    {
      __int128 s = 0;
      for (int j = 0; j < 3; ++j) s += (__int128)c.pose[3 * a + j] * (__int128)c.off[j];
      const __int128 half = (__int128)1 << 29, one = (__int128)1 << 30;
      halves += plain_floor_div(s + half, one) * one == s + half; // the sum lies exactly half a millimetre below a whole one
      const __int128 centre = (__int128)c.pose[9 + a] + plain_floor_div(s + half, one), voxel = plain_floor_div(centre, (__int128)c.res);
      negative += centre < 0;
      const unsigned long long mag = (unsigned long long)(s < 0 ? -s : s);
      widest = mag > widest ? mag : widest;
      if ((__int128)got_c[6 * i + a] != centre) host_fail(r, (long long)i, a, c.res, 0, got_c[6 * i + a], (long long)centre);
      if ((__int128)got_c[6 * i + 3 + a] != voxel) host_fail(r, (long long)i, a, c.res, 1, got_c[6 * i + 3 + a], (long long)voxel);
      if ((__int128)clear_voxel(clear_centre(c.pose, c.off, a), c.res) != voxel) host_fail(r, (long long)i, a, c.res, 2, clear_voxel(clear_centre(c.pose, c.off, a), c.res), (long long)voxel);
    }
  }
  finish_host("clear_centre", r, N_CENTRE);
  printf("clear_centre cases  exact halves: %llu  negative centres: %llu  widest sum: %llu\n", halves, negative, widest);
  CHECK_HIP(hipFree(d_c));

  uint64_t *d_s = nullptr;
  CHECK_HIP(hipMalloc((void **)&d_s, N_SMALL * 2 * sizeof(uint64_t)));
  begin();
  k_small<<<G, B>>>(d_s, g_rep);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  std::vector<uint64_t> got_s(N_SMALL * 2);
  CHECK_HIP(hipMemcpy(got_s.data(), d_s, N_SMALL * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < N_SMALL; ++i)
  {
    const int64_t m = small_margin((uint32_t)(i / 64)), s = small_soft((uint32_t)(i % 64));
    const uint64_t pen = s > m ? (uint64_t)((s - m) * (s - m)) : 0ull;
    const uint64_t key = ((uint64_t)(m + ((int64_t)1 << 31)) << 32) | (uint32_t)(i * 1021u); // the margin biased to unsigned, above the index
    if (got_s[2 * i] != pen) host_fail(r, (long long)m, (long long)s, 0, 0, (long long)got_s[2 * i], (long long)pen);
    if (got_s[2 * i + 1] != key || clear_key_margin(got_s[2 * i + 1]) != m) host_fail(r, (long long)m, (long long)s, 1, 0, (long long)got_s[2 * i + 1], (long long)key);
  }
  finish_host("clear_small", r, N_SMALL);
  CHECK_HIP(hipFree(d_s));
  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
