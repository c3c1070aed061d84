// ground_units.hip — the rules of ws_map_ground / ws_store_ground (ws_ground.h), evaluated ON THE DEVICE and held to a plain
// restatement that runs on the host of this program, bit by bit and never through the helpers under test:
//   ground_levels / ground_pick   for every H in 1 .. 64 and every level bit 0 .. 63: the full headroom (a level), and the headroom with
//                                 ONE voxel z + k missing, k = 1 .. H -- the deciding bit at every position of the current word and of
//                                 the carried word; and for the remaining indices random words, free-only and with unknown headroom
//   ground_frac                   over the edges of the value domain
//   ground_in_box, ground_step, ground_dist_class, ground_no_level   over small grids
// Prints one line per subject, exits 1 on any mismatch.
#include <cstdint>
#include <vector>

#include "ws_ground.h"

#include "unit_report.hpp"

using namespace ws;

constexpr uint64_t N_H = 64, N_L = 64, N_K = 65, CASES = N_H * N_L * N_K;
struct UnitCase
{
  int32_t H;
  uint64_t occ, fre, acc, fre_above, acc_above;
  bool planted;
};
__host__ __device__ inline UnitCase unit_case(uint64_t i)
{
  UnitCase c;
  c.H = (int32_t)(i / (N_L * N_K)) + 1;
  const int32_t L = (int32_t)((i / N_K) % N_L), k = (int32_t)(i % N_K);
  c.planted = k <= c.H;
  if (c.planted)
  {
    // voxels L + 1 .. L + H free, but for voxel L + k where k >= 1; bit 64 and above lie in the carried word
    uint64_t lo = 0, hi = 0;
    for (int32_t j = 1; j <= c.H; ++j)
    {
      if (j == k) continue;
      const int32_t b = L + j;
      if (b < 64) lo |= 1ull << b; else hi |= 1ull << (b - 64);
    }
    c.occ = 1ull << L;
    c.fre = c.acc = lo;
    c.fre_above = c.acc_above = hi;
    return c;
  }
  c.occ = mix64(i) & mix64(i ^ 0xabcdefull);
  c.fre = ~c.occ & (mix64(3 * i + 1) | mix64(5 * i + 2));
  c.fre_above = mix64(7 * i + 3) | mix64(11 * i + 4);
  const uint64_t box = (i & 2u) ? ~0ull : ~0ull >> (mix64(i + 17) & 31u); // the box ends inside the word
  c.occ &= box, c.fre &= box;
  c.acc = (i & 1u) ? c.fre : box & ~c.occ;
  c.acc_above = (i & 1u) ? c.fre_above : c.fre_above | mix64(i + 99);
  return c;
}

__global__ void k_levels(uint64_t *out, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long cnt = 0;
  FOR_RANGE(i, base, n)
  {
    const UnitCase c = unit_case(i);
    const uint64_t lv = ground_levels(c.occ, c.fre, c.acc, c.fre_above, c.acc_above, c.H);
    out[2 * i] = lv;
    out[2 * i + 1] = lv ? (uint64_t)ground_pick(lv, false) | ((uint64_t)ground_pick(lv, true) << 8) : 0xffffull;
    ++cnt;
  }
  count(rep, cnt);
}

// the sentences of the header: z is a level iff it is OCCUPIED, z + 1 is FREE and z + 1 .. z + H are acceptable
static void levels_plain(const UnitCase &c, uint64_t want[2])
{
  auto bit = [](uint64_t lo, uint64_t hi, int32_t b) { return b < 64 ? (lo >> b) & 1u : b < 128 ? (hi >> (b - 64)) & 1u : 0u; };
  uint64_t lv = 0;
  int32_t lowest = -1, highest = -1;
  for (int32_t z = 0; z < 64; ++z)
  {
    bool ok = ((c.occ >> z) & 1u) && bit(c.fre, c.fre_above, z + 1);
    for (int32_t k = 1; k <= c.H && ok; ++k) ok = bit(c.acc, c.acc_above, z + k) != 0;
    if (!ok) continue;
    lv |= 1ull << z;
    if (lowest < 0) lowest = z;
    highest = z;
  }
  want[0] = lv;
  want[1] = lv ? (uint64_t)lowest | ((uint64_t)highest << 8) : 0xffffull;
}

// ---- the small grids: {frac, in_box, step, dist class, no level}
constexpr int32_t V0[] = {-1, -2, -255, -256, -257, -16384, -32767, -32768}, V1[] = {0, 1, 2, 255, 256, 16384, 32766, 32767};
constexpr int64_t ZS[] = {-2147483648ll, -65, -64, -63, -1, 0, 1, 62, 63, 64, 127, 128, 2147483584ll, 2147483647ll};
constexpr uint32_t N_V = 8, N_Z = 14, N_FRAC = N_V * N_V, N_BOX = N_Z * N_Z * N_Z, N_STEP = N_Z * N_Z, N_CLS = 4 * 5 * 5, N_SMALL = N_FRAC + N_BOX + N_STEP + N_CLS + 4;
__device__ __constant__ int32_t d_v0[N_V], d_v1[N_V];
__device__ __constant__ int64_t d_zs[N_Z];
constexpr uint32_t STEPS[] = {0, 1, 256, 65534, 65535};

__host__ __device__ inline uint32_t cls_word(uint32_t j, uint32_t &max_step, const uint32_t *steps)
{
  const uint32_t cls = j / 25, s = (j / 5) % 5;
  max_step = steps[j % 5];
  return 0x37u | (steps[s] << 8) | (cls << 30);
}

__global__ void k_small(uint64_t *out, Report *rep)
{
  const uint32_t steps[] = {0, 1, 256, 65534, 65535};
  unsigned long long cnt = 0;
  FOR_RANGE(i, 0, N_SMALL)
  {
    uint32_t j = (uint32_t)i;
    if (j < N_FRAC)
      out[i] = ground_frac(d_v0[j / N_V], d_v1[j % N_V]);
    else if ((j -= N_FRAC) < N_BOX)
      out[i] = ground_in_box(d_zs[j / (N_Z * N_Z)] & ~63ll, d_zs[(j / N_Z) % N_Z], d_zs[j % N_Z]);
    else if ((j -= N_BOX) < N_STEP)
      out[i] = ground_step(d_zs[j / N_Z] * 256 + 255, d_zs[j % N_Z] * 256);
    else if ((j -= N_STEP) < N_CLS)
    {
      uint32_t max_step;
      const uint32_t w = cls_word(j, max_step, steps);
      out[i] = ground_dist_class(w, max_step) | (ground_class(w) << 4) | ((uint64_t)ground_step_of(w) << 8) | ((uint64_t)ground_height(-5, w) << 32);
    }
    else
      out[i] = ground_no_level(((j - N_CLS) & 1u) != 0, ((j - N_CLS) & 2u) != 0);
    ++cnt;
  }
  count(rep, cnt);
}

static uint64_t small_plain(uint32_t j)
{
  if (j < N_FRAC)
  {
    const int64_t v0 = V0[j / N_V], v1 = V1[j % N_V], f = (256 * -v0) / (v1 - v0);
    return (uint64_t)(f > 255 ? 255 : f);
  }
  if ((j -= N_FRAC) < N_BOX)
  {
    const int64_t base = ZS[j / (N_Z * N_Z)] & ~63ll, lo = ZS[(j / N_Z) % N_Z], hi = ZS[j % N_Z];
    uint64_t m = 0;
    for (int b = 0; b < 64; ++b)
      if (base + b >= lo && base + b <= hi) m |= 1ull << b;
    return m;
  }
  if ((j -= N_BOX) < N_STEP)
  {
    const int64_t a = ZS[j / N_Z] * 256 + 255, b = ZS[j % N_Z] * 256, d = a > b ? a - b : b - a;
    return (uint64_t)(d > 65535 ? 65535 : d);
  }
  if ((j -= N_STEP) < N_CLS)
  {
    uint32_t max_step;
    const uint32_t w = cls_word(j, max_step, STEPS), cls = j / 25, step = STEPS[(j / 5) % 5];
    const uint32_t d = cls == 0 ? 0u : (cls == 1 && step <= max_step) ? 1u : 2u;
    (void)w;
    return d | (cls << 4) | ((uint64_t)step << 8) | ((uint64_t)(int64_t)(-5 * 256 + 0x37) << 32);
  }
  j -= N_CLS;
  return (j & 1u) ? 2u : (j & 2u) ? 3u : 0u;
}

int main()
{
  const dim3 G(GRID), B(BLOCK);
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  Report r;
  uint64_t *d_out;
  std::vector<uint64_t> got(2 * CASES);
  CHECK_HIP(hipMalloc((void **)&d_out, 2 * CASES * sizeof(uint64_t)));
  CHECK_HIP(hipMemset(d_out, 0x55, 2 * CASES * sizeof(uint64_t)));
  begin();
  k_levels<<<G, B>>>(d_out, 0, CASES, g_rep);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(got.data(), d_out, 2 * CASES * sizeof(uint64_t), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
  unsigned long long planted = 0, planted_levels = 0, random_levels = 0;
  for (uint64_t i = 0; i < CASES; ++i)
  {
    const UnitCase c = unit_case(i);
    uint64_t want[2];
    levels_plain(c, want);
    if (c.planted)
    {
      // the answer of a planted case is known without any loop: a level at L iff no voxel of the headroom is missing
      const uint64_t L = (i / N_K) % N_L, k = i % N_K;
      const uint64_t known = k == 0 ? 1ull << L : 0ull;
      if (want[0] != known) host_fail(r, (long long)i, c.H, (long long)L, (long long)k, (long long)want[0], (long long)known);
      ++planted, planted_levels += want[0] != 0;
    }
    else
      random_levels += want[0] != 0;
    for (int k = 0; k < 2; ++k)
      if (got[2 * i + k] != want[k]) host_fail(r, (long long)i, c.H, (long long)c.occ, k, (long long)got[2 * i + k], (long long)want[k]);
  }
  finish_host("ground_levels", r, CASES);
  printf("ground_levels cases  planted: %llu  planted levels: %llu  random with a level: %llu\n", planted, planted_levels, random_levels);

  CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_v0), V0, sizeof V0));
  CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_v1), V1, sizeof V1));
  CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_zs), ZS, sizeof ZS));
  begin();
  k_small<<<G, B>>>(d_out, g_rep);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(got.data(), d_out, N_SMALL * sizeof(uint64_t), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
  for (uint32_t j = 0; j < N_SMALL; ++j)
    if (got[j] != small_plain(j)) host_fail(r, j, 0, 0, 0, (long long)got[j], (long long)small_plain(j));
  finish_host("ground_small", r, N_SMALL);
  CHECK_HIP(hipFree(d_out));
  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
