// coarsen_units.hip — the rule of ws_store_coarsen (ws_coarsen.h), evaluated ON THE DEVICE and held to a plain restatement of the
// same operation that runs on the host of this program: coarsen_div over its whole domain, and coarsen_add / coarsen_entry on eight
// children for every assignment of the weights {-5, 0, 1, 32767} and every min_observed.  The restatement uses the built-in / and %
// with an explicit floor and plain loops; it never calls the helpers under test.  Every mismatch is counted; the first few are recorded
// with their inputs.  Prints one line per subject, exits 1 on any mismatch.
#include <cstdint>
#include <vector>

#include "ws_coarsen.h"

#include "unit_report.hpp"

using namespace ws;

// ---- coarsen_div(S, n): every S in -262144 .. 262136 (eight int16 values) for every n in 1 .. 8
constexpr int32_t S_LO = -262144, S_HI = 262136;
constexpr uint64_t DIV_PER_N = (uint64_t)(S_HI - S_LO) + 1, DIV_CASES = 8 * DIV_PER_N;
__global__ void k_div(int32_t *out, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    out[i] = coarsen_div(S_LO + (int32_t)(i % DIV_PER_N), 1 + (int32_t)(i / DIV_PER_N));
    ++c;
  }
  count(rep, c);
}
static int32_t floor_div_plain(int32_t S, int32_t n)
{
  int32_t q = S / n;
  if (S % n != 0 && S < 0) q -= 1;
  return q;
}

// ---- the entry: case i = ((set * 8 + (min_observed - 1)) * 65536 + w), the weights of the children are the eight base-4 digits of
// w in {-5, 0, 1, 32767}; the values come from the ends of int16, the neighbours of zero and a hash
constexpr uint32_t N_SETS = 16;
constexpr uint64_t ENTRY_CASES = (uint64_t)N_SETS * 8 * 65536;
constexpr uint32_t UNIT_FILL = 0x00000258u | (0xfff9u << 16); // value 600, weight -7
__host__ __device__ inline int32_t unit_weight(uint32_t w, int j)
{
  const uint32_t d = (w >> (2 * j)) & 3u;
  return d == 0 ? -5 : d == 1 ? 0 : d == 2 ? 1 : 32767;
}
__host__ __device__ inline int32_t unit_value(uint32_t set, uint32_t w, int j)
{
  const uint64_t h = mix64(((uint64_t)set << 32) | ((uint64_t)w << 3) | (uint64_t)j);
  if (set == 0) return -32768;
  if (set == 1) return 32767;
  if (set == 2) return j == 0 ? -1 : 0; // S = -1 whenever child 0 is observed
  const uint32_t kind = (uint32_t)(h >> 60);
  return kind == 0 ? -32768 : kind == 1 ? 32767 : kind == 2 ? -1 : kind == 3 ? 1 : (int32_t)(int16_t)(h & 0xffffu);
}
__host__ __device__ inline uint32_t unit_raw(int32_t value, int32_t weight) { return ((uint32_t)value & 0xffffu) | ((uint32_t)weight << 16); }
__global__ void k_entry(uint32_t *out, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const uint32_t w = (uint32_t)(i & 0xffffu), set = (uint32_t)(i >> 19);
    const int32_t min_observed = 1 + (int32_t)((i >> 16) & 7u);
    CoarsenAcc acc;
    for (int j = 0; j < 8; ++j) coarsen_add(acc, unit_raw(unit_value(set, w, j), unit_weight(w, j)));
    out[i] = coarsen_entry(acc, min_observed, UNIT_FILL);
    ++c;
  }
  count(rep, c);
}
static uint32_t entry_plain(uint32_t set, uint32_t w, int32_t min_observed)
{
  int32_t n = 0, S = 0, W = 0;
  for (int j = 0; j < 8; ++j)
  {
    const int32_t weight = unit_weight(w, j);
    if (weight <= 0) continue;
    W = n == 0 || weight < W ? weight : W;
    n += 1;
    S += unit_value(set, w, j);
  }
  if (n < min_observed) return UNIT_FILL;
  return unit_raw(floor_div_plain(S, n), W);
}

int main()
{
  const dim3 G(GRID), B(BLOCK);
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  Report r;

  {
    int32_t *d_out;
    std::vector<int32_t> got(DIV_CASES);
    CHECK_HIP(hipMalloc((void **)&d_out, DIV_CASES * sizeof(int32_t)));
    CHECK_HIP(hipMemset(d_out, 0x55, DIV_CASES * sizeof(int32_t)));
    begin();
    k_div<<<G, B>>>(d_out, 0, DIV_CASES, g_rep);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(got.data(), d_out, DIV_CASES * sizeof(int32_t), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < DIV_CASES; ++i)
    {
      const int32_t S = S_LO + (int32_t)(i % DIV_PER_N), n = 1 + (int32_t)(i / DIV_PER_N), want = floor_div_plain(S, n);
      if (got[i] != want) host_fail(r, S, n, 0, 0, got[i], want);
    }
    finish_host("coarsen_div", r, DIV_CASES);
    CHECK_HIP(hipFree(d_out));
  }

  {
    uint32_t *d_out;
    std::vector<uint32_t> got(ENTRY_CASES);
    unsigned long long n_fill = 0, n_value = 0;
    CHECK_HIP(hipMalloc((void **)&d_out, ENTRY_CASES * sizeof(uint32_t)));
    CHECK_HIP(hipMemset(d_out, 0x55, ENTRY_CASES * sizeof(uint32_t)));
    begin();
    k_entry<<<G, B>>>(d_out, 0, ENTRY_CASES, g_rep);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(got.data(), d_out, ENTRY_CASES * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < ENTRY_CASES; ++i)
    {
      const uint32_t w = (uint32_t)(i & 0xffffu), set = (uint32_t)(i >> 19);
      const int32_t min_observed = 1 + (int32_t)((i >> 16) & 7u);
      const uint32_t want = entry_plain(set, w, min_observed);
      (want == UNIT_FILL ? n_fill : n_value) += 1;
      if (got[i] != want) host_fail(r, set, w, min_observed, 0, got[i], want);
    }
    finish_host("coarsen_entry", r, ENTRY_CASES);
    printf("coarsen_entry kinds    fill: %llu  value: %llu\n", n_fill, n_value);
    if (n_fill < 100000 || n_value < 100000) g_bad = 1;
    CHECK_HIP(hipFree(d_out));
  }

  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
