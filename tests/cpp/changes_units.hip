// changes_units.hip — the rule of ws_store_changes (ws_changes.h), evaluated ON THE DEVICE and held to a plain restatement of the
// same rule that runs on the host of this program: changes_verdict and changes_word over the full grid of ev and nv in
// {-32768, -band, -band + 1, 0, band - 1, band, free - 1, free, 32767}, ew and nw in {-5, 0, min_weight - 1, min_weight, 32767},
// valid / not valid, for three parameter sets.  The restatement is written from the sentences of the header with plain comparisons;
// it never calls the helpers under test.  Every mismatch is counted; the first few are recorded with their inputs.  Prints one line
// per subject, exits 1 on any mismatch.
#include <cstdint>
#include <vector>

#include "ws_changes.h"

#include "unit_report.hpp"

using namespace ws;

constexpr uint32_t N_SETS = 3, N_V = 9, N_W = 5;
constexpr uint64_t PER_SET = (uint64_t)N_V * N_V * N_W * N_W * 2, CASES = N_SETS * PER_SET;
struct UnitSet
{
  int32_t band, free_value, min_weight;
};
__host__ __device__ inline UnitSet unit_set(uint32_t s)
{
  // the usual map (band = resolution, free = tau); band == free_value == 1 with min_weight 1; the upper ends
  return s == 0 ? UnitSet{64, 600, 1} : s == 1 ? UnitSet{1, 1, 1} : UnitSet{32767, 32767, 32767};
}
__host__ __device__ inline int32_t unit_value(const UnitSet &u, uint32_t i)
{
  const int32_t v[N_V] = {-32768, -u.band, -u.band + 1, 0, u.band - 1, u.band, u.free_value - 1, u.free_value, 32767};
  return v[i];
}
__host__ __device__ inline int32_t unit_weight(const UnitSet &u, uint32_t i)
{
  const int32_t w[N_W] = {-5, 0, u.min_weight - 1, u.min_weight, 32767};
  return w[i];
}
struct UnitCase
{
  UnitSet u;
  int32_t ev, ew, nv, nw;
  bool valid;
};
__host__ __device__ inline UnitCase unit_case(uint64_t i)
{
  UnitCase c;
  c.u = unit_set((uint32_t)(i / PER_SET));
  uint64_t r = i % PER_SET;
  c.valid = (r & 1u) != 0;
  r >>= 1;
  c.nw = unit_weight(c.u, (uint32_t)(r % N_W)), r /= N_W;
  c.ew = unit_weight(c.u, (uint32_t)(r % N_W)), r /= N_W;
  c.nv = unit_value(c.u, (uint32_t)(r % N_V)), r /= N_V;
  c.ev = unit_value(c.u, (uint32_t)r);
  return c;
}

// out[i]: the verdict in the low byte, the record's word's kind and value above it is checked apart: {verdict, diff, word}
__global__ void k_verdict(uint32_t *out, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long cnt = 0;
  FOR_RANGE(i, base, n)
  {
    const UnitCase c = unit_case(i);
    const ChangesRule r = {c.u.band, c.u.free_value, c.u.min_weight};
    uint32_t diff;
    const uint32_t v = changes_verdict(c.ev, c.ew, c.valid, c.nv, c.nw, r, diff);
    out[3 * i] = v, out[3 * i + 1] = diff, out[3 * i + 2] = changes_word(c.nv, v & 3u);
    ++cnt;
  }
  count(rep, cnt);
}

// the sentences of the header, one after the other
static void verdict_plain(const UnitCase &c, uint32_t want[3], int &cls)
{
  const bool cur_known = c.ew >= c.u.min_weight;
  const bool ref_known = c.valid && c.nw >= c.u.min_weight;
  auto occupied = [&](int32_t d) { return (d < 0 ? -(int64_t)d : (int64_t)d) < (int64_t)c.u.band; };
  auto is_free = [&](int32_t d) { return d >= c.u.free_value; };
  uint32_t kind = 0;
  if (cur_known && ref_known)
  {
    if (occupied(c.ev) && is_free(c.nv)) kind = 1;
    if (is_free(c.ev) && occupied(c.nv)) kind = 2;
  }
  want[0] = kind | (cur_known && ref_known ? 4u : 0u) | (cur_known && !ref_known ? 8u : 0u);
  want[1] = cur_known && ref_known ? (uint32_t)(c.nv > c.ev ? c.nv - c.ev : c.ev - c.nv) : 0u;
  want[2] = (uint32_t)(uint16_t)(int16_t)c.nv | (kind << 16);
  cls = !cur_known ? 0 : !ref_known ? 1 : kind == 0 ? 2 : kind == 1 ? 3 : 4;
}

int main()
{
  const dim3 G(GRID), B(BLOCK);
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  Report r;
  uint32_t *d_out;
  std::vector<uint32_t> got(3 * CASES);
  unsigned long long n_cls[5] = {0, 0, 0, 0, 0};
  CHECK_HIP(hipMalloc((void **)&d_out, 3 * CASES * sizeof(uint32_t)));
  CHECK_HIP(hipMemset(d_out, 0x55, 3 * CASES * sizeof(uint32_t)));
  begin();
  k_verdict<<<G, B>>>(d_out, 0, CASES, g_rep);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(got.data(), d_out, 3 * CASES * sizeof(uint32_t), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < CASES; ++i)
  {
    const UnitCase c = unit_case(i);
    uint32_t want[3];
    int cls;
    verdict_plain(c, want, cls);
    n_cls[cls] += 1;
    for (int k = 0; k < 3; ++k)
      if (got[3 * i + k] != want[k]) host_fail(r, (long long)i, c.ev, c.nv, k, got[3 * i + k], want[k]);
  }
  finish_host("changes_verdict", r, CASES);
  printf("changes_verdict kinds  unknown: %llu  new: %llu  same: %llu  appeared: %llu  vanished: %llu\n", n_cls[0], n_cls[1], n_cls[2], n_cls[3], n_cls[4]);
  CHECK_HIP(hipFree(d_out));
  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
