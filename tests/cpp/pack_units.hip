// pack_units.hip — the two scans of ws_store_pack / ws_store_unpack (ws_pack.h), run ON THE DEVICE on their own and held to serial
// loops on the host of this program.  The kernels below call the very functions the library's kernels call (store_pack.hip) and
// add nothing but the copy of the result.
//   pack_brick_offsets: one 256-thread workgroup per class map, a grid that strides over the maps as the emit and unpack kernels
//     stride over their chunks; off[512] against the serial prefix sum of {0, 1, 512}[code].  The edge maps (all of one class; two
//     and three classes alternating; one dense brick, and one brick that is not dense, at the bricks where the two-codes-per-thread
//     layout changes its wave) and 4096 maps drawn from mix64.
//   pack_scan: synthetic headers (counts in words 3 and 4, the first-word fields poisoned, everything else drawn) for n around the
//     ends of a wave and of a round of 1024 chunks, and 20 000 chunks of 512 dense bricks, whose offsets pass 2^32 words.  The first
//     word of every header and the three sums against a 64-bit serial loop; every other header word must be as it was.
// Every mismatch is counted; the first few are recorded with their inputs.  Prints one line per subject, exits 1 on any mismatch.
#include <cstdint>
#include <vector>

#include "ws_pack.h"

#include "unit_report.hpp"

using namespace ws;

// ------------------------------------------------------------------------------------------------ pack_brick_offsets
constexpr uint32_t EDGE_BRICKS[6] = {0, 127, 128, 255, 256, 511}; // first and last brick of the four waves' 128
constexpr uint32_t N_RANDOM = 4096, OFFSET_GRID = 120;            // (the grid is no divisor of the number of maps)

static std::vector<std::vector<uint32_t>> offset_maps()
{
  std::vector<std::vector<uint32_t>> maps;
  const auto add = [&](auto &&code) {
    std::vector<uint32_t> m(PACK_BRICKS);
    for (uint32_t b = 0; b < PACK_BRICKS; ++b) m[b] = code(b);
    maps.push_back(m);
  };
  for (uint32_t c = 0; c < 3; ++c) add([&](uint32_t) { return c; });
  for (uint32_t c0 = 0; c0 < 3; ++c0) // period 2: every ordered pair of unlike classes
    for (uint32_t c1 = 0; c1 < 3; ++c1)
      if (c0 != c1) add([&](uint32_t b) { return b & 1u ? c1 : c0; });
  for (uint32_t p = 0; p < 3; ++p) add([&](uint32_t b) { return (b + p) % 3u; }); // period 3, every phase
  for (uint32_t e : EDGE_BRICKS) add([&](uint32_t b) { return b == e ? PACK_DENSE : PACK_DEFAULT; });
  for (uint32_t c = 0; c < 2; ++c) // everything dense but one brick, which is default or uniform
    for (uint32_t e : EDGE_BRICKS) add([&](uint32_t b) { return b == e ? c : PACK_DENSE; });
  const size_t n_edge = maps.size();
  for (uint32_t r = 0; r < N_RANDOM; ++r) add([&](uint32_t b) { return (uint32_t)(mix64(((uint64_t)r << 9) | b) % 3u); });
  printf("pack_brick_offsets maps  edge: %zu  random: %u\n", n_edge, N_RANDOM);
  return maps;
}

__global__ __launch_bounds__(PACK_OFFSETS_WG) void k_offsets(const uint32_t *headers, uint32_t n, uint32_t *out, Report *rep)
{
  __shared__ uint32_t map[32], off[PACK_BRICKS], part[4];
  for (uint32_t m = blockIdx.x; m < n; m += gridDim.x)
  {
    pack_brick_offsets(headers + (size_t)m * PACK_HDR, map, off, part);
    out[(size_t)m * PACK_BRICKS + threadIdx.x] = off[threadIdx.x];
    out[(size_t)m * PACK_BRICKS + PACK_OFFSETS_WG + threadIdx.x] = off[PACK_OFFSETS_WG + threadIdx.x];
    if (threadIdx.x == 0u) count(rep, PACK_BRICKS);
    __syncthreads();
  }
}

static void offsets_subject()
{
  const std::vector<std::vector<uint32_t>> maps = offset_maps();
  const uint32_t n = (uint32_t)maps.size();
  std::vector<uint32_t> headers((size_t)n * PACK_HDR, 0u), got((size_t)n * PACK_BRICKS);
  for (uint32_t m = 0; m < n; ++m)
    for (uint32_t b = 0; b < PACK_BRICKS; ++b) headers[(size_t)m * PACK_HDR + PACK_HDR_MAP + (b >> 4)] |= maps[m][b] << (2u * (b & 15u));
  uint32_t *d_headers, *d_out;
  CHECK_HIP(hipMalloc((void **)&d_headers, headers.size() * sizeof(uint32_t)));
  CHECK_HIP(hipMalloc((void **)&d_out, got.size() * sizeof(uint32_t)));
  CHECK_HIP(hipMemcpy(d_headers, headers.data(), headers.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemset(d_out, 0x55, got.size() * sizeof(uint32_t)));
  begin();
  k_offsets<<<dim3(OFFSET_GRID), dim3(PACK_OFFSETS_WG)>>>(d_headers, n, d_out, g_rep);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(got.data(), d_out, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  Report r;
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
  const uint32_t words[3] = {0u, 1u, 512u};
  for (uint32_t m = 0; m < n; ++m)
  {
    uint32_t at = 0;
    for (uint32_t b = 0; b < PACK_BRICKS; ++b)
    {
      if (got[(size_t)m * PACK_BRICKS + b] != at) host_fail(r, m, b, maps[m][b], b ? (long long)maps[m][b - 1] : -1ll, got[(size_t)m * PACK_BRICKS + b], at);
      at += words[maps[m][b]];
    }
  }
  finish_host("pack_brick_offsets", r, (unsigned long long)n * PACK_BRICKS);
  CHECK_HIP(hipFree(d_headers));
  CHECK_HIP(hipFree(d_out));
}

// ------------------------------------------------------------------------------------------------ pack_scan
constexpr uint32_t SCAN_N[11] = {1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 5780};
constexpr uint32_t SCAN_LONG = 20000, POISON = 0xDEADBEEFu;

__global__ __launch_bounds__(PACK_SCAN_WG) void k_scan(uint32_t *headers, uint32_t n, unsigned long long *sums, Report *rep)
{
  __shared__ unsigned long long wtot[PACK_SCAN_WG / 64], red[2][PACK_SCAN_WG / 64];
  pack_scan(headers, n, sums, wtot, red);
  if (threadIdx.x == 0u) count(rep, n);
}

// one run of n headers; dense_only: 512 dense bricks in every chunk.  Adds its mismatches to r.
static void scan_run(uint32_t n, bool dense_only, Report &r)
{
  std::vector<uint32_t> before((size_t)n * PACK_HDR), got((size_t)n * PACK_HDR);
  for (uint32_t i = 0; i < n; ++i)
  {
    uint32_t *h = &before[(size_t)i * PACK_HDR];
    for (uint32_t k = 0; k < PACK_HDR; ++k) h[k] = (uint32_t)mix64(((uint64_t)n << 40) | ((uint64_t)i << 8) | k);
    const uint32_t uniform = dense_only ? 0u : (uint32_t)(mix64(((uint64_t)n << 32) | i) % 513u);
    h[PACK_HDR_UNIFORM] = uniform;
    h[PACK_HDR_DENSE] = dense_only ? 512u : (uint32_t)(mix64(((uint64_t)n << 32) | (1ull << 31) | i) % (513u - uniform));
    h[PACK_HDR_OFF_LO] = h[PACK_HDR_OFF_HI] = POISON;
  }
  uint32_t *d_headers;
  unsigned long long *d_sums, sums[3];
  CHECK_HIP(hipMalloc((void **)&d_headers, before.size() * sizeof(uint32_t)));
  CHECK_HIP(hipMalloc((void **)&d_sums, sizeof sums));
  CHECK_HIP(hipMemcpy(d_headers, before.data(), before.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemset(d_sums, 0x55, sizeof sums));
  k_scan<<<dim3(1), dim3(PACK_SCAN_WG)>>>(d_headers, n, d_sums, g_rep);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(got.data(), d_headers, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost));
  uint64_t first = 0, n_uniform = 0, n_dense = 0;
  for (uint32_t i = 0; i < n; ++i)
  {
    const uint32_t *b = &before[(size_t)i * PACK_HDR], *g = &got[(size_t)i * PACK_HDR];
    const uint64_t have = (uint64_t)g[PACK_HDR_OFF_LO] | ((uint64_t)g[PACK_HDR_OFF_HI] << 32);
    if (have != first) host_fail(r, n, i, b[PACK_HDR_UNIFORM], b[PACK_HDR_DENSE], (long long)have, (long long)first);
    for (uint32_t k = 0; k < PACK_HDR; ++k)
      if (k != PACK_HDR_OFF_LO && k != PACK_HDR_OFF_HI && g[k] != b[k]) host_fail(r, n, i, k, -1, g[k], b[k]);
    first += (uint64_t)b[PACK_HDR_UNIFORM] + 512ull * b[PACK_HDR_DENSE];
    n_uniform += b[PACK_HDR_UNIFORM], n_dense += b[PACK_HDR_DENSE];
  }
  const uint64_t want[3] = {first, n_uniform, n_dense};
  for (int k = 0; k < 3; ++k)
    if (sums[k] != want[k]) host_fail(r, n, -1, k, -1, (long long)sums[k], (long long)want[k]);
  if (dense_only) // the numbers of the host's test of ws_pack_check: 5 242 880 000 words, the last chunk starts beyond 2^32
  {
    const uint32_t hi = got[(size_t)(n - 1) * PACK_HDR + PACK_HDR_OFF_HI];
    if (first <= (1ull << 32) || hi != 1u) host_fail(r, n, n - 1, -2, -2, hi, 1);
    printf("pack_scan long  chunks: %u  words: %llu  last hi: %u\n", n, sums[0], hi);
  }
  CHECK_HIP(hipFree(d_headers));
  CHECK_HIP(hipFree(d_sums));
}

static void scan_subject()
{
  begin();
  Report host = {};
  unsigned long long total = SCAN_LONG;
  for (uint32_t n : SCAN_N) scan_run(n, false, host), total += n;
  scan_run(SCAN_LONG, true, host);
  Report r;
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost)); // the count is the device's, the mismatches are the host's
  host.checked = r.checked;
  finish_host("pack_scan", host, total);
}

int main()
{
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  offsets_subject();
  scan_subject();
  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
