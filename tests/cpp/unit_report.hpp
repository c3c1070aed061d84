// unit_report.hpp — the scaffolding of the device unit programs (device_units.hip, query_units.hip, gn_units.hip): a report in device memory that
// counts cases and mismatches and keeps the inputs of the first few, the index loop of the check kernels, and the line printed per
// helper.  Included once per program, after the library's headers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK_HIP(x)                                                                                                                   \
  do                                                                                                                                   \
  {                                                                                                                                    \
    hipError_t e_ = (x);                                                                                                               \
    if (e_ != hipSuccess)                                                                                                              \
    {                                                                                                                                  \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__);                                                  \
      exit(2);                                                                                                                         \
    }                                                                                                                                  \
  } while (0)

constexpr int MAX_REC = 8;
struct Report
{
  unsigned long long mismatches;
  unsigned long long checked;
  uint32_t n_rec;
  uint32_t pad;
  long long rec[MAX_REC][6]; // inputs and the two results of the first mismatches
};

__device__ void fail(Report *r, long long a, long long b, long long c, long long d, long long got, long long want)
{
  atomicAdd(&r->mismatches, 1ull);
  const uint32_t i = atomicAdd(&r->n_rec, 1u);
  if (i < MAX_REC)
  {
    r->rec[i][0] = a;
    r->rec[i][1] = b;
    r->rec[i][2] = c;
    r->rec[i][3] = d;
    r->rec[i][4] = got;
    r->rec[i][5] = want;
  }
}
// one add per thread and launch: how many cases were looked at (a kernel that silently skipped its domain fails the count)
__device__ void count(Report *r, unsigned long long n)
{
  if (n) atomicAdd(&r->checked, n);
}

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z)
{
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr uint32_t GRID = 4096, BLOCK = 256;
#define FOR_RANGE(i, base, n)                                                                                                          \
  for (uint64_t i = (base) + (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < (base) + (n); i += (uint64_t)GRID * BLOCK)

static Report *g_rep;
static int g_bad = 0;

static void begin() { CHECK_HIP(hipMemset(g_rep, 0, sizeof(Report))); }
static void finish(const char *name, unsigned long long expect_checked)
{
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  Report r;
  CHECK_HIP(hipMemcpy(&r, g_rep, sizeof r, hipMemcpyDeviceToHost));
  printf("%-22s checked %14llu  mismatches %llu\n", name, r.checked, r.mismatches);
  for (uint32_t j = 0; j < r.n_rec && j < (uint32_t)MAX_REC; ++j)
    printf("    in (%lld, %lld, %lld, %lld): got %lld, want %lld\n", r.rec[j][0], r.rec[j][1], r.rec[j][2], r.rec[j][3], r.rec[j][4], r.rec[j][5]);
  if (r.mismatches || (expect_checked && r.checked != expect_checked) || r.checked == 0)
  {
    if (expect_checked && r.checked != expect_checked) printf("    expected %llu cases\n", expect_checked);
    g_bad = 1;
  }
  fflush(stdout);
}
// a long index space in launches of at most 2^34 cases (each launch well below a second)
template <class F>
static void chunked(uint64_t n, F &&launch)
{
  const uint64_t STEP = 1ull << 34;
  for (uint64_t b = 0; b < n; b += STEP) launch(b, n - b < STEP ? n - b : STEP);
}

// a line whose comparison ran on the host: the report goes through the same finish()
static void finish_host(const char *name, const Report &r, unsigned long long expect)
{
  CHECK_HIP(hipMemcpy(g_rep, &r, sizeof r, hipMemcpyHostToDevice));
  finish(name, expect);
}
static void host_fail(Report &r, long long a, long long b, long long c, long long d, long long got, long long want)
{
  ++r.mismatches;
  if (r.n_rec < (uint32_t)MAX_REC)
  {
    const long long v[6] = {a, b, c, d, got, want};
    for (int k = 0; k < 6; ++k) r.rec[r.n_rec][k] = v[k];
  }
  ++r.n_rec;
}
