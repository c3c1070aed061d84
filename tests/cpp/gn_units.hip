// gn_units.hip — the Gauss-Newton update of reg_gn.h and the sums of reg_reduce.h below it, evaluated ON THE DEVICE on inputs that no
// scan chose.  The update: sequences of synthetic sums from a case file (tests/gn_cases.py writes it: start states, slot totals, the
// 44 words, the state the CPU oracle leaves after every update); one 64-lane workgroup runs one sequence, one launch per form of the
// update, and after every update the state is compared with the oracle's as bit patterns -- in every lane, the state is uniform:
//   gn_update_terms   from the 29 terms in LDS (reg_batch_kernel, reg_iter_kernel)
//   gn_update         from the 44 words through lambdas (reg_solve_kernel, reg_pass_kernel)
//   gn_update_total   set up as reg_loop_kernel does it: the slot totals in lanes 0 .. 31, the pose element in lanes 0 .. 15, the state
//                     pinned to vector registers, T_sh / TI_sh in LDS; also T_sh, TI_sh against make_int_transform of the expected pose,
//                     and load_int_pose
// The sums: wave_reduce32, wave_reduce32_add, block_reduce32 for 8 waves and block_reduce32<WAVES> for 1, 2, 4, sum_partials<false> and
// <true> on per-lane int64 values of the full range (sums wrap) against plain uint64 sums computed on the host -- random values, low
// words of all ones (every carry crosses the halves), all ones, and a single non-zero thread (workgroup, for the partials) at every
// position; expand_sums against the words of the case file.
// Prints one line per form or helper, exits 1 on any mismatch.  usage: gn_units CASEFILE
#include <cstdint>
#include <cstring>
#include <vector>

#include "reg_gn.h"

#include "unit_report.hpp"

using namespace ws;

constexpr int MAXU = 8, START_W = 20, EXPECT_W = 24; // the case file's layout (gn_cases.write_case_file)
constexpr int32_t MAGIC = 0x474E3031;
// fields of a mismatch record: 0 .. 15 T, 16 alpha, 17 .. 20 prev, 21 iterations, 22 finished, then what gn_update_total leaves beside them
constexpr int F_ALPHA = 16, F_PREV = 17, F_ITERATIONS = 21, F_FINISHED = 22, F_TEL = 100, F_TI = 200, F_LOAD = 300;

struct Cases
{
  const uint32_t *start;   // [n][START_W]: T[16], max_iterations, it_weight_gradient, epsilon, updates
  const int32_t *center;   // [n][3]: (int) translation of the start pose, converted on the host as gn_init does
  const int64_t *slots;    // [n][MAXU][REG_SLOTS]
  const int64_t *words;    // [n][MAXU][44]
  const uint32_t *expect;  // [n][MAXU][EXPECT_W]
  uint32_t n;
};

__device__ __forceinline__ GnCore start_core(const Cases &cs, uint32_t seq)
{
  const uint32_t *s = cs.start + (size_t)seq * START_W;
  GnCore c;
#pragma unroll
  for (int i = 0; i < 16; ++i) c.T[i] = __uint_as_float(s[i]);
#pragma unroll
  for (int k = 0; k < 3; ++k) c.center[k] = cs.center[(size_t)seq * 3 + k];
  c.alpha = 0.f;
  c.prev[0] = c.prev[1] = c.prev[2] = c.prev[3] = 0.f;
  c.it_weight_gradient = __uint_as_float(s[17]);
  c.epsilon = __uint_as_float(s[18]);
  c.max_iterations = (int32_t)s[16];
  c.iterations = 0;
  c.finished = 0;
  c.error = 0;
  return c;
}

__device__ __forceinline__ void check_word(Report *rep, uint32_t seq, int u, int field, int form, uint32_t got, uint32_t want)
{
  if (got != want) fail(rep, seq, u, field, form, got, want);
}
// alpha, prev, iterations, finished of this lane's copy of the state
__device__ __forceinline__ void check_scalars(Report *rep, uint32_t seq, int u, int form, const GnCore &st, const uint32_t *want)
{
  check_word(rep, seq, u, F_ALPHA, form, __float_as_uint(st.alpha), want[F_ALPHA]);
#pragma unroll
  for (int i = 0; i < 4; ++i) check_word(rep, seq, u, F_PREV + i, form, __float_as_uint(st.prev[i]), want[F_PREV + i]);
  check_word(rep, seq, u, F_ITERATIONS, form, (uint32_t)st.iterations, want[F_ITERATIONS]);
  check_word(rep, seq, u, F_FINISHED, form, (uint32_t)st.finished, want[F_FINISHED]);
}
__device__ __forceinline__ void check_core(Report *rep, uint32_t seq, int u, int form, const GnCore &st, const uint32_t *want)
{
#pragma unroll
  for (int i = 0; i < 16; ++i) check_word(rep, seq, u, i, form, __float_as_uint(st.T[i]), want[i]);
  check_scalars(rep, seq, u, form, st, want);
}

// ---- form 0: gn_update_terms, the 29 terms in LDS
__global__ __launch_bounds__(64) void k_update_terms(Cases cs, Report *rep)
{
  __shared__ int64_t terms[REG_SLOTS];
  const uint32_t seq = blockIdx.x;
  GnCore st = start_core(cs, seq);
  const int n = (int)cs.start[(size_t)seq * START_W + 19];
  for (int u = 0; u < n; ++u)
  {
    __syncthreads();
    if (threadIdx.x < REG_SLOTS) terms[threadIdx.x] = cs.slots[((size_t)seq * MAXU + u) * REG_SLOTS + threadIdx.x];
    __syncthreads();
    gn_update_terms(st, terms);
    check_core(rep, seq, u, 0, st, cs.expect + ((size_t)seq * MAXU + u) * EXPECT_W);
  }
  if (threadIdx.x == 0) count(rep, (unsigned long long)n);
}

// ---- form 1: gn_update, the 44 words through lambdas as reg_solve_kernel passes them
__global__ __launch_bounds__(64) void k_update_words(Cases cs, Report *rep)
{
  __shared__ int64_t s[44];
  const uint32_t seq = blockIdx.x;
  GnCore st = start_core(cs, seq);
  const int n = (int)cs.start[(size_t)seq * START_W + 19];
  for (int u = 0; u < n; ++u)
  {
    __syncthreads();
    if (threadIdx.x < 44) s[threadIdx.x] = cs.words[((size_t)seq * MAXU + u) * 44 + threadIdx.x];
    __syncthreads();
    gn_update(
        st, [](int r, int c) { return s[c * 6 + r]; }, [](int r) { return s[36 + r]; }, (int32_t)s[42], (int32_t)s[43]);
    check_core(rep, seq, u, 1, st, cs.expect + ((size_t)seq * MAXU + u) * EXPECT_W);
  }
  if (threadIdx.x == 0) count(rep, (unsigned long long)n);
}

// ---- form 2: gn_update_total, the resident loop's
__global__ __launch_bounds__(64) void k_update_total(Cases cs, Report *rep)
{
  __shared__ alignas(16) float T_sh[16];
  __shared__ alignas(16) int32_t TI_sh[16];
  const uint32_t seq = blockIdx.x;
  const int lane = (int)threadIdx.x;
  GnCore st = start_core(cs, seq);
  pin_vgpr(st.center[0]); pin_vgpr(st.center[1]); pin_vgpr(st.center[2]);
  pin_vgpr(st.alpha); pin_vgpr(st.it_weight_gradient); pin_vgpr(st.epsilon);
  pin_vgpr(st.prev[0]); pin_vgpr(st.prev[1]); pin_vgpr(st.prev[2]); pin_vgpr(st.prev[3]);
  pin_vgpr(st.max_iterations); pin_vgpr(st.iterations); pin_vgpr(st.finished); pin_vgpr(st.error);
  float Tel = 0.f; // lanes 0 .. 15: the pose element (lane & 3, lane >> 2)
#pragma unroll
  for (int i = 0; i < 16; ++i) Tel = lane == i ? st.T[i] : Tel;
  if (lane < 16)
  {
    T_sh[lane] = Tel;
    if (lane == 15) TI_sh[15] = 0; // (read by load_int_pose, used by nobody)
    store_int_pose(TI_sh, lane, Tel);
  }
  const int n = (int)cs.start[(size_t)seq * START_W + 19];
  for (int u = 0; u < n; ++u)
  {
    // lanes 0 .. 28 hold the slot totals; what the other lanes hold is nobody's business
    const int64_t total = lane < REG_TERMS ? cs.slots[((size_t)seq * MAXU + u) * REG_SLOTS + lane] : (int64_t)mix64(((uint64_t)seq << 16) | (uint64_t)(u * 64 + lane));
    __syncthreads();
    gn_update_total(st, total, Tel, T_sh, TI_sh);
    __syncthreads();
    const uint32_t *want = cs.expect + ((size_t)seq * MAXU + u) * EXPECT_W;
    check_scalars(rep, seq, u, 2, st, want);
    float wantT[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
      wantT[i] = __uint_as_float(want[i]);
      check_word(rep, seq, u, i, 2, __float_as_uint(T_sh[i]), want[i]);
      if (lane == i) check_word(rep, seq, u, F_TEL + i, 2, __float_as_uint(Tel), want[i]);
    }
    const IntTransform wi = make_int_transform(wantT), li = load_int_pose(TI_sh);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i)
      {
        check_word(rep, seq, u, F_TI + 4 * j + i, 2, (uint32_t)TI_sh[4 * j + i], (uint32_t)wi.M[3 * j + i]);
        check_word(rep, seq, u, F_LOAD + 3 * j + i, 2, (uint32_t)li.M[3 * j + i], (uint32_t)wi.M[3 * j + i]);
      }
    check_word(rep, seq, u, F_TI + 3, 2, (uint32_t)TI_sh[3], (uint32_t)wi.cx);
    check_word(rep, seq, u, F_TI + 7, 2, (uint32_t)TI_sh[7], (uint32_t)wi.cy);
    check_word(rep, seq, u, F_TI + 11, 2, (uint32_t)TI_sh[11], (uint32_t)wi.cz);
    check_word(rep, seq, u, F_LOAD + 12, 2, (uint32_t)li.cx, (uint32_t)wi.cx);
    check_word(rep, seq, u, F_LOAD + 13, 2, (uint32_t)li.cy, (uint32_t)wi.cy);
    check_word(rep, seq, u, F_LOAD + 14, 2, (uint32_t)li.cz, (uint32_t)wi.cz);
  }
  if (threadIdx.x == 0) count(rep, (unsigned long long)n);
}

// ---- expand_sums: 29 terms -> the 44 words of the case file
__global__ void k_expand(Cases cs, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, 0, (uint64_t)cs.n * MAXU)
  {
    const uint32_t seq = (uint32_t)(i / MAXU), u = (uint32_t)(i % MAXU);
    if (u >= cs.start[(size_t)seq * START_W + 19]) continue;
    int64_t sums[44];
    expand_sums(cs.slots + i * REG_SLOTS, sums);
    for (int k = 0; k < 44; ++k)
      if (sums[k] != cs.words[i * 44 + k]) fail(rep, seq, u, k, 0, sums[k], cs.words[i * 44 + k]);
    c += 44;
  }
  count(rep, c);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The reductions.  Pattern p of a helper run by `units` threads (workgroups, for the partials) -- host and device code:
//   p < N_RANDOM         every value random over all of int64
//   N_RANDOM             random high words over low words of all ones
//   N_RANDOM + 1         every value -1
//   N_RANDOM + 2 + t     a single non-zero unit, t
constexpr uint32_t N_RANDOM = 48;
__host__ __device__ inline uint32_t n_patterns(uint32_t units) { return N_RANDOM + 2 + units; }
__host__ __device__ inline int64_t red_value(uint32_t fn, uint32_t p, uint32_t unit, uint32_t slot)
{
  const uint64_t h = mix64(((uint64_t)fn << 56) ^ ((uint64_t)p << 36) ^ ((uint64_t)unit << 8) ^ slot);
  if (p < N_RANDOM) return (int64_t)h;
  if (p == N_RANDOM) return (int64_t)(h | 0xffffffffull);
  if (p == N_RANDOM + 1) return -1;
  return unit == p - (N_RANDOM + 2) ? (int64_t)(h | 1ull) : 0;
}

enum { M_WAVE = 0, M_WAVE_ADD = 1, M_BLOCK8 = 2, M_BLOCK = 3 };
// one workgroup of WAVES waves per pattern.  out: M_WAVE [pattern][wave][slot], otherwise [pattern][slot]
template <int WAVES, int MODE>
__global__ __launch_bounds__(WAVES * 64) void k_reduce(uint32_t fn, int64_t *out)
{
  __shared__ int64_t wave_part[WAVES][REG_SLOTS];
  __shared__ int64_t red[REG_SLOTS];
  __shared__ unsigned long long wg_sum[REG_SLOTS];
  const uint32_t p = blockIdx.x;
  int64_t v[REG_SLOTS];
#pragma unroll
  for (int s = 0; s < REG_SLOTS; ++s) v[s] = red_value(fn, p, threadIdx.x, (uint32_t)s);
  if constexpr (MODE == M_WAVE)
  {
    wave_reduce32(v, wave_part);
    for (uint32_t i = threadIdx.x; i < WAVES * REG_SLOTS; i += WAVES * 64) out[(size_t)p * WAVES * REG_SLOTS + i] = wave_part[i / REG_SLOTS][i % REG_SLOTS];
  }
  else if constexpr (MODE == M_WAVE_ADD)
  {
    if (threadIdx.x < REG_SLOTS) wg_sum[threadIdx.x] = 0;
    __syncthreads();
    wave_reduce32_add(v, wg_sum);
    __syncthreads();
    if (threadIdx.x < REG_SLOTS) out[(size_t)p * REG_SLOTS + threadIdx.x] = (int64_t)wg_sum[threadIdx.x];
  }
  else
  {
    if constexpr (MODE == M_BLOCK8)
    {
      static_assert(MODE != M_BLOCK8 || WAVES == REG_THREADS / 64, "block_reduce32 sums REG_THREADS / 64 waves");
      block_reduce32(v, wave_part, red);
    }
    else
      block_reduce32<WAVES>(v, wave_part, red);
    if (threadIdx.x < REG_SLOTS) out[(size_t)p * REG_SLOTS + threadIdx.x] = red[threadIdx.x];
  }
}

// sum_partials: one workgroup of REG_THREADS threads per pattern, its partials [REG_BLOCKS][REG_SLOTS] filled by the host
template <bool COHERENT>
__global__ __launch_bounds__(REG_THREADS) void k_partials(const int64_t *pp, int64_t *out)
{
  __shared__ int64_t wave_part[REG_THREADS / 64][REG_SLOTS];
  __shared__ int64_t red[REG_SLOTS];
  sum_partials<COHERENT>(pp + (size_t)blockIdx.x * REG_BLOCKS * REG_SLOTS, wave_part, red);
  if (threadIdx.x < REG_SLOTS) out[(size_t)blockIdx.x * REG_SLOTS + threadIdx.x] = red[threadIdx.x];
}

// the host's sums: plain uint64 additions, unit after unit
static void reduce_line(const char *name, uint32_t fn, int waves, int mode, int64_t *d_out, std::vector<int64_t> &out)
{
  const uint32_t units = (uint32_t)waves * 64, np = n_patterns(units), groups = mode == M_WAVE ? (uint32_t)waves : 1u;
  const size_t n_out = (size_t)np * groups * REG_SLOTS;
  out.resize(n_out);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipMemcpy(out.data(), d_out, n_out * sizeof(int64_t), hipMemcpyDeviceToHost));
  Report r = {};
  for (uint32_t p = 0; p < np; ++p)
    for (uint32_t g = 0; g < groups; ++g)
      for (uint32_t s = 0; s < REG_SLOTS; ++s)
      {
        uint64_t want = 0;
        const uint32_t t0 = mode == M_WAVE ? g * 64 : 0, t1 = mode == M_WAVE ? g * 64 + 64 : units;
        for (uint32_t t = t0; t < t1; ++t) want += (uint64_t)red_value(fn, p, t, s);
        const uint64_t got = (uint64_t)out[((size_t)p * groups + g) * REG_SLOTS + s];
        if (got != want) host_fail(r, p, g, s, mode, (long long)got, (long long)want);
        ++r.checked;
      }
  finish_host(name, r, n_out);
}

template <class T>
static T *upload(const void *src, size_t bytes)
{
  T *d;
  CHECK_HIP(hipMalloc((void **)&d, bytes ? bytes : 1));
  CHECK_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
  return d;
}

int main(int argc, char **argv)
{
  if (argc < 2)
  {
    printf("usage: gn_units CASEFILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int32_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!f || fread(head, sizeof(int32_t), 8, f) != 8 || head[0] != MAGIC || head[1] < 1 || head[3] != MAXU)
  {
    printf("%s: not a case file\n", argv[1]);
    return 2;
  }
  const size_t n = (size_t)head[1];
  const unsigned long long updates = (unsigned long long)head[2];
  std::vector<uint32_t> start(n * START_W), expect(n * MAXU * EXPECT_W);
  std::vector<int64_t> slots(n * MAXU * REG_SLOTS), words(n * MAXU * 44);
  if (fread(start.data(), 4, start.size(), f) != start.size() || fread(slots.data(), 8, slots.size(), f) != slots.size() ||
      fread(words.data(), 8, words.size(), f) != words.size() || fread(expect.data(), 4, expect.size(), f) != expect.size())
  {
    printf("%s: short case file\n", argv[1]);
    return 2;
  }
  fclose(f);
  std::vector<int32_t> center(n * 3);
  unsigned long long listed = 0;
  for (size_t i = 0; i < n; ++i)
  {
    for (int k = 0; k < 3; ++k)
    {
      float t;
      std::memcpy(&t, &start[i * START_W + 12 + k], 4);
      center[i * 3 + k] = (int32_t)t; // gn_init: Point center = total_transform.block<3,1>(0,3).cast<int>()
    }
    if (start[i * START_W + 19] < 1 || start[i * START_W + 19] > (uint32_t)MAXU)
    {
      printf("%s: sequence %zu has %u updates\n", argv[1], i, start[i * START_W + 19]);
      return 2;
    }
    listed += start[i * START_W + 19];
  }
  if (listed != updates)
  {
    printf("%s: %llu updates listed, %llu in the header\n", argv[1], listed, updates);
    return 2;
  }

  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  Cases cs;
  cs.start = upload<uint32_t>(start.data(), start.size() * 4);
  cs.center = upload<int32_t>(center.data(), center.size() * 4);
  cs.slots = upload<int64_t>(slots.data(), slots.size() * 8);
  cs.words = upload<int64_t>(words.data(), words.size() * 8);
  cs.expect = upload<uint32_t>(expect.data(), expect.size() * 4);
  cs.n = (uint32_t)n;

  begin();
  k_update_terms<<<dim3((unsigned)n), dim3(64)>>>(cs, g_rep);
  finish("gn_update_terms", updates);
  begin();
  k_update_words<<<dim3((unsigned)n), dim3(64)>>>(cs, g_rep);
  finish("gn_update", updates);
  begin();
  k_update_total<<<dim3((unsigned)n), dim3(64)>>>(cs, g_rep);
  finish("gn_update_total", updates);
  begin();
  k_expand<<<dim3(GRID), dim3(BLOCK)>>>(cs, g_rep);
  finish("expand_sums", 44 * updates);

  {
    constexpr int W8 = REG_THREADS / 64;
    int64_t *d_out;
    CHECK_HIP(hipMalloc((void **)&d_out, (size_t)n_patterns(W8 * 64) * W8 * REG_SLOTS * sizeof(int64_t)));
    std::vector<int64_t> out;
    k_reduce<W8, M_WAVE><<<dim3(n_patterns(W8 * 64)), dim3(W8 * 64)>>>(1, d_out);
    reduce_line("wave_reduce32", 1, W8, M_WAVE, d_out, out);
    k_reduce<W8, M_WAVE_ADD><<<dim3(n_patterns(W8 * 64)), dim3(W8 * 64)>>>(2, d_out);
    reduce_line("wave_reduce32_add", 2, W8, M_WAVE_ADD, d_out, out);
    k_reduce<W8, M_BLOCK8><<<dim3(n_patterns(W8 * 64)), dim3(W8 * 64)>>>(3, d_out);
    reduce_line("block_reduce32", 3, W8, M_BLOCK8, d_out, out);
    k_reduce<1, M_BLOCK><<<dim3(n_patterns(64)), dim3(64)>>>(4, d_out);
    reduce_line("block_reduce32<1>", 4, 1, M_BLOCK, d_out, out);
    k_reduce<2, M_BLOCK><<<dim3(n_patterns(128)), dim3(128)>>>(5, d_out);
    reduce_line("block_reduce32<2>", 5, 2, M_BLOCK, d_out, out);
    k_reduce<4, M_BLOCK><<<dim3(n_patterns(256)), dim3(256)>>>(6, d_out);
    reduce_line("block_reduce32<4>", 6, 4, M_BLOCK, d_out, out);

    // the partials of REG_BLOCKS workgroups per pattern
    const uint32_t np = n_patterns(REG_BLOCKS);
    std::vector<int64_t> pp((size_t)np * REG_BLOCKS * REG_SLOTS);
    std::vector<uint64_t> want((size_t)np * REG_SLOTS, 0);
    for (uint32_t p = 0; p < np; ++p)
      for (uint32_t b = 0; b < (uint32_t)REG_BLOCKS; ++b)
        for (uint32_t s = 0; s < REG_SLOTS; ++s)
        {
          const int64_t v = red_value(7, p, b, s);
          pp[((size_t)p * REG_BLOCKS + b) * REG_SLOTS + s] = v;
          want[(size_t)p * REG_SLOTS + s] += (uint64_t)v;
        }
    int64_t *d_pp = upload<int64_t>(pp.data(), pp.size() * 8);
    for (int coherent = 0; coherent < 2; ++coherent)
    {
      CHECK_HIP(hipMemset(d_out, 0xff, (size_t)np * REG_SLOTS * sizeof(int64_t)));
      if (coherent)
        k_partials<true><<<dim3(np), dim3(REG_THREADS)>>>(d_pp, d_out);
      else
        k_partials<false><<<dim3(np), dim3(REG_THREADS)>>>(d_pp, d_out);
      CHECK_HIP(hipGetLastError());
      out.resize((size_t)np * REG_SLOTS);
      CHECK_HIP(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
      Report r = {};
      for (size_t i = 0; i < out.size(); ++i)
      {
        if ((uint64_t)out[i] != want[i]) host_fail(r, (long long)(i / REG_SLOTS), (long long)(i % REG_SLOTS), coherent, 0, out[i], (long long)want[i]);
        ++r.checked;
      }
      finish_host(coherent ? "sum_partials<true>" : "sum_partials<false>", r, out.size());
    }
    CHECK_HIP(hipFree(d_pp));
    CHECK_HIP(hipFree(d_out));
  }

  CHECK_HIP(hipFree((void *)cs.start));
  CHECK_HIP(hipFree((void *)cs.center));
  CHECK_HIP(hipFree((void *)cs.slots));
  CHECK_HIP(hipFree((void *)cs.words));
  CHECK_HIP(hipFree((void *)cs.expect));
  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
