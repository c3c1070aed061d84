// points_units.hip — a lane's points of reg_points.h, evaluated ON THE DEVICE on inputs that no scan chose (tests/points_cases.py
// writes the case file; tests/test_points_cases_host.py holds it to its claims):
//   central_gradient      every pair of raw entries from a list of values x a list of weights, against registration.cu:233-246 restated
//   point_terms           Gathered values at the edges of q, v, the gradients, ok and the voxel's weight, against registration.cu:217-250
//                         restated on int64 with the reference's int32 wraps, in the same thread
//   sums int64            consume_point + wave_reduce32_add   } one workgroup of REG_THREADS threads per pattern, wg_sum and the staging
//   sums mfma             mfma_consume + mfma_flush +         } area set up as reg_loop_kernel sets them up, two passes per launch (the
//                         mfma_finalize                       } second on the next pattern's data), the 29 totals of every pass against
//                                                               plain uint64 sums of the restated terms computed on the host
//   mfma_finalize zeroes  the 32 + 8 words read by the first wave straight after mfma_finalize
//   gather_point, gather_point<true>, gather_point_loop + make_loop_gather
//                         windows A .. E of tests/reg_cases.py, one point per lane, a sequence of poses in one launch with the voxel
//                         caches kept: J, value and mask per point against the oracle's, and the cached forms field by field against
//                         the uncached gather of the same pose
// Prints one line per helper, exits 1 on any mismatch.  usage: points_units CASEFILE
#include <cstdint>
#include <cstring>
#include <vector>

#include "reg_points.h"

#include "unit_report.hpp"

using namespace ws;

constexpr int32_t MAGIC = 0x50543031;
constexpr int GW = 12; // words of a Gathered in the case file: qx qy qz cur xn xl yn yl zn zl ok pad
constexpr int WAVES = REG_THREADS / 64;

// ---- the restatement: plain int64, wrapped to int32 where the reference computes in int
struct RefTerms
{
  int64_t J[6], v, used;
};
__host__ __device__ inline int64_t ref_wrap32(int64_t x) { return (int64_t)(int32_t)(uint32_t)((uint64_t)x & 0xffffffffull); }
__host__ __device__ inline int64_t ref_value(uint32_t raw) { return (int64_t)(int16_t)(uint16_t)(raw & 0xffffu); }
__host__ __device__ inline int64_t ref_gradient(uint32_t next, uint32_t last)
{
  const int64_t nv = ref_value(next), lv = ref_value(last);
  if ((next >> 16) == 0u || (last >> 16) == 0u) return 0;
  if ((nv > 0 && lv < 0) || (nv < 0 && lv > 0)) return 0;
  return (nv - lv) / 2; // C division: toward zero
}
__host__ __device__ inline RefTerms ref_point_terms(const uint32_t *w)
{
  RefTerms r = {};
  if (w[10] == 0u || (w[3] >> 16) == 0u) return r;
  const int64_t q[3] = {ref_wrap32(w[0]), ref_wrap32(w[1]), ref_wrap32(w[2])};
  const int64_t g[3] = {ref_gradient(w[4], w[5]), ref_gradient(w[6], w[7]), ref_gradient(w[8], w[9])};
  r.J[0] = ref_wrap32(ref_wrap32(q[1] * g[2]) - ref_wrap32(q[2] * g[1]));
  r.J[1] = ref_wrap32(ref_wrap32(q[2] * g[0]) - ref_wrap32(q[0] * g[2]));
  r.J[2] = ref_wrap32(ref_wrap32(q[0] * g[1]) - ref_wrap32(q[1] * g[0]));
  r.J[3] = g[0];
  r.J[4] = g[1];
  r.J[5] = g[2];
  r.v = ref_value(w[3]);
  r.used = 1;
  return r;
}

__device__ __forceinline__ Gathered load_gathered(const uint32_t *w)
{
  Gathered g;
  g.qx = (int32_t)w[0]; g.qy = (int32_t)w[1]; g.qz = (int32_t)w[2];
  g.cur = w[3]; g.xn = w[4]; g.xl = w[5]; g.yn = w[6]; g.yl = w[7]; g.zn = w[8]; g.zl = w[9];
  g.ok = w[10] != 0u;
  return g;
}

// ---- central_gradient: case i = ((value a, weight a), (value b, weight b))
__global__ void k_gradient(const int32_t *vals, uint32_t nv, const int32_t *weights, uint32_t nw, Report *rep)
{
  unsigned long long c = 0;
  const uint64_t ne = (uint64_t)nv * nw;
  FOR_RANGE(i, 0, ne * ne)
  {
    const uint32_t a = (uint32_t)(i / ne), b = (uint32_t)(i % ne);
    const uint32_t next = pack_entry(vals[a / nw], weights[a % nw]), last = pack_entry(vals[b / nw], weights[b % nw]);
    const int64_t got = central_gradient(next, last), want = ref_gradient(next, last);
    if (got != want) fail(rep, vals[a / nw], weights[a % nw], vals[b / nw], weights[b % nw], got, want);
    ++c;
  }
  count(rep, c);
}

// ---- point_terms: field 0 .. 5 J, 6 v, 7 used
__device__ __forceinline__ void check_terms(Report *rep, long long a, long long b, long long form, const Gathered &g, const int64_t (&J)[6], int64_t v, int64_t used)
{
  int32_t gJ[6], gv, gu;
  point_terms(g, gJ, gv, gu);
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if ((int64_t)gJ[k] != J[k]) fail(rep, a, b, k, form, gJ[k], J[k]);
  if ((int64_t)gv != v) fail(rep, a, b, 6, form, gv, v);
  if ((int64_t)gu != used) fail(rep, a, b, 7, form, gu, used);
}
__global__ void k_point_terms(const uint32_t *cases, uint32_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, 0, (uint64_t)n)
  {
    const RefTerms r = ref_point_terms(cases + i * GW);
    check_terms(rep, (long long)i, 0, 0, load_gathered(cases + i * GW), r.J, r.v, r.used);
    ++c;
  }
  count(rep, c);
}

// ---- the sums: workgroup p runs pattern p and then, without touching wg_sum in between, the data of pattern (p + 1) % n; only
// its first waves[p] waves call the sums (reg_loop_kernel: wave_has_points)
template <bool MFMA>
__global__ __launch_bounds__(REG_THREADS) void k_sums(const uint32_t *pat, const int32_t *waves, uint32_t n_pat, unsigned long long *out /* [p][pass][32] */,
                                                      unsigned long long *left /* [p][pass][32 + MF_AUX] */)
{
  __shared__ unsigned long long wg_sum[REG_SLOTS + MF_AUX];
  __shared__ alignas(16) uint32_t mf_stage[WAVES * MF_STAGE_WORDS];
  const MfLane mfl = make_mf_lane();
  const uint32_t p = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const bool wave_has_points = (int32_t)wave < waves[p];
  if (threadIdx.x < REG_SLOTS + MF_AUX) wg_sum[threadIdx.x] = 0;
  for (uint32_t pass = 0; pass < 2; ++pass)
  {
    const Gathered g = load_gathered(pat + ((size_t)((p + pass) % n_pat) * REG_THREADS + threadIdx.x) * GW);
    __syncthreads();
    if (wave_has_points)
    {
      if (MFMA)
      {
        mf_v16i C;
#pragma unroll
        for (int i = 0; i < 16; ++i) C[i] = 0;
        mfma_consume(g, C, mf_stage + wave * MF_STAGE_WORDS, mfl);
        mfma_flush(C, wg_sum, mfl);
      }
      else
      {
        int64_t acc[REG_SLOTS];
#pragma unroll
        for (int t = 0; t < REG_SLOTS; ++t) acc[t] = 0;
        consume_point(g, acc);
        wave_reduce32_add(acc, wg_sum);
      }
    }
    __syncthreads();
    if (threadIdx.x < 64)
    {
      unsigned long long s;
      if (MFMA)
        s = mfma_finalize(wg_sum, mfl);
      else
      {
        s = wg_sum[lane & 31u];
        if (lane < REG_SLOTS) wg_sum[lane] = 0; // counted_publish<false>
      }
      if (lane < REG_SLOTS) out[((size_t)p * 2 + pass) * REG_SLOTS + lane] = s;
      __builtin_amdgcn_wave_barrier();
      if (lane < REG_SLOTS + MF_AUX) left[((size_t)p * 2 + pass) * (REG_SLOTS + MF_AUX) + lane] = wg_sum[lane];
    }
  }
}

// ---- the gathers.  FORM 0: gather_point, 1: gather_point<true>, 2: gather_point_loop; one point per lane, the poses of the
// sequence one after the other with the lane's voxel cache kept.  fields of a mismatch: 0 .. 7 J, v, used against the oracle,
// 10 .. 20 the Gathered against the uncached gather's
struct GatherCase
{
  PointArgs a;
  const int32_t *steps;  // [n_steps][16]: M[12], centre, pad
  const int32_t *expect; // [n_steps][n_points][8]
  uint32_t n_steps, n_points, window; // (a mismatch names its point as 1000 window + point)
};
template <int FORM>
__global__ __launch_bounds__(64) void k_gather(GatherCase cs, Report *rep)
{
  const uint32_t idx = blockIdx.x * 64 + threadIdx.x;
  const bool valid = idx < cs.n_points;
  const size_t o = valid ? 3 * (size_t)idx : 0;
  const int32_t px = cs.a.points[o], py = cs.a.points[o + 1], pz = cs.a.points[o + 2];
  const LoopGather lg = make_loop_gather(cs.a);
  VoxelCache vc;
  vc.bx = vc.by = vc.bz = 0;
  vc.cur = vc.xn = vc.xl = vc.yn = vc.yl = vc.zn = vc.zl = 0;
  vc.filled = false;
  unsigned long long c = 0;
  for (uint32_t s = 0; s < cs.n_steps; ++s)
  {
    IntTransform t;
#pragma unroll
    for (int k = 0; k < 12; ++k) t.M[k] = cs.steps[s * 16 + k];
    t.cx = cs.steps[s * 16 + 12];
    t.cy = cs.steps[s * 16 + 13];
    t.cz = cs.steps[s * 16 + 14];
    const Gathered plain = gather_point(cs.a, t, px, py, pz, valid);
    Gathered g = plain;
    if (FORM == 1) g = gather_point<true>(cs.a, t, px, py, pz, valid, &vc);
    if (FORM == 2) g = gather_point_loop(cs.a, lg, t, px, py, pz, valid, vc);
    if (!valid) continue;
    const int32_t *e = cs.expect + ((size_t)s * cs.n_points + idx) * 8;
    const int64_t J[6] = {e[0], e[1], e[2], e[3], e[4], e[5]};
    check_terms(rep, s, 1000 * cs.window + idx, FORM, g, J, e[6], e[7]);
    if (FORM != 0)
    {
      const long long got[11] = {g.qx, g.qy, g.qz, g.cur, g.xn, g.xl, g.yn, g.yl, g.zn, g.zl, g.ok};
      const long long want[11] = {plain.qx, plain.qy, plain.qz, plain.cur, plain.xn, plain.xl, plain.yn, plain.yl, plain.zn, plain.zl, plain.ok};
#pragma unroll
      for (int k = 0; k < 11; ++k)
        if (got[k] != want[k]) fail(rep, s, 1000 * cs.window + idx, 10 + k, FORM, got[k], want[k]);
    }
    ++c;
  }
  count(rep, c);
}

template <class T>
static T *upload(const void *src, size_t bytes)
{
  T *d;
  CHECK_HIP(hipMalloc((void **)&d, bytes ? bytes : 1));
  CHECK_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
  return d;
}
template <class T>
static bool read_vec(FILE *f, std::vector<T> &v, size_t n)
{
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}
static int short_file(const char *path)
{
  printf("%s: short case file\n", path);
  return 2;
}

int main(int argc, char **argv)
{
  if (argc < 2)
  {
    printf("usage: points_units CASEFILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int32_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!f || fread(head, sizeof(int32_t), 8, f) != 8 || head[0] != MAGIC || head[1] < 1 || head[2] < 1 || head[3] < 1 || head[4] < 1 || head[5] < 0 ||
      head[6] < 1 || head[7] < 1)
  {
    printf("%s: not a case file\n", argv[1]);
    return 2;
  }
  const uint32_t n_vals = (uint32_t)head[1], n_w = (uint32_t)head[2], n_pt = (uint32_t)head[3], n_pat = (uint32_t)head[4], n_win = (uint32_t)head[5],
                 n_points = (uint32_t)head[6], n_steps = (uint32_t)head[7];
  std::vector<int32_t> vals, weights, waves;
  std::vector<uint32_t> pt, pat;
  if (!read_vec(f, vals, n_vals) || !read_vec(f, weights, n_w) || !read_vec(f, pt, (size_t)n_pt * GW) || !read_vec(f, waves, n_pat) ||
      !read_vec(f, pat, (size_t)n_pat * REG_THREADS * GW))
    return short_file(argv[1]);
  for (uint32_t p = 0; p < n_pat; ++p)
    if (waves[p] < 0 || waves[p] > WAVES)
    {
      printf("%s: pattern %u has %d waves\n", argv[1], p, waves[p]);
      return 2;
    }

  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));

  // ---- 1. the point terms
  {
    int32_t *d_vals = upload<int32_t>(vals.data(), vals.size() * 4), *d_w = upload<int32_t>(weights.data(), weights.size() * 4);
    begin();
    k_gradient<<<dim3(GRID), dim3(BLOCK)>>>(d_vals, n_vals, d_w, n_w, g_rep);
    finish("central_gradient", (unsigned long long)n_vals * n_w * n_vals * n_w);
    uint32_t *d_pt = upload<uint32_t>(pt.data(), pt.size() * 4);
    begin();
    k_point_terms<<<dim3(GRID), dim3(BLOCK)>>>(d_pt, n_pt, g_rep);
    finish("point_terms", n_pt);
    CHECK_HIP(hipFree(d_vals));
    CHECK_HIP(hipFree(d_w));
    CHECK_HIP(hipFree(d_pt));
  }

  // ---- 2. the sums
  {
    // the host's totals: plain uint64 additions, lane after lane, of the restated terms
    std::vector<uint64_t> want((size_t)n_pat * 2 * REG_SLOTS, 0);
    for (uint32_t p = 0; p < n_pat; ++p)
      for (uint32_t pass = 0; pass < 2; ++pass)
      {
        uint64_t *t = &want[((size_t)p * 2 + pass) * REG_SLOTS];
        const uint32_t *data = &pat[(size_t)((p + pass) % n_pat) * REG_THREADS * GW];
        for (int lane = 0; lane < 64 * waves[p]; ++lane)
        {
          const RefTerms r = ref_point_terms(data + (size_t)lane * GW);
          for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) t[tri_index(i, j)] += (uint64_t)r.J[i] * (uint64_t)r.J[j];
          for (int i = 0; i < 6; ++i) t[21 + i] += (uint64_t)r.J[i] * (uint64_t)r.v;
          t[27] += (uint64_t)(r.v < 0 ? -r.v : r.v);
          t[28] += (uint64_t)r.used;
        }
      }
    uint32_t *d_pat = upload<uint32_t>(pat.data(), pat.size() * 4);
    int32_t *d_waves = upload<int32_t>(waves.data(), waves.size() * 4);
    const size_t n_out = (size_t)n_pat * 2 * REG_SLOTS, n_left = (size_t)n_pat * 2 * (REG_SLOTS + MF_AUX);
    unsigned long long *d_out, *d_left;
    CHECK_HIP(hipMalloc((void **)&d_out, n_out * 8));
    CHECK_HIP(hipMalloc((void **)&d_left, n_left * 8));
    std::vector<unsigned long long> out(n_out), left(n_left);
    for (int mfma = 0; mfma < 2; ++mfma)
    {
      CHECK_HIP(hipMemset(d_out, 0xff, n_out * 8));
      CHECK_HIP(hipMemset(d_left, 0xff, n_left * 8));
      if (mfma)
        k_sums<true><<<dim3(n_pat), dim3(REG_THREADS)>>>(d_pat, d_waves, n_pat, d_out, d_left);
      else
        k_sums<false><<<dim3(n_pat), dim3(REG_THREADS)>>>(d_pat, d_waves, n_pat, d_out, d_left);
      CHECK_HIP(hipGetLastError());
      CHECK_HIP(hipMemcpy(out.data(), d_out, n_out * 8, hipMemcpyDeviceToHost));
      CHECK_HIP(hipMemcpy(left.data(), d_left, n_left * 8, hipMemcpyDeviceToHost));
      Report r = {};
      for (uint32_t p = 0; p < n_pat; ++p)
        for (uint32_t pass = 0; pass < 2; ++pass)
          for (uint32_t s = 0; s < (uint32_t)REG_TERMS; ++s)
          {
            const size_t i = ((size_t)p * 2 + pass) * REG_SLOTS + s;
            if ((uint64_t)out[i] != want[i]) host_fail(r, p, pass, s, mfma, (long long)out[i], (long long)want[i]);
            ++r.checked;
          }
      finish_host(mfma ? "sums mfma" : "sums int64", r, (unsigned long long)n_pat * 2 * REG_TERMS);
      if (mfma)
      {
        Report z = {};
        for (size_t i = 0; i < n_left; ++i)
        {
          if (left[i] != 0ull) host_fail(z, (long long)(i / (2 * (REG_SLOTS + MF_AUX))), (long long)(i / (REG_SLOTS + MF_AUX) % 2), (long long)(i % (REG_SLOTS + MF_AUX)), 0, (long long)left[i], 0);
          ++z.checked;
        }
        finish_host("mfma_finalize zeroes", z, n_left);
      }
    }
    CHECK_HIP(hipFree(d_pat));
    CHECK_HIP(hipFree(d_waves));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_left));
  }

  // ---- 3. the gathers
  {
    struct Window
    {
      GatherCase cs;
      uint32_t *data;
      int32_t *points, *steps, *expect;
    };
    std::vector<Window> wins;
    for (uint32_t w = 0; w < n_win; ++w)
    {
      int32_t wh[12];
      std::vector<uint32_t> data;
      std::vector<int32_t> points, steps, expect;
      if (fread(wh, 4, 12, f) != 12 || wh[10] < 27 || (int64_t)wh[0] * wh[1] * wh[2] != (int64_t)wh[10] || wh[9] < 1) return short_file(argv[1]);
      if (!read_vec(f, data, (size_t)wh[10]) || !read_vec(f, points, (size_t)n_points * 3) || !read_vec(f, steps, (size_t)n_steps * 16) ||
          !read_vec(f, expect, (size_t)n_steps * n_points * 8))
        return short_file(argv[1]);
      Window win;
      win.data = upload<uint32_t>(data.data(), data.size() * 4);
      win.points = upload<int32_t>(points.data(), points.size() * 4);
      win.steps = upload<int32_t>(steps.data(), steps.size() * 4);
      win.expect = upload<int32_t>(expect.data(), expect.size() * 4);
      GatherCase &cs = win.cs;
      cs.a.points = win.points;
      cs.a.first = 0;
      cs.a.end = n_points;
      cs.a.map_data = win.data;
      for (int k = 0; k < 3; ++k)
      {
        cs.a.map.size[k] = wh[k];
        cs.a.map.pos[k] = wh[3 + k];
        cs.a.map.offset[k] = wh[6 + k];
      }
      cs.a.resdiv = make_fastdiv(wh[9]);
      cs.steps = win.steps;
      cs.expect = win.expect;
      cs.n_steps = n_steps;
      cs.n_points = n_points;
      cs.window = w;
      wins.push_back(win);
    }
    const unsigned long long per_form = (unsigned long long)n_win * n_steps * n_points;
    const dim3 grid((n_points + 63) / 64), block(64);
    begin();
    for (const Window &w : wins) k_gather<0><<<grid, block>>>(w.cs, g_rep);
    finish("gather_point", per_form);
    begin();
    for (const Window &w : wins) k_gather<1><<<grid, block>>>(w.cs, g_rep);
    finish("gather_point<true>", per_form);
    begin();
    for (const Window &w : wins) k_gather<2><<<grid, block>>>(w.cs, g_rep);
    finish("gather_point_loop", per_form);
    for (const Window &w : wins)
    {
      CHECK_HIP(hipFree(w.data));
      CHECK_HIP(hipFree(w.points));
      CHECK_HIP(hipFree(w.steps));
      CHECK_HIP(hipFree(w.expect));
    }
  }
  fclose(f);
  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
