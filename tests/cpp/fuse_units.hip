// fuse_units.hip — the integer rules of ws_store_fuse (ws_fuse.h), evaluated ON THE DEVICE and held to a plain restatement of the same
// operation over the domain each helper's comment claims: fuse_div with make_fuse_div, fuse_pull and fuse_dead, fuse_integrate, and
// fuse_sample on a small field of chunks.  The restatement is computed in the same thread with uint64 / int64 / __int128 and the
// built-in / and %; it never calls the helper under test, FastDiv, or the chunk lookup of ws_field_store.h.  Every mismatch is counted;
// the first few are recorded with their inputs.  Prints one line per subject, exits 1 on any mismatch.
#include <cstdint>
#include <vector>

#include "ws_fuse.h"

#include "unit_report.hpp"

using namespace ws;
typedef __int128 i128;

// ---- fuse_div(n, make_fuse_div(d)): M and k come from the header's own inline function, run on the host, and are passed in.
// (a) the domain of fuse_sample: d = res^3 for every res in 1 .. 1024, n from {j d - 1, j d, j d + 1, j d + d / 2} for j in 0 .. 65536,
// held to [0, 2^16 d): per resolution 4 65537 cases less j = 0's -1 and the three beyond the end at j = 65536; at d = 1 also
// 65535 + 1.  1024 262144 - 1 cases.
constexpr uint64_t DIVA_PER_RES = 4ull * 65537, DIVA_SPACE = 1024 * DIVA_PER_RES, DIVA_CASES = 1024ull * 262144 - 1;
__global__ void k_div_res3(const FuseDiv *fd, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const uint64_t res = 1 + i / DIVA_PER_RES, t = i % DIVA_PER_RES, j = t >> 2, d = res * res * res;
    const uint32_t v = (uint32_t)(t & 3);
    if (j == 0 && v == 0) continue;
    const uint64_t x = v == 0 ? j * d - 1 : (v == 1 ? j * d : (v == 2 ? j * d + 1 : j * d + d / 2));
    if (x >= (d << 16)) continue;
    const uint64_t got = fuse_div(x, fd[res]), want = x / d;
    if (got != want) fail(rep, (long long)x, (long long)d, (long long)fd[res].M, fd[res].k, (long long)got, (long long)want);
    ++c;
  }
  count(rep, c);
}

// (b) the routine's own claim, 0 <= n < 2^47 and 1 <= d <= 2^30: per divisor of the list 2048 multiples j d with j d - 1 beside each
// (j = 1 .. 1024 and the last 1024 below 2^47; those that do not exist for a large d are left out and not counted), the largest n,
// and 2^16 random n, half of them of every magnitude
constexpr uint64_t DIVB_J = 2048, DIVB_RANDOM = 1ull << 16, DIVB_PER_D = 2 * DIVB_J + 1 + DIVB_RANDOM, N47 = 1ull << 47;
__host__ __device__ inline bool divb_case(uint64_t d, uint64_t t, uint64_t seed, uint64_t &x)
{
  if (t < 2 * DIVB_J)
  {
    const uint64_t jmax = (N47 - 1) / d, s = t >> 1;
    if (s >= 1024 && jmax < 1024 + (s - 1024) + 1) return false; // (the j below jmax - 1023 .. jmax that j = 1 .. 1024 already are)
    const uint64_t j = s < 1024 ? s + 1 : jmax - (s - 1024);
    if (j < 1 || j > jmax) return false;
    x = j * d - ((t & 1) ? 0 : 1);
    return true;
  }
  if (t == 2 * DIVB_J)
  {
    x = N47 - 1;
    return true;
  }
  const uint64_t h = mix64(seed);
  x = (h >> 17) >> ((t & 1) ? mix64(h) % 47 : 0);
  return true;
}
__global__ void k_div_claim(const FuseDiv *fd, const uint32_t *divs, uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const uint64_t di = i / DIVB_PER_D, d = divs[di];
    uint64_t x;
    if (!divb_case(d, i % DIVB_PER_D, i, x)) continue;
    const uint64_t got = fuse_div(x, fd[di]), want = x / d;
    if (got != want) fail(rep, (long long)x, (long long)d, (long long)fd[di].M, fd[di].k, (long long)got, (long long)want);
    ++c;
  }
  count(rep, c);
}

// ---- fuse_pull(base, rot_z, dz, pivot_src) against floor((base + rot_z dz) / 2^30) + pivot_src in __int128 with a true floor.
// |base| <= 2^55 + 2^29 is what two products of |rot| <= 2^30 and |d| < 2^24 and the rounding term can give.
constexpr int N_ROT = 7, N_DZ = 5, N_PS = 5, N_MULT = 64;
constexpr uint64_t PULL_RANDOM = 1ull << 14, PULL_BASES = 2 + N_MULT * 5 + PULL_RANDOM, PULL_CASES = (uint64_t)N_ROT * N_DZ * N_PS * PULL_BASES;
constexpr int64_t BASE_MAX = 2 * (1ll << 54) + (1ll << 29);
__constant__ int64_t c_rot[N_ROT] = {1ll << 30, -(1ll << 30), (1ll << 30) - 1, -((1ll << 30) - 1), 1, -1, 0};
__constant__ int64_t c_dz[N_DZ] = {(1ll << 24) - 1, -((1ll << 24) - 1), 1, -1, 0};
__constant__ int64_t c_ps[N_PS] = {INT32_MIN, INT32_MAX, 1ll << 30, -(1ll << 30), 0};
__constant__ int64_t c_mult[8] = {0, 1, -1, 2, -2, 1ll << 24, -(1ll << 24), 12345};
__global__ void k_pull(uint64_t base0, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base0, n)
  {
    uint64_t t = i;
    const uint64_t bi = t % PULL_BASES;
    t /= PULL_BASES;
    const int64_t ps = c_ps[t % N_PS];
    t /= N_PS;
    const int64_t dz = c_dz[t % N_DZ], rz = c_rot[t / N_DZ];
    int64_t base;
    if (bi < 2)
      base = bi ? -BASE_MAX : BASE_MAX;
    else if (bi < 2 + N_MULT * 5)
    {
      // the sum within +-2 of a multiple m 2^30 of either sign (|m| <= 2^24: base stays in its domain)
      const uint64_t mi = (bi - 2) / 5;
      const int64_t m = mi < 8 ? c_mult[mi] : (int64_t)(mix64(mi) % ((1ull << 25) + 1)) - (1ll << 24);
      base = m * (1ll << 30) + (int64_t)((bi - 2) % 5) - 2 - rz * dz;
    }
    else
      base = (int64_t)(mix64(i) % (uint64_t)(2 * BASE_MAX + 1)) - BASE_MAX;
    const int64_t got = fuse_pull(base, (int32_t)rz, (int32_t)dz, (int32_t)ps);
    const i128 s = (i128)base + (i128)rz * (i128)dz, D = (i128)1 << 30;
    i128 q = s / D;
    if (s % D != 0 && s < 0) q -= 1;
    const i128 want = q + (i128)ps;
    if ((i128)got != want) fail(rep, base, rz, dz, ps, got, (long long)want);
    ++c;
  }
  count(rep, c);
}

// ---- fuse_dead(q): dead iff |q| >= 2^30
constexpr int N_DEAD = 11;
__constant__ int64_t c_dead[N_DEAD] = {1ll << 30, -(1ll << 30), (1ll << 30) - 1, -((1ll << 30) - 1), (1ll << 30) + 1, -((1ll << 30) + 1), 0, 1ll << 62, -(1ll << 62), 1, -1};
__global__ void k_dead(Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, 0, N_DEAD)
  {
    const int64_t q = c_dead[i];
    const i128 a = q < 0 ? -(i128)q : (i128)q;
    const bool want = a >= ((i128)1 << 30), got = fuse_dead(q);
    if (got != want) fail(rep, q, 0, 0, 0, got, want);
    ++c;
  }
  count(rep, c);
}

// ---- fuse_integrate(existing, nv, nw, max_weight) for a valid sample (nw > 0): the header's rule on int64 with the casts to int16
__device__ __forceinline__ uint32_t integrate_ref(int64_t ev, int64_t ew, int64_t nv, int64_t nw, int64_t max_weight)
{
  int64_t v = nv, w = nw;
  if (ew > 0)
  {
    v = (ev * ew + nv * nw) / (ew + nw);
    w = max_weight < ew + nw ? max_weight : ew + nw;
  }
  return ((uint32_t)(uint16_t)(int16_t)v) | ((uint32_t)(uint16_t)(int16_t)w << 16);
}
__device__ __forceinline__ uint32_t pack_ref(int64_t v, int64_t w) { return ((uint32_t)(uint16_t)(int16_t)v) | ((uint32_t)(uint16_t)(int16_t)w << 16); }
// every pair (ev, nv) of int16 values for each weight triple (ew, nw, max_weight) of the list
constexpr int N_TRIPLE = 12;
__constant__ int32_t c_triple[N_TRIPLE][3] = {{1, 1, 1},       {1, 1, 32767},   {32767, 32767, 32767}, {32767, 1, 640},     {1, 32767, 640},   {32766, 2, 32767},
                                              {0, 5, 640},     {-1, 5, 640},    {-32768, 32767, 640},  {32767, 32767, 1},   {300, 400, 640},   {16384, 16383, 32767}};
constexpr uint64_t INTEG_PAIRS = (uint64_t)N_TRIPLE << 32, INTEG_RANDOM = 1ull << 24;
__global__ void k_integrate_pairs(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const int32_t *t = c_triple[i >> 32];
    const int32_t ev = (int16_t)(uint16_t)i, nv = (int16_t)(uint16_t)(i >> 16);
    const uint32_t got = fuse_integrate(pack_ref(ev, t[0]), nv, t[1], t[2]), want = integrate_ref(ev, t[0], nv, t[1], t[2]);
    if (got != want) fail(rep, ev, t[0], nv, t[1], got, want);
    ++c;
  }
  count(rep, c);
}
// random quintuples: ev, nv, ew any int16, nw and max_weight in 1 .. 32767
__global__ void k_integrate_random(uint64_t base, uint64_t n, Report *rep)
{
  unsigned long long c = 0;
  FOR_RANGE(i, base, n)
  {
    const uint64_t h = mix64(i), g = mix64(h);
    const int32_t ev = (int16_t)(uint16_t)h, nv = (int16_t)(uint16_t)(h >> 16), ew = (int16_t)(uint16_t)(h >> 32);
    const int32_t nw = 1 + (int32_t)((g & 0xffffffffu) % 32767u), mw = 1 + (int32_t)((g >> 32) % 32767u);
    const uint32_t got = fuse_integrate(pack_ref(ev, ew), nv, nw, mw), want = integrate_ref(ev, ew, nv, nw, mw);
    if (got != want) fail(rep, pack_ref(ev, ew), nv, nw, mw, got, want);
    ++c;
  }
  count(rep, c);
}

// ---- fuse_sample.  SRC: the 2 x 2 x 2 chunk positions with keys -1 and 0 on each axis, (0, 0, 0) absent; seven chunks in two segments
// of four slots, found through the table store_ray_table_fill builds.  The restatement finds a voxel through a plain array of eight
// pointers instead.  The world voxels [-64, 64)^3 are filled in blocks of 8^3, the kind of a block drawn from its position.
constexpr int KIND_MIN = 0, KIND_MAX = 1, KIND_MIX = 2, KIND_RANDOM = 3, KIND_ZERO_W = 4, KIND_NEG_W = 5, KIND_ABSENT = 6, N_KIND = 7;
static const char *const kind_name[N_KIND] = {"all -32768", "all 32767", "mix of both", "random", "zero weight", "negative weight", "absent corner"};
static uint32_t fill_voxel(int x, int y, int z)
{
  static const int32_t weights[4] = {1, 2, 700, 32767};
  const uint64_t blk = mix64(((uint64_t)((x + 64) >> 3) << 16) | ((uint64_t)((y + 64) >> 3) << 8) | (uint64_t)((z + 64) >> 3)) % 6;
  const uint64_t h = mix64(0xF05Eull ^ ((uint64_t)(x + 64) << 32) ^ ((uint64_t)(y + 64) << 16) ^ (uint64_t)(z + 64));
  int32_t w = weights[h & 3], v;
  switch (blk)
  {
  case KIND_MIN: v = -32768; break;
  case KIND_MAX: v = 32767; break;
  case KIND_MIX: v = (h & 4) ? -32768 : 32767; break;
  default: v = (int16_t)(uint16_t)(h >> 16);
  }
  if (blk == KIND_ZERO_W && ((h >> 40) & 7) == 0) w = 0;
  if (blk == KIND_NEG_W && ((h >> 40) & 7) == 0) w = -1 - (int32_t)((h >> 44) & 0x7fff);
  return ((uint32_t)v & 0xffffu) | ((uint32_t)w << 16);
}
struct RefChunks
{
  const uint32_t *p[8]; // key (kx, ky, kz) in {-1, 0}^3 at (kx + 1) 4 + (ky + 1) 2 + (kz + 1); nullptr: absent
};
// b per axis: both sides of every chunk face of the arrangement, the outer ones included (the chunks beyond them are absent), and
// three places inside a chunk
constexpr int N_B = 15;
__constant__ int32_t c_b[N_B] = {-66, -65, -64, -63, -34, -3, -2, -1, 0, 1, 30, 62, 63, 64, 65};
constexpr uint64_t SAMPLE_GRID = (uint64_t)N_B * N_B * N_B * 64, SAMPLE_RANDOM = 1ull << 20, SAMPLE_PER_RES = SAMPLE_GRID + SAMPLE_RANDOM;
__global__ void k_sample(FuseArgs a, RefChunks ref, uint64_t base, uint64_t n, unsigned long long *kinds, Report *rep)
{
  unsigned long long c = 0;
  StoreRayArgs sa; // (only what lookup() reads)
  sa.table = a.src_table, sa.mask = a.src_mask, sa.segs = a.src_segs, sa.seg_shift = a.src_shift;
  StoreField fld(sa);
  FOR_RANGE(i, base, n)
  {
    int32_t b[3], f[3];
    if (i < SAMPLE_GRID)
    {
      uint64_t t = i;
      const int32_t pick[4] = {0, 1, a.res / 2, a.res - 1};
      for (int k = 0; k < 3; ++k)
      {
        f[k] = min(pick[t & 3], a.res - 1);
        t >>= 2;
      }
      for (int k = 0; k < 3; ++k)
      {
        b[k] = c_b[t % N_B];
        t /= N_B;
      }
    }
    else
    {
      const uint64_t h = mix64(i ^ ((uint64_t)a.res << 48)), g = mix64(h);
      for (int k = 0; k < 3; ++k)
      {
        b[k] = (int32_t)((h >> (16 * k)) & 0xffffu) % 132 - 66;
        f[k] = (int32_t)(((g >> (16 * k)) & 0xffffu) % (uint32_t)a.res);
      }
    }
    int32_t nv = 0, nw = 0;
    const bool got = fuse_sample(a, fld, b, f, nv, nw);
    // the rule (warpsense_hip.h at ws_store_fuse) in int64
    const int64_t res = a.res, res3 = res * res * res;
    int64_t T = 0, wmin = INT64_MAX;
    bool valid = true, any_absent = false, any_zero = false, any_neg = false, all_min = true, all_max = true, all_ext = true;
    for (int j = 0; j < 8; ++j)
    {
      const int cx = j >> 2, cy = (j >> 1) & 1, cz = j & 1;
      const int64_t coef = (cx ? f[0] : res - f[0]) * (cy ? f[1] : res - f[1]) * (cz ? f[2] : res - f[2]);
      const int64_t v[3] = {(int64_t)b[0] + cx, (int64_t)b[1] + cy, (int64_t)b[2] + cz};
      const uint32_t *p = nullptr;
      if (v[0] >= -64 && v[0] < 64 && v[1] >= -64 && v[1] < 64 && v[2] >= -64 && v[2] < 64) p = ref.p[(v[0] >= 0 ? 4 : 0) + (v[1] >= 0 ? 2 : 0) + (v[2] >= 0 ? 1 : 0)];
      int64_t val = 0, wt = 0;
      if (p)
      {
        const uint32_t raw = p[((v[0] + 64) % 64) * 4096 + ((v[1] + 64) % 64) * 64 + (v[2] + 64) % 64];
        val = (int16_t)(raw & 0xffffu), wt = (int16_t)(raw >> 16);
      }
      any_absent = any_absent || !p;
      any_zero = any_zero || (p && wt == 0);
      any_neg = any_neg || (p && wt < 0);
      all_min = all_min && val == -32768;
      all_max = all_max && val == 32767;
      all_ext = all_ext && (val == -32768 || val == 32767);
      if (coef == 0) continue; // takes part neither in validity nor in the weight
      if (!p || wt <= 0)
      {
        valid = false;
        continue;
      }
      wmin = wt < wmin ? wt : wmin;
      T += val * coef;
    }
    int64_t want = T / res3;
    if (T % res3 != 0 && T < 0) want -= 1;
    if (got != valid)
      fail(rep, ((long long)(b[0] + 66) << 16) | ((b[1] + 66) << 8) | (b[2] + 66), ((long long)f[0] << 20) | (f[1] << 10) | f[2], res, 0, got, valid);
    else if (valid && ((int64_t)nv != want || (int64_t)nw != wmin))
      fail(rep, ((long long)(b[0] + 66) << 16) | ((b[1] + 66) << 8) | (b[2] + 66), ((long long)f[0] << 20) | (f[1] << 10) | f[2], res, (int64_t)nw == wmin ? 1 : 2, nv, want);
    // the kind of the cell, by all eight corners whatever their coefficients
    const int kind = any_absent ? KIND_ABSENT : (any_neg ? KIND_NEG_W : (any_zero ? KIND_ZERO_W : (all_min ? KIND_MIN : (all_max ? KIND_MAX : (all_ext ? KIND_MIX : KIND_RANDOM)))));
    atomicAdd(kinds + kind, 1ull);
    // the ends of the shifted numerator: 0 and 2^16 res^3 - res^3
    if (valid && T == -32768 * res3) atomicAdd(kinds + N_KIND, 1ull);
    if (valid && T == 32767 * res3) atomicAdd(kinds + N_KIND + 1, 1ull);
    ++c;
  }
  count(rep, c);
}

int main()
{
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  const dim3 G(GRID), B(BLOCK);

  {
    std::vector<FuseDiv> fd(1025);
    unsigned long long lo = 0, hi = 0;
    for (int64_t r = 1; r <= 1024; ++r)
    {
      fd[r] = make_fuse_div(r * r * r);
      (fd[r].k < 64u ? lo : hi) += 1;
    }
    fd[0] = fd[1];
    FuseDiv *d_fd;
    CHECK_HIP(hipMalloc((void **)&d_fd, fd.size() * sizeof(FuseDiv)));
    CHECK_HIP(hipMemcpy(d_fd, fd.data(), fd.size() * sizeof(FuseDiv), hipMemcpyHostToDevice));
    begin();
    k_div_res3<<<G, B>>>(d_fd, 0, DIVA_SPACE, g_rep);
    finish("fuse_div res^3", DIVA_CASES);
    CHECK_HIP(hipFree(d_fd));

    // the claim: 2^e, 2^e - 1, 2^e + 1 within [1, 2^30], and 4096 random divisors, half of them of every magnitude
    std::vector<uint32_t> divs;
    for (int e = 0; e <= 30; ++e)
      for (int64_t o = -1; o <= 1; ++o)
      {
        const int64_t d = (1ll << e) + o;
        if (d >= 1 && d <= (1ll << 30)) divs.push_back((uint32_t)d);
      }
    for (uint64_t t = 0; t < 4096; ++t)
    {
      const uint64_t h = mix64(0xD1Dull + t);
      divs.push_back(1u + (uint32_t)((h % (1ull << 30)) >> ((t & 1) ? mix64(h) % 30 : 0)));
    }
    std::vector<FuseDiv> fb(divs.size());
    unsigned long long expect = 0;
    for (size_t k = 0; k < divs.size(); ++k)
    {
      fb[k] = make_fuse_div(divs[k]);
      (fb[k].k < 64u ? lo : hi) += 1;
      for (uint64_t t = 0; t < 2 * DIVB_J + 1; ++t)
      {
        uint64_t x;
        expect += divb_case(divs[k], t, 0, x) ? 1 : 0;
      }
      expect += DIVB_RANDOM;
    }
    uint32_t *d_divs;
    CHECK_HIP(hipMalloc((void **)&d_fd, fb.size() * sizeof(FuseDiv)));
    CHECK_HIP(hipMalloc((void **)&d_divs, divs.size() * sizeof(uint32_t)));
    CHECK_HIP(hipMemcpy(d_fd, fb.data(), fb.size() * sizeof(FuseDiv), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_divs, divs.data(), divs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    begin();
    k_div_claim<<<G, B>>>(d_fd, d_divs, 0, divs.size() * DIVB_PER_D, g_rep);
    finish("fuse_div claim", expect);
    printf("fuse_div branches      k < 64: %llu divisors  k >= 64: %llu divisors\n", lo, hi);
    if (lo == 0 || hi == 0) g_bad = 1;
    CHECK_HIP(hipFree(d_fd));
    CHECK_HIP(hipFree(d_divs));
  }

  begin();
  k_pull<<<G, B>>>(0, PULL_CASES, g_rep);
  finish("fuse_pull", PULL_CASES);
  begin();
  k_dead<<<G, B>>>(g_rep);
  finish("fuse_dead", N_DEAD);

  begin();
  chunked(INTEG_PAIRS, [&](uint64_t b, uint64_t n) { k_integrate_pairs<<<G, B>>>(b, n, g_rep); });
  finish("fuse_integrate pairs", INTEG_PAIRS);
  begin();
  k_integrate_random<<<G, B>>>(0, INTEG_RANDOM, g_rep);
  finish("fuse_integrate random", INTEG_RANDOM);

  {
    // seven chunks, slots 0 .. 6 in key order, four slots per segment
    const uint32_t seg_shift = 2;
    uint32_t *segs[2], **d_segs;
    for (int s = 0; s < 2; ++s) CHECK_HIP(hipMalloc((void **)&segs[s], (size_t)STORE_CHUNK_WORDS * 4 * sizeof(uint32_t)));
    CHECK_HIP(hipMalloc((void **)&d_segs, sizeof segs));
    CHECK_HIP(hipMemcpy(d_segs, segs, sizeof segs, hipMemcpyHostToDevice));
    std::vector<StoreRaySlot> listed;
    std::vector<uint32_t> chunk((size_t)STORE_CHUNK_WORDS);
    RefChunks ref;
    for (int kx = -1; kx <= 0; ++kx)
      for (int ky = -1; ky <= 0; ++ky)
        for (int kz = -1; kz <= 0; ++kz)
        {
          const int at = (kx + 1) * 4 + (ky + 1) * 2 + (kz + 1);
          ref.p[at] = nullptr;
          if (kx == 0 && ky == 0 && kz == 0) continue;
          const uint32_t slot = (uint32_t)listed.size();
          for (int x = 0; x < 64; ++x)
            for (int y = 0; y < 64; ++y)
              for (int z = 0; z < 64; ++z) chunk[(size_t)x * 4096 + y * 64 + z] = fill_voxel(kx * 64 + x, ky * 64 + y, kz * 64 + z);
          uint32_t *p = segs[slot >> seg_shift] + (size_t)(slot & 3u) * (size_t)STORE_CHUNK_WORDS;
          CHECK_HIP(hipMemcpy(p, chunk.data(), chunk.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
          ref.p[at] = p;
          listed.push_back(StoreRaySlot{kx, ky, kz, slot});
        }
    const size_t places = store_ray_table_slots(listed.size());
    std::vector<StoreRaySlot> table(places);
    store_ray_table_fill(listed.data(), listed.size(), table.data());
    StoreRaySlot *d_table;
    unsigned long long *d_kinds, kinds[N_KIND + 2];
    CHECK_HIP(hipMalloc((void **)&d_table, places * sizeof(StoreRaySlot)));
    CHECK_HIP(hipMemcpy(d_table, table.data(), places * sizeof(StoreRaySlot), hipMemcpyHostToDevice));
    CHECK_HIP(hipMalloc((void **)&d_kinds, sizeof kinds));
    CHECK_HIP(hipMemset(d_kinds, 0, sizeof kinds));

    // 40 | 41: the two shift branches of fuse_div; 645^3 < 2^28 < 646^3 and 812^3 < 2^29 < 813^3; 1024^3 = 2^30
    const int32_t reslist[10] = {1, 2, 7, 40, 41, 64, 645, 813, 1023, 1024};
    begin();
    for (int32_t res : reslist)
    {
      FuseArgs a = {};
      a.res = res, a.half = res / 2;
      a.res3 = (int64_t)res * res * res;
      a.tdiv = make_fuse_div(a.res3);
      a.src_table = d_table, a.src_mask = (uint32_t)places - 1u;
      a.src_segs = d_segs, a.src_shift = seg_shift;
      k_sample<<<G, B>>>(a, ref, 0, SAMPLE_PER_RES, d_kinds, g_rep);
    }
    finish("fuse_sample", 10 * SAMPLE_PER_RES);
    CHECK_HIP(hipMemcpy(kinds, d_kinds, sizeof kinds, hipMemcpyDeviceToHost));
    printf("fuse_sample cells     ");
    for (int k = 0; k < N_KIND; ++k) printf(" %s: %llu ", kind_name[k], kinds[k]);
    printf(" numerator 0: %llu  numerator at its maximum: %llu\n", kinds[N_KIND], kinds[N_KIND + 1]);
    for (int k = 0; k < N_KIND + 2; ++k)
      if (kinds[k] < 1000) g_bad = 1;
    for (int s = 0; s < 2; ++s) CHECK_HIP(hipFree(segs[s]));
    CHECK_HIP(hipFree(d_segs));
    CHECK_HIP(hipFree(d_table));
    CHECK_HIP(hipFree(d_kinds));
  }

  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
