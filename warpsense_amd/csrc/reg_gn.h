// reg_gn.h — the Gauss-Newton update of the registration kernels (gfx950), second layer: the 6x6 solve on one wave, xi -> SE(3),
// the convergence test and the pose in the forms the passes over the points read it in.  Everything here is executed by one whole
// wave whose lanes hold the same state.
#pragma once

#include "reg_reduce.h"

namespace ws
{
#ifndef WS_SOLVE_DIAG_FIRST
#define WS_SOLVE_DIAG_FIRST 1
#endif

// ---- 6x6 solve on one wave: Gauss-Jordan with partial pivoting in double, the same operations in the same order as
// oracle/ws_oracle.c:wso_solve6 (Eigen hf.inverse()*g, tsdf_registration.cpp:69), so the result is bit-identical
// to a serial solve.  Lane 8*r + c holds element (r, c) of the augmented matrix [A | b] (c == 6 is b): the 5
// divisions and the rank-1 update of an elimination step are one instruction each instead of 5 / 35, and no
// element ever needs a dynamic register index (a serial version spills the matrix to scratch for the row swap:
// 2.9 us per solve on one lane).  All 64 lanes of the wave must be active.
//
// The solve is one wave's chain of ~500 instructions in the middle of every Gauss-Newton iteration.  Measured with
// tools/solve_bench.hip (cycles per solve on one wave): what costs is every hop through the scalar unit.  The pivot
// candidates are uniform, so the compiler compares them into an SGPR mask, selects with s_cselect and moves the winner
// back with v_mov -- 70 cycles per candidate, 1050 of 3360 per solve.  Copied into VGPRs behind an opaque asm the
// same search is v_cmp + v_cndmask, ~20 cycles per candidate: 2660 cycles per solve.  (Tried and slower: rows that
// stay in place + DPP instead of two of the three gathers (4130), the reciprocal half of each division hoisted off the
// dependency chain (2860-3150), a tournament instead of the chain (3690): the wave is bound by instruction issue, not
// by the length of the chain.)
__device__ __forceinline__ double lane_read(double v, int src_lane /* uniform */)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_gather(double v, int src_lane /* per lane */)
{
  const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// the same value in a vector register the compiler knows nothing about (keeps what follows out of the scalar unit)
__device__ __forceinline__ double in_vgpr(double v)
{
  asm volatile("" : "+v"(v));
  return v;
}

template <typename V>
__device__ __forceinline__ void pin_vgpr(V &v)
{
  static_assert(sizeof(V) == 4, "32-bit values");
  asm volatile("" : "+v"(v));
}

// a: this lane's element of [A | b].  Returns 0 and x (identical in every lane), or -1 for a singular matrix.
// Gauss-Jordan with partial pivoting, the same operations in the same order as oracle/ws_oracle.c:wso_solve6 (round 5; LU +
// back substitution before): every step clears its column in ALL other rows -- in this layout the rows above the pivot cost
// nothing, they are other lanes of the same instruction -- and the multipliers come from the pivot's reciprocal, so after the
// sixth step x[i] = b[i] / pivot i is one multiplication.  Gone: the back substitution's six chained divisions, fifteen
// multiply-subtracts and 42 operand fetches through v_readlane.
__device__ __forceinline__ int solve6_wave(double a, double (&x)[6])
{
  const int lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
  int singular = 0;
  double inv[6];
#pragma unroll
  for (int k = 0; k < 6; ++k)
  {
    // pivot: first row of maximal |A[i][k]|, i >= k
    double pv, an, rowk, colk;
#if WS_SOLVE_DIAG_FIRST
    // The diagonal element keeps its place unless an element BELOW it is strictly larger (the search takes the first maximum):
    // every lane of the column compares its own element with the diagonal, one ballot decides.  Then nothing changes places
    // -- no candidate chain (8 instructions per candidate), no gather of the swapped row.  The normal equations of a scan put
    // the large rotational terms first, so this is the usual case; otherwise the general search below runs.
    const double dk = lane_read(a, 8 * k + k);
    const bool below_larger = c == k && r > k && r < 6 && fabs(a) > fabs(dk);
    if (__ballot(below_larger) == 0ull)
    {
      pv = in_vgpr(dk);
      an = a;
      rowk = lane_gather(a, 8 * k + c);
      colk = lane_gather(a, 8 * r + k);
    }
    else
#endif
    {
      int piv = k;
      pv = in_vgpr(lane_read(a, 8 * k + k));
#pragma unroll
      for (int i = k + 1; i < 6; ++i)
      {
        const double v = in_vgpr(lane_read(a, 8 * i + k));
        const bool larger = fabs(v) > fabs(pv);
        pv = larger ? v : pv;
        piv = larger ? i : piv;
      }
      // rows k and piv change places; fetch the swapped element, the pivot row and the k-th column in one go
      const int rr = r == k ? piv : (r == piv ? k : r);
      an = lane_gather(a, 8 * rr + c);
      rowk = lane_gather(a, 8 * piv + c);
      colk = lane_gather(a, 8 * rr + k);
    }
    singular |= pv == 0.0 ? 1 : 0; // the exit is taken once, below (x is not used then)
    inv[k] = 1.0 / pv;
    const double f = colk * inv[k];
    a = (r != k && c > k) ? an - f * rowk : an;
  }
  if (__builtin_amdgcn_readfirstlane(singular) != 0) return -1;
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = lane_read(a, 8 * i + 6) * inv[i];
  return 0;
}

// One Gauss-Newton update (tsdf_registration.cpp:63-92, registration/util.h:5-39), executed by one whole wave;
// every lane holds the same state and computes the same result.  H(r, c), G(r): the int64 sums.
#ifdef WS_REG_TIMING_GN
__device__ long long g_gn_ticks[5];
#define WS_GN_STAMP(i) const long long gn_t##i = wall_clock64()
#else
#define WS_GN_STAMP(i)
#endif

// First half: solve for xi and build the incremental transform `tr` (column-major 4x4).  false: no update this time
// (loop already over, no correspondences, singular matrix).
// what xi_to_transform (registration/util.h:5-39) needs to build the incremental transform
struct GnStep
{
  float L01, L02, L10, L12, L20, L21; // the skew matrix of the unit axis (all +0 for a zero rotation, like the reference's initialiser)
  float s, omc;                       // (float)sin theta, (float)(1 - cos theta)
  float t3, t4, t5;                   // (float)xi[3..5]
};

// Solve for xi and reduce it to GnStep.  false: no update this time (loop already over, no correspondences, singular matrix).
template <typename HF, typename GF>
__device__ __forceinline__ bool gn_step(GnCore &st, HF H, GF G, int32_t c, GnStep &o)
{
  if (st.finished || st.iterations >= st.max_iterations) return false;
  st.iterations += 1;
  if (c == 0)
  {
    st.finished = 1; // guard: the reference would divide by zero (tsdf_registration.cpp:80)
    return false;
  }
  WS_GN_STAMP(0);
  const double w = (double)(st.alpha * (float)c);
  const int lane = threadIdx.x & 63, lr = lane >> 3, lc = lane & 7;
  double a = 0.0;
  if (lr < 6 && lc < 6) a = (double)H(lr, lc) + (lr == lc ? w : 0.0);
  if (lr < 6 && lc == 6) a = (double)G(lr);
  double xi[6];
  WS_GN_STAMP(1);
  if (solve6_wave(a, xi) != 0)
  {
    st.finished = 1;
    return false;
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) xi[r] = -xi[r];
  WS_GN_STAMP(2);

  // xi_to_transform
  const double theta = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
  o.L01 = o.L02 = o.L10 = o.L12 = o.L20 = o.L21 = 0.f;
  if (theta != 0.0)
  {
    const double lx = xi[0] / theta, ly = xi[1] / theta, lz = xi[2] / theta;
    o.L01 = (float)-lz; o.L02 = (float)ly;
    o.L10 = (float)lz;  o.L12 = (float)-lx;
    o.L20 = (float)-ly; o.L21 = (float)lx;
  }
  double sin_t, cos_t;
  if (theta < 0.25)
  {
    // Gauss-Newton steps are small rotations: Taylor polynomials (truncation < 1e-19 below 0.25 rad) instead of the
    // library's sincos with its argument reduction (428 -> 184 cycles on the one wave everybody waits for).  What the
    // update uses are (float)sin and (float)(1 - cos): the cosine is summed with its rounding error carried (u + (e + w)),
    // so that 1 - cos_t cancels like the host's correctly rounded cos() does -- against glibc on 20 million angles in
    // [1e-9, 0.25] both floats agree in every case (the plain polynomial misses (float)(1 - cos) in 0.2 % of them).
    // (Horner steps as explicit fused multiply-adds -- half the length of the dependent chain; tools/polycheck.c: both forms
    // give libm's two floats on 20 million angles.)
    const double z = theta * theta;
    double p = fma(z, 1.0 / 6227020800.0, -1.0 / 39916800);
    p = fma(z, p, 1.0 / 362880);
    p = fma(z, p, -1.0 / 5040);
    p = fma(z, p, 1.0 / 120);
    p = fma(z, p, -1.0 / 6);
    sin_t = fma(theta * z, p, theta);
    double q = fma(z, -1.0 / 87178291200.0, 1.0 / 479001600.0);
    q = fma(z, q, -1.0 / 3628800);
    q = fma(z, q, 1.0 / 40320);
    q = fma(z, q, -1.0 / 720);
    q = fma(z, q, 1.0 / 24);
    const double t = 0.5 * z, u = 1.0 - t, e = (1.0 - u) - t, ww = z * z * q;
    cos_t = u + (e + ww);
  }
  else
    sincos(theta, &sin_t, &cos_t); // one argument reduction for both
  o.s = (float)sin_t;
  o.omc = (float)(1 - cos_t);
  o.t3 = (float)xi[3];
  o.t4 = (float)xi[4];
  o.t5 = (float)xi[5];
  WS_GN_STAMP(3);
#ifdef WS_REG_TIMING_GN
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    g_gn_ticks[0] += gn_t1 - gn_t0;
    g_gn_ticks[1] += gn_t2 - gn_t1;
    g_gn_ticks[2] += gn_t3 - gn_t2;
    g_gn_ticks[4] += 1;
  }
#endif
  return true;
}

// First half: solve for xi and build the incremental transform `tr` (column-major 4x4).  false: no update this time
// (loop already over, no correspondences, singular matrix).
template <typename HF, typename GF>
__device__ __forceinline__ bool gn_increment(GnCore &st, HF H, GF G, int32_t c, float (&tr)[16])
{
  GnStep o;
  if (!gn_step(st, H, G, c, o)) return false;
  const float L[3][3] = {{0.f, o.L01, o.L02}, {o.L10, 0.f, o.L12}, {o.L20, o.L21, 0.f}};
  const float s = o.s, omc = o.omc;
  float R[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
      float ll = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) ll = __fadd_rn(ll, __fmul_rn(__fmul_rn(omc, L[i][k]), L[k][j]));
      R[i][j] = __fadd_rn(__fadd_rn((i == j ? 1.f : 0.f), __fmul_rn(s, L[i][j])), ll);
    }
#pragma unroll
  for (int i = 0; i < 16; ++i) tr[i] = 0.f;
  tr[15] = 1.f;
  const float oc0 = -(float)st.center[0], oc1 = -(float)st.center[1], oc2 = -(float)st.center[2];
  const float tx[3] = {o.t3, o.t4, o.t5};
#pragma unroll
  for (int i = 0; i < 3; ++i)
  {
#pragma unroll
    for (int j = 0; j < 3; ++j) tr[j * 4 + i] = R[i][j];
    const float shift = __fadd_rn(__fadd_rn(__fmul_rn(R[i][0], oc0), __fmul_rn(R[i][1], oc1)), __fmul_rn(R[i][2], oc2));
    tr[12 + i] = __fadd_rn(__fadd_rn(shift, (float)st.center[i]), tx[i]);
  }
  st.alpha = __fadd_rn(st.alpha, st.it_weight_gradient);
  return true;
}

// Second half: convergence test on the mean error (tsdf_registration.cpp:80-92)
__device__ __forceinline__ void gn_convergence(GnCore &st, int32_t e, int32_t c)
{
  const float err = __fdiv_rn((float)e, (float)c);
  if (fabsf(err - st.prev[2]) < st.epsilon && fabsf(err - st.prev[0]) < st.epsilon) st.finished = 1;
  st.prev[0] = st.prev[1];
  st.prev[1] = st.prev[2];
  st.prev[2] = st.prev[3];
  st.prev[3] = err;
}

// T = tr * T with every lane computing all 16 elements (uniform state)
__device__ __forceinline__ void pose_product(float (&T)[16], const float (&tr)[16])
{
  float out[16];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc = __fadd_rn(acc, __fmul_rn(tr[k * 4 + i], T[j * 4 + k]));
      out[j * 4 + i] = acc;
    }
#pragma unroll
  for (int i = 0; i < 16; ++i) T[i] = out[i];
}

// ---- phase B building blocks (registration.cu:194-257 + :41-118 fused) ----
struct IntTransform
{
  int32_t M[12];
  int32_t cx, cy, cz;
};

// The pose as make_int_transform needs it, next to the float pose in LDS: TI[4 j + i] = (int)(T[4 j + i] * 32768) for the rows
// i < 3, and the integer centre (int)T[12 + i] in the fourth-row places 3, 7, 11.  Written by the lane that has just computed
// the element (two instructions on the first wave) instead of 22 conversions in each of the eight waves of every iteration.
__device__ __forceinline__ void store_int_pose(int32_t *TI_sh, int lane /* < 16: element (lane & 3, lane >> 2) */, float v)
{
  const int i = lane & 3, j = lane >> 2;
  if (i < 3) TI_sh[lane] = (int32_t)(v * (float)MATRIX_RESOLUTION);
  if (j == 3 && i < 3) TI_sh[4 * i + 3] = (int32_t)v;
}
__device__ __forceinline__ IntTransform load_int_pose(const int32_t *TI_sh)
{
  IntTransform t;
  int32_t w[16];
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    const int4 v = *reinterpret_cast<const int4 *>(TI_sh + 4 * q);
    w[4 * q + 0] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) t.M[j * 3 + i] = w[j * 4 + i];
  t.cx = w[3];
  t.cy = w[7];
  t.cz = w[11];
  return t;
}

// cu_to_int_mat (cuda/util.h:24-35): (int)(float * 32768); registration.cu:208: center = (int) translation of the CURRENT transform
__device__ __forceinline__ IntTransform make_int_transform(const float *T)
{
  IntTransform t;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) t.M[j * 3 + i] = (int32_t)(T[j * 4 + i] * (float)MATRIX_RESOLUTION);
  t.cx = (int32_t)T[12];
  t.cy = (int32_t)T[13];
  t.cz = (int32_t)T[14];
  return t;
}

// One Gauss-Newton update with the whole state in registers, identical in every lane of the wave
template <typename HF, typename GF>
__device__ __forceinline__ void gn_update(GnCore &st, HF H, GF G, int32_t e, int32_t c)
{
  float tr[16];
  if (!gn_increment(st, H, G, c, tr)) return;
  pose_product(st.T, tr);
  gn_convergence(st, e, c);
}

// the update fed from the 29 reduced terms in LDS
__device__ __forceinline__ void gn_update_terms(GnCore &st, const int64_t *terms)
{
  gn_update(
      st, [terms](int r, int c) { return terms[h_slot(r, c)]; }, [terms](int r) { return terms[word_slot(36 + r)]; },
      (int32_t)terms[word_slot(42)], (int32_t)terms[word_slot(43)]);
}

// The update fed from REGISTERS (reg_loop_kernel): `total` is what the exchange left in lanes 0 .. 31 (the total of slot
// `lane`), `Tel` the pose element (lane & 3, (lane >> 2) & 3) in lanes 0 .. 15.  Lane 8 r + c fetches its element of [H | g] with
// one ds_bpermute pair and the pose's column comes over the quad with DPP: no LDS write -> read round trip between the
// exchange and the solve, none between the increment and the product.  Same operations per element as gn_update.
__device__ __forceinline__ void gn_update_total(GnCore &st, int64_t total, float &Tel, float *T_sh, int32_t *TI_sh)
{
  const int lane = threadIdx.x & 63, lr = lane >> 3, lc = lane & 7;
  int src = 29; // an empty slot
  if (lr < 6 && lc < 6) src = h_slot(lr, lc);
  if (lr < 6 && lc == 6) src = word_slot(36 + lr);
  const int lo = __builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)((uint64_t)total & 0xffffffffull));
  const int hi = __builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)((uint64_t)total >> 32));
  const int64_t mine = pack64(lo, hi);
  // (uniform values the vector unit computes with: kept out of the scalar registers, like the loop state; the low 32 bits are the
  // `int` words 42, 43)
  int32_t e = __builtin_amdgcn_ds_bpermute(word_slot(42) << 2, (int)(uint32_t)((uint64_t)total & 0xffffffffull));
  int32_t c = __builtin_amdgcn_ds_bpermute(word_slot(43) << 2, (int)(uint32_t)((uint64_t)total & 0xffffffffull));
  pin_vgpr(e);
  pin_vgpr(c);
  GnStep o;
  if (!gn_step(
          st, [mine](int, int) { return mine; }, [mine](int) { return mine; }, c, o))
    return;
  // T = tr * T: lane 4 j + i computes element (i, j) and needs ROW i of tr only -- built here per lane (the same operations
  // in the same order as gn_increment does for that row: 60 instructions instead of the 170 of all sixteen elements in every
  // lane plus twelve selects).  Row 3 of tr is (0, 0, 0, 1): its lanes select zeros and compute exactly that.
  // (The selects are v_cndmask on lane masks: as C selects over an array the compiler turned them into an INDEXED read, i.e. a
  // copy in scratch memory and a round trip to it in the middle of the chain.)
  const unsigned long long m1 = 0xaaaaaaaaaaaaaaaaull, m2 = 0xccccccccccccccccull; // lanes with bit 0 / bit 1 of the row set
  auto pick = [](float a, float b, unsigned long long mask) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
    return r;
  };
  auto row4 = [&](float r0, float r1, float r2, float r3) { return pick(pick(r0, r1, m1), pick(r2, r3, m1), m2); };
  const float L[3][3] = {{0.f, o.L01, o.L02}, {o.L10, 0.f, o.L12}, {o.L20, o.L21, 0.f}};
  const float Li[3] = {row4(0.f, o.L10, o.L20, 0.f), row4(o.L01, 0.f, o.L21, 0.f), row4(o.L02, o.L12, 0.f, 0.f)}; // L[i][0..2]
  const float dl[3] = {row4(1.f, 0.f, 0.f, 0.f), row4(0.f, 1.f, 0.f, 0.f), row4(0.f, 0.f, 1.f, 0.f)};            // i == j
  float row[4];
#pragma unroll
  for (int j = 0; j < 3; ++j)
  {
    float ll = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) ll = __fadd_rn(ll, __fmul_rn(__fmul_rn(o.omc, Li[k]), L[k][j]));
    row[j] = __fadd_rn(__fadd_rn(dl[j], __fmul_rn(o.s, Li[j])), ll);
  }
  {
    const float oc0 = -(float)st.center[0], oc1 = -(float)st.center[1], oc2 = -(float)st.center[2];
    const float shift = __fadd_rn(__fadd_rn(__fmul_rn(row[0], oc0), __fmul_rn(row[1], oc1)), __fmul_rn(row[2], oc2));
    const float ci = row4((float)st.center[0], (float)st.center[1], (float)st.center[2], 0.f), ti = row4(o.t3, o.t4, o.t5, 0.f);
    row[3] = pick(__fadd_rn(__fadd_rn(shift, ci), ti), 1.f, m1 & m2); // tr[15] = 1
  }
  st.alpha = __fadd_rn(st.alpha, st.it_weight_gradient);
  const int tb = __float_as_int(Tel);
  const float tk[4] = {__int_as_float(__builtin_amdgcn_update_dpp(0, tb, 0x00, 0xf, 0xf, false)),  // quad_perm [0,0,0,0]: column j of the old
                       __int_as_float(__builtin_amdgcn_update_dpp(0, tb, 0x55, 0xf, 0xf, false)),  // [1,1,1,1]     pose sits in the lane's quad
                       __int_as_float(__builtin_amdgcn_update_dpp(0, tb, 0xaa, 0xf, 0xf, false)),  // [2,2,2,2]
                       __int_as_float(__builtin_amdgcn_update_dpp(0, tb, 0xff, 0xf, 0xf, false))}; // [3,3,3,3]
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) acc = __fadd_rn(acc, __fmul_rn(row[k], tk[k]));
  Tel = acc;
  if (lane < 16)
  {
    T_sh[lane] = acc;
    store_int_pose(TI_sh, lane, acc);
  }
  gn_convergence(st, e, c);
}

} // namespace ws
