// reg_points.h — a lane's points of the registration kernels (gfx950), third layer: transform, voxel + 6-neighbour gather (with
// the per-lane voxel cache of the resident kernels), gradient and Jacobian, and the 29 sums over the points in int64 registers or
// on the matrix cores; for the host, the points and the map as a launch passes them.
#pragma once

#include "reg_gn.h"

namespace ws
{
#ifndef WS_REG_MFMA
#define WS_REG_MFMA 1 // 0: the resident loop sums with v_mad_i64_i32 + the transposing butterfly for every cloud size
#endif

struct PointArgs
{
  const int32_t *points;
  uint32_t first;
  uint32_t end; // exclusive
  const uint32_t *map_data;
  MapParams map;
  FastDiv resdiv;
};

// ---- phase B building blocks (registration.cu:194-257 + :41-118 fused) ----

struct Gathered
{
  int32_t qx, qy, qz; // transformed point minus center
  uint32_t cur, xn, xl, yn, yl, zn, zl;
  bool ok;
};

// The voxel a point fell into at the previous iteration of the resident loop and the 7 entries read there.  Late in
// the Gauss-Newton loop the pose moves by a fraction of a millimetre per iteration, almost every point stays in its
// voxel, and a wave whose 128 points all stayed issues no load at all (the map does not change during the loop).
struct VoxelCache
{
  int32_t bx, by, bz;
  uint32_t cur, xn, xl, yn, yl, zn, zl;
  bool filled;
};

// transform one point and issue its 7 gathers (nothing here waits for memory)
template <bool CACHED = false>
__device__ __forceinline__ Gathered gather_point(const PointArgs &a, const IntTransform &t, int32_t px, int32_t py, int32_t pz, bool valid,
                                                 VoxelCache *cache = nullptr)
{
  Gathered g;
  // cu_transform_point (cuda/util.h:11-22), int32 wrap like the reference
  int32_t qx = wadd(wadd(wadd(wmul(t.M[0], px), wmul(t.M[3], py)), wmul(t.M[6], pz)), t.M[9]) / MATRIX_RESOLUTION;
  int32_t qy = wadd(wadd(wadd(wmul(t.M[1], px), wmul(t.M[4], py)), wmul(t.M[7], pz)), t.M[10]) / MATRIX_RESOLUTION;
  int32_t qz = wadd(wadd(wadd(wmul(t.M[2], px), wmul(t.M[5], py)), wmul(t.M[8], pz)), t.M[11]) / MATRIX_RESOLUTION;
  const int32_t bx = div_trunc(qx, a.resdiv), by = div_trunc(qy, a.resdiv), bz = div_trunc(qz, a.resdiv);
  g.qx = wsub(qx, t.cx);
  g.qy = wsub(qy, t.cy);
  g.qz = wsub(qz, t.cz);
  g.ok = valid && in_bounds_buffer(a.map, bx, by, bz, -1); // in_bounds_with_buffer_neg(buf, 1), registration.cu:217
  g.cur = g.xn = g.xl = g.yn = g.yl = g.zn = g.zl = 0;
  if (CACHED)
  {
    VoxelCache &c = *cache;
    const bool refill = g.ok && !(c.filled && c.bx == bx && c.by == by && c.bz == bz);
    if (refill) // one exec-mask region; everything else is selects
    {
      c.cur = a.map_data[get_index(a.map, bx, by, bz)];
      c.xn = a.map_data[get_index(a.map, bx + 1, by, bz)];
      c.xl = a.map_data[get_index(a.map, bx - 1, by, bz)];
      c.yn = a.map_data[get_index(a.map, bx, by + 1, bz)];
      c.yl = a.map_data[get_index(a.map, bx, by - 1, bz)];
      c.zn = a.map_data[get_index(a.map, bx, by, bz + 1)];
      c.zl = a.map_data[get_index(a.map, bx, by, bz - 1)];
      c.bx = bx;
      c.by = by;
      c.bz = bz;
      c.filled = true;
    }
    const uint32_t keep = g.ok ? 0xffffffffu : 0u;
    g.cur = c.cur & keep; g.xn = c.xn & keep; g.xl = c.xl & keep; g.yn = c.yn & keep; g.yl = c.yl & keep; g.zn = c.zn & keep; g.zl = c.zl & keep;
    return g;
  }
  if (g.ok)
  {
    // the 6 neighbours are in bounds by the test above
    g.cur = a.map_data[get_index(a.map, bx, by, bz)];
    g.xn = a.map_data[get_index(a.map, bx + 1, by, bz)];
    g.xl = a.map_data[get_index(a.map, bx - 1, by, bz)];
    g.yn = a.map_data[get_index(a.map, bx, by + 1, bz)];
    g.yl = a.map_data[get_index(a.map, bx, by - 1, bz)];
    g.zn = a.map_data[get_index(a.map, bx, by, bz + 1)];
    g.zl = a.map_data[get_index(a.map, bx, by, bz - 1)];
  }
  return g;
}

// The map's constants as the resident loop holds them: uniform values, but in VECTOR registers.  As kernel arguments they
// live in scalar registers, and the loop has more uniform state than scalar registers: the compiler spilled them to vector
// lanes and fetched them back (v_readlane + s_nop) in every iteration, and since a vector instruction takes at most one scalar
// operand it copied a further 28 of them into vector registers per point anyway.
struct LoopGather
{
  int32_t ringK[3]; // offset + size - pos: ring coordinate = ring(x + ringK, size)
  int32_t size[3];
  int32_t pos[3];
  uint32_t lim[3];  // size / 2 - 1: in_bounds_with_buffer_neg(buf, 1)
  uint32_t divM;    // division by the map resolution (FastDiv)
  int32_t divK;
};
__device__ __forceinline__ LoopGather make_loop_gather(const PointArgs &a)
{
  LoopGather c;
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    c.ringK[k] = wsub(wadd(a.map.offset[k], a.map.size[k]), a.map.pos[k]);
    c.size[k] = a.map.size[k];
    c.pos[k] = a.map.pos[k];
    c.lim[k] = (uint32_t)(a.map.size[k] / 2 - 1); // size >= 3 (ws_map_create)
    pin_vgpr(c.ringK[k]); pin_vgpr(c.size[k]); pin_vgpr(c.pos[k]); pin_vgpr(c.lim[k]);
  }
  c.divM = (uint32_t)a.resdiv.M; // < 2^32 (make_fastdiv)
  c.divK = a.resdiv.k;
  pin_vgpr(c.divM); pin_vgpr(c.divK);
  return c;
}
__device__ __forceinline__ int64_t loop_index(const LoopGather &c, int32_t x, int32_t y, int32_t z)
{
  // get_index (ws_device.h) with x - pos + offset + size folded into one constant per axis (the same bits: wrapping adds)
  const int32_t xi = ring(wadd(x, c.ringK[0]), c.size[0]), yi = ring(wadd(y, c.ringK[1]), c.size[1]), zi = ring(wadd(z, c.ringK[2]), c.size[2]);
  const int32_t row = xi * c.size[1] + yi;
  return (int64_t)row * (int64_t)c.size[2] + zi;
}
// gather_point<true> on those constants (same arithmetic, same results)
__device__ __forceinline__ Gathered gather_point_loop(const PointArgs &a, const LoopGather &c, const IntTransform &t, int32_t px, int32_t py, int32_t pz, bool valid,
                                                      VoxelCache &vc)
{
  Gathered g;
  int32_t qx = wadd(wadd(wadd(wmul(t.M[0], px), wmul(t.M[3], py)), wmul(t.M[6], pz)), t.M[9]) / MATRIX_RESOLUTION;
  int32_t qy = wadd(wadd(wadd(wmul(t.M[1], px), wmul(t.M[4], py)), wmul(t.M[7], pz)), t.M[10]) / MATRIX_RESOLUTION;
  int32_t qz = wadd(wadd(wadd(wmul(t.M[2], px), wmul(t.M[5], py)), wmul(t.M[8], pz)), t.M[11]) / MATRIX_RESOLUTION;
  const int32_t bx = div_trunc(qx, (uint64_t)c.divM, c.divK, 0), by = div_trunc(qy, (uint64_t)c.divM, c.divK, 0), bz = div_trunc(qz, (uint64_t)c.divM, c.divK, 0);
  g.qx = wsub(qx, t.cx);
  g.qy = wsub(qy, t.cy);
  g.qz = wsub(qz, t.cz);
  g.ok = valid && (uint32_t)iabs32(wsub(bx, c.pos[0])) <= c.lim[0] && (uint32_t)iabs32(wsub(by, c.pos[1])) <= c.lim[1] &&
         (uint32_t)iabs32(wsub(bz, c.pos[2])) <= c.lim[2];
  const bool refill = g.ok && !(vc.filled && vc.bx == bx && vc.by == by && vc.bz == bz);
  if (refill)
  {
    // Ring coordinates of the voxel and of its neighbours.  The voxel is in bounds with a margin of one, so x + ringK lies in
    // [0, 3 size): ring() as two conditional subtractions written as unsigned minima (v - size wraps to a huge number when
    // v < size), and a neighbour is the voxel's own ring coordinate +- 1 with one wrap -- 30 instructions instead of the
    // nine full ring() of seven loop_index calls (54); the same indices.
    uint32_t rc[3], rn[3], rl[3];
    const int32_t b3[3] = {bx, by, bz};
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      const uint32_t sz = (uint32_t)c.size[k];
      uint32_t v = (uint32_t)wadd(b3[k], c.ringK[k]);
      v = min(v, v - sz);
      v = min(v, v - sz);
      rc[k] = v;
      rn[k] = min(v + 1u, v + 1u - sz);      // v + 1 == size -> 0
      rl[k] = min(v - 1u, v - 1u + sz);      // v == 0 -> size - 1 (v - 1 wraps)
    }
    const uint32_t sy = (uint32_t)c.size[1], sz = (uint32_t)c.size[2];
    // (row * size_z + z as ONE v_mad_u64_u32: all three operands unsigned 32-bit, the index 64-bit for 2049^3)
    auto at = [&](uint32_t row, uint32_t z) { return a.map_data[(uint64_t)row * (uint64_t)sz + (uint64_t)z]; };
    const uint32_t row_c = rc[0] * sy + rc[1];
    vc.cur = at(row_c, rc[2]);
    vc.xn = at(rn[0] * sy + rc[1], rc[2]);
    vc.xl = at(rl[0] * sy + rc[1], rc[2]);
    vc.yn = at(rc[0] * sy + rn[1], rc[2]);
    vc.yl = at(rc[0] * sy + rl[1], rc[2]);
    vc.zn = at(row_c, rn[2]);
    vc.zl = at(row_c, rl[2]);
    vc.bx = bx;
    vc.by = by;
    vc.bz = bz;
    vc.filled = true;
  }
  const uint32_t keep = g.ok ? 0xffffffffu : 0u;
  g.cur = vc.cur & keep; g.xn = vc.xn & keep; g.xl = vc.xl & keep; g.yn = vc.yn & keep; g.yl = vc.yl & keep; g.zn = vc.zn & keep; g.zl = vc.zl & keep;
  return g;
}

// Both functions below are written without branches on purpose: nested `if`s over three gradients became nine exec-mask
// regions with a round trip through the scalar unit each (v_cmp -> SGPR -> s_and_saveexec -> s_cbranch), which cost more
// than the arithmetic they skipped; masks keep the whole point in the vector unit.
__device__ __forceinline__ int32_t central_gradient(uint32_t next, uint32_t last)
{
  // registration.cu:233-246: both neighbours observed and not of strictly opposite sign
  const int32_t nv = entry_value(next), lv = entry_value(last);
  const int32_t observed = ((next >> 16) != 0u) & ((last >> 16) != 0u);
  const int32_t opposite = (nv * lv) < 0; // 16-bit values: the product is negative iff the signs are strictly opposite
  const int32_t keep = -(observed & (opposite ^ 1));
  return ((nv - lv) / 2) & keep;
}

// J (registration.cu:224-250), the voxel's value and whether the point counts, all zero for a point that does not
__device__ __forceinline__ void point_terms(const Gathered &g, int32_t (&J)[6], int32_t &v, int32_t &used)
{
  // a point outside the map or in an unobserved voxel (registration.cu:217-222) contributes zeros
  used = (g.ok ? 1 : 0) & ((g.cur >> 16) != 0u);
  const int32_t keep = -used;
  const int32_t gx = central_gradient(g.xn, g.xl) & keep, gy = central_gradient(g.yn, g.yl) & keep, gz = central_gradient(g.zn, g.zl) & keep;
  // point.cross(gradient) in int (math/vector3.h:269-277); J = (cross, gradient) as long
  J[0] = wsub(wmul(g.qy, gz), wmul(g.qz, gy));
  J[1] = wsub(wmul(g.qz, gx), wmul(g.qx, gz));
  J[2] = wsub(wmul(g.qx, gy), wmul(g.qy, gx));
  J[3] = gx;
  J[4] = gy;
  J[5] = gz;
  v = entry_value(g.cur) & keep;
}

__device__ __forceinline__ void consume_point(const Gathered &g, int64_t (&acc)[REG_SLOTS])
{
  int32_t J[6], v, used;
  point_terms(g, J, v, used);
  // 21 unique terms of J J^T (registration.cu:55-97); int32 x int32 + int64 maps onto v_mad_i64_i32
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) acc[tri_index(i, j)] = wadd64(acc[tri_index(i, j)], (int64_t)J[i] * (int64_t)J[j]);
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] = wadd64(acc[21 + i], (int64_t)J[i] * (int64_t)v);
  acc[27] += (v < 0 ? -v : v);
  acc[28] += used;
}

// ---- the same sums on the matrix cores (resident loop, clouds of at most one point per lane) ---------------------------
// h = sum J J^T, g = sum J v, e = sum |v|, c = sum 1 are one Gram matrix A A^T over the points, and v_mfma_i32_32x32x32_i8
// computes exactly that -- in int32, exactly -- for rows of signed bytes.  A point's 32 rows are the bytes of 8 dwords:
//   d0..d5  J[0..5] ^ 0x00808080   limbs s0 s1 s2 s3 with J = s0 + 256 s1 + 65536 s2 + 2^24 s3 + 0x808080  (s3: the sign byte;
//           the three low bytes become SIGNED limbs by flipping their top bit, i.e. by carrying a bias of 128 each)
//   d6      (v ^ 0x80) | (n ^ 0x80) << 16   with n = -|v|: two limbs each (v, n in [-32768, 32767]), bias 128
//   d7      1 | used << 8                   a row of ones (what multiplies the biases) and the row that counts
// One instruction multiplies the 32 x 32 rows of 32 points; the SAME register is its A and its B operand (B[k][j] = A[j][k]),
// so whatever order the hardware gives the 32 points inside the operand, a row meets itself in the same order.  Lane (r, half)
// must supply row r of 16 points, while a point's rows are computed in ONE lane: the wave's 64 x 32 bytes pass through LDS,
// point-major as they are computed (two 128-bit writes per lane, points 48 bytes apart), and come back TRANSPOSED by the
// hardware: ds_read_b64_tr_b8 hands every lane of a 16-lane group one byte column of an 8-point x 16-byte block (tools/
// tr_probe.hip prints what it does), i.e. row r of 8 points per read -- four reads per wave, no byte shuffling in registers
// (the first version read [dword][point] with eight 128-bit reads and picked bytes with 24 v_perm_b32: +0.05 us).  Two
// matrix instructions per wave replace 27 v_mad_i64_i32 per lane AND the 190-instruction transposing butterfly: the K
// dimension of the product is the reduction over the lanes.  What comes out, per wave: C[a][b] = sum over its 64 points of limb a x limb b.  Lane (b, half) holds rows
// 8g + 4 half + t: the four limbs t of dword 2g + half, i.e. (Horner) the sum over the points of Js_i x (limb b % 4 of dword
// b / 4); shifted by 8 (b % 4) it goes straight into the workgroup's slot with an LDS atomic -- the 4 limb columns of a dword
// meet there.  The biases: sum (Js_i + B)(Js_j + B) = sum Js_i Js_j + B (T_i + T_j) + B^2 N with T_i = sum Js_i x 1 (the ones
// column) and N = sum 1 x 1, all from the same product; the first wave adds those terms once per iteration when it reads the
// slots (mfma_finalize).  Everything is integer arithmetic mod 2^64 like the int64 sums it replaces: bit-identical.
typedef int mf_v4i __attribute__((ext_vector_type(4)));
typedef int mf_v16i __attribute__((ext_vector_type(16)));
#ifndef WS_MF_POINT_STRIDE
#define WS_MF_POINT_STRIDE 12
#endif
constexpr int MF_POINT_STRIDE = WS_MF_POINT_STRIDE;  // words per staged point: 8 used, 48 bytes apart (128-bit writes without bank conflicts)
constexpr int MF_STAGE_WORDS = 64 * MF_POINT_STRIDE; // per wave
constexpr int MF_AUX = 8;                          // behind the 32 slots: T_0..T_5, sum vs, N
constexpr uint32_t MF_NONE = 0xffffffffu;
constexpr uint64_t MF_BJ = 0x00808080ull, MF_BV = 0x80ull;

struct MfLane // constants of a lane
{
  uint32_t rd;      // first staged word this lane reads
  uint32_t shift;   // 8 x (column limb)
  uint32_t slot[3]; // where the lane's values of g = 0, 1, 2 go (index into wg_sum[32 + MF_AUX]), MF_NONE: nowhere
  // first wave, lane -> slot (lane & 31): raw + ca * aux[ia] + cb * aux[ib] + cn * N
  uint32_t ia, ib;
  uint64_t ca, cb, cn;
};
__device__ __forceinline__ MfLane make_mf_lane()
{
  MfLane L;
  const int lane = threadIdx.x & 63, j = lane & 31, half = lane >> 5, jd = j >> 2, m = j & 3;
  // ds_read_b64_tr_b8: a 16-lane group reads a block of 8 points x 16 row bytes, every lane 8 contiguous bytes at its OWN
  // address (lane j of the group: point j / 2, bytes 8 (j % 2) .. of the 16-byte window), and gets back the block's column j:
  // the row byte (lane & 15) of the window for the 8 points.  Groups 0 / 1 take the windows of rows 0..15 / 16..31, the upper
  // half of the wave the points 16 further on.
  L.rd = (uint32_t)((16 * half + ((lane & 15) >> 1)) * MF_POINT_STRIDE * 4 + ((lane >> 4) & 1) * 16 + (lane & 1) * 8); // bytes
  L.shift = (uint32_t)(8 * m);
#pragma unroll
  for (int g = 0; g < 3; ++g)
  {
    const int i = 2 * g + half;
    uint32_t t = MF_NONE;
    if (jd < 6 && i <= jd)
      t = (uint32_t)tri_index(i, jd);
    else if (jd == 6 && m < 2)
      t = (uint32_t)(21 + i); // the value's two limbs as columns: g[i]
    else if (j == 28)
      t = (uint32_t)(REG_SLOTS + i); // the ones column: T_i
    L.slot[g] = t;
  }
  const int slot = lane & 31;
  L.ia = L.ib = 0;
  L.ca = L.cb = L.cn = 0;
  if (slot < 21)
  {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int jj = i; jj < 6; ++jj)
        if (tri_index(i, jj) == slot)
        {
          L.ia = (uint32_t)i;
          L.ib = (uint32_t)jj;
        }
    L.ca = L.cb = MF_BJ;
    L.cn = MF_BJ * MF_BJ;
  }
  else if (slot < 27)
  {
    L.ia = (uint32_t)(slot - 21);
    L.ib = 6; // sum vs
    L.ca = MF_BV;
    L.cb = MF_BJ;
    L.cn = MF_BJ * MF_BV;
  }
  else if (slot == 27)
    L.cn = MF_BV; // e = -(sum ns + 128 N)
  return L;
}

// one point per lane (all 64 lanes active; a lane without a point has g.ok == false): C += A A^T of the wave's 64 points
__device__ __forceinline__ void mfma_consume(const Gathered &g, mf_v16i &C, uint32_t *stage /* this wave's MF_STAGE_WORDS */, const MfLane &L)
{
  int32_t J[6], v, used;
  point_terms(g, J, v, used);
  const int lane = threadIdx.x & 63;
  const int32_t n = v < 0 ? v : -v;
  uint4 d0, d1;
  d0.x = (uint32_t)J[0] ^ (uint32_t)MF_BJ; d0.y = (uint32_t)J[1] ^ (uint32_t)MF_BJ; d0.z = (uint32_t)J[2] ^ (uint32_t)MF_BJ; d0.w = (uint32_t)J[3] ^ (uint32_t)MF_BJ;
  d1.x = (uint32_t)J[4] ^ (uint32_t)MF_BJ; d1.y = (uint32_t)J[5] ^ (uint32_t)MF_BJ;
  d1.z = (((uint32_t)v ^ (uint32_t)MF_BV) & 0xffffu) | (((uint32_t)n ^ (uint32_t)MF_BV) << 16);
  d1.w = 1u | ((uint32_t)used << 8);
  *reinterpret_cast<uint4 *>(&stage[lane * MF_POINT_STRIDE]) = d0;
  *reinterpret_cast<uint4 *>(&stage[lane * MF_POINT_STRIDE + 4]) = d1;
  __builtin_amdgcn_wave_barrier(); // (LDS serves a wave's accesses in order: the reads below see all 64 lanes' writes)
  typedef int mf_v2i __attribute__((ext_vector_type(2)));
  const char *base = reinterpret_cast<const char *>(stage) + L.rd;
#pragma unroll
  for (int q = 0; q < 2; ++q)
  {
    // the transposing read delivers the operand as the instruction wants it: row (lane & 31) of 8 points per read
    const mf_v2i lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) mf_v2i *)(base + (32 * q) * MF_POINT_STRIDE * 4));
    const mf_v2i hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) mf_v2i *)(base + (32 * q + 8) * MF_POINT_STRIDE * 4));
    mf_v4i a;
    a[0] = lo[0]; a[1] = lo[1]; a[2] = hi[0]; a[3] = hi[1];
    C = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, a, C, 0, 0, 0);
  }
  __builtin_amdgcn_wave_barrier(); // the next call's writes stay behind these reads
}

// the wave's product into the workgroup's slots (wg_sum[32 + MF_AUX], zero before the iteration)
__device__ __forceinline__ void mfma_flush(const mf_v16i &C, unsigned long long *wg_sum, const MfLane &L)
{
  const int lane = threadIdx.x & 63;
  int32_t lo[4], hi[4]; // |C| <= 2^14 x 64 points: the pairs fit 32 bits
#pragma unroll
  for (int g = 0; g < 4; ++g)
  {
    lo[g] = C[4 * g + 1] * 256 + C[4 * g + 0];
    hi[g] = C[4 * g + 3] * 256 + C[4 * g + 2];
  }
  // The four limb columns of a dword are four adjacent lanes and meet in the slot itself: 48 lanes on 12 addresses per
  // instruction.  (Summing them over the quad first -- two DPP stages, one lane adds -- is slower: 5.49 vs 5.38 us per iteration.)
#pragma unroll
  for (int g = 0; g < 3; ++g)
  {
    const int64_t P = (int64_t)hi[g] * 65536 + (int64_t)lo[g];
    if (L.slot[g] != MF_NONE) atomicAdd(&wg_sum[L.slot[g]], (unsigned long long)P << L.shift);
  }
  // rows 24..27 (lower half): the limbs of v and n; rows 28, 29 (upper half): ones and used -- against the ones column (28)
  if (lane == 28 || lane == 60)
  {
    const bool up = lane == 60;
    atomicAdd(&wg_sum[up ? REG_SLOTS + 7 : REG_SLOTS + 6], (unsigned long long)(int64_t)(up ? C[12] : lo[3])); // N : sum vs
    atomicAdd(&wg_sum[up ? 28 : 27], (unsigned long long)(int64_t)(up ? C[13] : hi[3]));                       // c : sum ns
  }
}

// first wave, after the barrier: the value of slot (lane & 31) with the bias terms added; leaves the slots zero
__device__ __forceinline__ unsigned long long mfma_finalize(unsigned long long *wg_sum, const MfLane &L)
{
  const int lane = threadIdx.x & 63, slot = lane & 31;
  const unsigned long long raw = wg_sum[slot], Ta = wg_sum[REG_SLOTS + L.ia], Tb = wg_sum[REG_SLOTS + L.ib], N = wg_sum[REG_SLOTS + 7];
  __builtin_amdgcn_wave_barrier();
  if (lane < REG_SLOTS) wg_sum[slot] = 0;
  if (lane < MF_AUX) wg_sum[REG_SLOTS + lane] = 0;
  unsigned long long s = raw + L.ca * Ta + L.cb * Tb + L.cn * N;
  if (slot == 27) s = 0ull - s;
  return s;
}

constexpr uint32_t REG_STRIDE = REG_BLOCKS * REG_THREADS; // points covered by one pass of the grid

// Which point a thread takes in pass u of the grid: the grid's WAVES in the order (wave-in-workgroup, workgroup), 64 consecutive
// points each.  A cloud (or a rank's shard) smaller than one pass then fills wave 0 of every workgroup before wave 1 of any:
// the points are spread over all compute units, and a workgroup's unused waves skip the accumulate and reduce phases, so the
// phase costs a 16 384-point shard (1 wave per workgroup) a third of what it costs the full cloud (8 waves, two per SIMD).
// With workgroup-major order the same shard filled 32 workgroups to the brim and left 224 idle: no gain from sharding at all.
__device__ __forceinline__ uint32_t point_slot() { return (((threadIdx.x >> 6) * gridDim.x + blockIdx.x) << 6) + (threadIdx.x & 63u); }

// raw coordinates of this lane's first two points, loaded before anything else in the kernel
struct Prefetched
{
  int32_t p[2][3];
  bool valid[2];
};
__device__ __forceinline__ Prefetched prefetch_points(const PointArgs &a, const uint32_t REG_STRIDE = ws::REG_STRIDE)
{
  Prefetched f;
#pragma unroll
  for (int u = 0; u < 2; ++u)
  {
    const uint32_t idx = a.first + point_slot() + (uint32_t)u * REG_STRIDE;
    f.valid[u] = idx < a.end;
    const size_t o = f.valid[u] ? 3 * (size_t)idx : 0;
    f.p[u][0] = f.valid[u] ? a.points[o + 0] : 0;
    f.p[u][1] = f.valid[u] ? a.points[o + 1] : 0;
    f.p[u][2] = f.valid[u] ? a.points[o + 2] : 0;
  }
  return f;
}

template <bool CACHED = false>
__device__ __forceinline__ void accumulate_points(const PointArgs &a, const float *T, const Prefetched &f, int64_t (&acc)[REG_SLOTS],
                                                  VoxelCache *cache = nullptr, const uint32_t REG_STRIDE = ws::REG_STRIDE)
{
  const IntTransform t = make_int_transform(T);
  // the two prefetched points: 14 gathers in flight before the first is consumed
  const Gathered g0 = gather_point<CACHED>(a, t, f.p[0][0], f.p[0][1], f.p[0][2], f.valid[0], CACHED ? &cache[0] : nullptr);
  if (__ballot(f.valid[1]) != 0ull) // a whole wave without a second point (cloud <= one pass of the grid) skips its arithmetic
  {
    const Gathered g1 = gather_point<CACHED>(a, t, f.p[1][0], f.p[1][1], f.p[1][2], f.valid[1], CACHED ? &cache[1] : nullptr);
    consume_point(g0, acc);
    consume_point(g1, acc);
  }
  else
    consume_point(g0, acc);
  // clouds larger than two passes of the grid (N > 131 072)
  for (uint32_t idx = a.first + point_slot() + 2 * REG_STRIDE; idx < a.end; idx += REG_STRIDE)
  {
    const Gathered g = gather_point(a, t, a.points[3 * (size_t)idx + 0], a.points[3 * (size_t)idx + 1], a.points[3 * (size_t)idx + 2], true);
    consume_point(g, acc);
  }
}

// One pass of a resident kernel (an iteration of the loop, a request to the server) over the points for the pose in T_sh / TI_sh:
// the workgroup's totals added into wg_sum (zero before; the caller's barrier follows).  MFMA: one point per lane, the sums on the
// matrix cores; else v_mad_i64_i32 and the transposing butterfly.  The voxel caches stay valid for as long as the map and the cloud
// do not change, which is the whole launch of either kernel.  mid(): between the sums and their flush into wg_sum (timing stamps).
template <bool MFMA, typename Mid>
__device__ __forceinline__ void pass_sums(const PointArgs &a, const LoopGather &lg, const Prefetched &f, uint32_t stride, const float *T_sh,
                                          const int32_t *TI_sh, VoxelCache (&cache)[2], uint32_t *mf_stage, const MfLane &mfl,
                                          unsigned long long *wg_sum, Mid mid)
{
  if (MFMA)
  {
    const IntTransform t = load_int_pose(TI_sh);
    const Gathered g0 = gather_point_loop(a, lg, t, f.p[0][0], f.p[0][1], f.p[0][2], f.valid[0], cache[0]);
    mf_v16i C;
#pragma unroll
    for (int i = 0; i < 16; ++i) C[i] = 0;
    mfma_consume(g0, C, mf_stage + (threadIdx.x >> 6) * MF_STAGE_WORDS, mfl);
    mid();
    mfma_flush(C, wg_sum, mfl);
  }
  else
  {
    float T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = T_sh[i];
    int64_t acc[REG_SLOTS];
#pragma unroll
    for (int t = 0; t < REG_SLOTS; ++t) acc[t] = 0;
    accumulate_points<true>(a, T, f, acc, cache, stride);
    mid();
    wave_reduce32_add(acc, wg_sum);
  }
}

inline PointArgs make_point_args(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t first, size_t count)
{
  size_t end = first + count;
  if (end > r->n) end = r->n;
  if (flags & WS_REG_COMPAT_REFERENCE_LAUNCH)
  {
    // <<<128,512>>> covers points 0..65535 only; the reduction drops the last N % 32 points for N >= 128
    size_t lim = r->n;
    if (lim > 65536) lim = 65536;
    if (r->n >= 128)
    {
      size_t red = 32 * (r->n / 32);
      if (red < lim) lim = red;
    }
    if (end > lim) end = lim;
  }
  if (first > end) first = end;
  PointArgs p;
  p.points = r->points.as<int32_t>();
  p.first = (uint32_t)first;
  p.end = (uint32_t)end;
  p.map_data = m->data[WS_MAP_AVG].as<uint32_t>();
  p.map = m->par[WS_MAP_AVG];
  p.resdiv = make_fastdiv(res);
  return p;
}

} // namespace ws
