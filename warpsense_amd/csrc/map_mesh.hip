// map_mesh.hip — a triangle mesh of a device map (gfx950) by naive surface nets: one vertex per cell the surface passes through,
// one quad (two triangles) per lattice edge that crosses the surface.  The rules are stated in include/warpsense_hip.h at
// ws_map_mesh; everything is integer, and vertices and faces leave in a fixed order (cells / owner voxels ascending, z fastest), so
// the output bytes are a function of the map alone.
//
// The map is read densely ONCE.  What the neighbourhood tests need of a voxel is two bits (valid, inside), so the first pass turns
// every (x, y) voxel column of the box into bit words in world z order, and the neighbourhood work is 64 cells per 64-bit operation:
//
//   mesh_bits_kernel     one wave per voxel column, lane = world z: valid / inside as ballots        -> valid[t], inside[t]
//   mesh_cells_kernel    one thread per word t = (column, 64 z): the active cells of the cell column  -> act[t]
//   mesh_quads_kernel    one thread per word: the crossing edges whose four cells are active (three masks, counted) -> qcnt[t];
//                        per workgroup of 256 words the number of vertices and quads
//   mesh_scan_kernel     exclusive scans of the two workgroup totals (one workgroup each; the last elements are the totals)
//   mesh_vertex_kernel   per workgroup a scan of popcount(act) -> vbase[t] (index of the word's first vertex); the active cells gather
//                        their eight corners from the map (sparse: the surface is a few per cent of the cells) and write a vertex
//   mesh_face_kernel     per workgroup a scan of qcnt; a quad's four vertex indices are vbase of the cell's word plus a popcount
//
// A word index t = column * nw + w ascends exactly like the output order (column = x * ey + y of the box, then z), so ONE flat scan
// gives every position: no per-column bases, no atomics, nothing waits for another workgroup.  Voxel columns, cell columns and
// owner-voxel columns share the index: the cell column of (x, y) is the one whose lowest corner column is (x, y); it has no cells
// for x = ex - 1 or y = ey - 1, and act is zero there.
// Scratch: valid, inside, act (one bit each), vbase (32 bits per 64 voxels), qcnt (8 bits per 64): 29 bytes per 64 voxels of the box,
// plus 24 bytes per 256 words.
#include "ws_device.h"

namespace ws
{
typedef unsigned long long mu64;
typedef uint32_t mu32x2 __attribute__((ext_vector_type(2)));
typedef int32_t mi32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t MESH_WORDS = 256; // words per workgroup of the word passes (one per thread)

struct MeshArgs
{
  BoxArgs box;
  uint32_t nw, n_words; // words per column, box.n_cols * nw (< 2^31)
  int32_t res;
  uint32_t any_weight;
  mu64 *valid, *inside, *act; // [n_words]
  uint32_t *vbase;            // [n_words]
  uint8_t *qcnt;              // [n_words] quads owned by the word's voxels (<= 192)
  uint32_t *vtot, *qtot;      // [workgroups]
  mu64 *voff, *qoff;          // [workgroups] exclusive scans
  mu64 *totals;               // vertices, quads
  mi32x4 *vert;               // x_mm, y_mm, z_mm, weight
  uint32_t *face;             // 3 indices per triangle
  mu64 vcap, qcap;            // vertices / quads the output buffers hold
};

__device__ __forceinline__ mu64 shift_down(mu64 cur, mu64 next) { return (cur >> 1) | (next << 63); } // bit z := bit z + 1
__device__ __forceinline__ uint32_t popc_below(mu64 mask, int lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); }

// ---- pass 1: the map, once
__global__ __launch_bounds__(256) void mesh_bits_kernel(MeshArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t col = blockIdx.x * 4u + (uint32_t)wave;
  if (col >= a.box.n_cols) return; // (the same for the whole wave; no barrier in this kernel)
  int32_t x, y, zs0;
  const uint32_t *column = a.box.data + box_column(a.box, col, x, y, zs0);
  const int32_t sz = a.box.mp.size[2];
  mu64 *vout = a.valid + (size_t)col * a.nw, *iout = a.inside + (size_t)col * a.nw;
  for (uint32_t w0 = 0; w0 < a.nw; w0 += 4)
  {
    // four loads in flight per lane, each 256 contiguous bytes per wave (two pieces where the ring seam falls into it)
    uint32_t raw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const int32_t z = (int32_t)(w0 + j) * 64 + lane;
      raw[j] = 0u; // weight 0: not valid; value 0: not inside
      if (z < a.box.ez)
      {
        int32_t zs = zs0 + z; // < 2 sz
        if (zs >= sz) zs -= sz;
        raw[j] = __builtin_nontemporal_load(column + zs);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const int32_t wt = entry_weight(raw[j]);
      const mu64 bv = __ballot(a.any_weight ? wt != 0 : wt > 0), bi = __ballot(entry_value(raw[j]) < 0);
      if (lane == j && w0 + j < a.nw)
      {
        vout[w0 + j] = bv;
        iout[w0 + j] = bi;
      }
    }
  }
}

// ---- pass 2: active cells, 64 per thread
__global__ __launch_bounds__(256) void mesh_cells_kernel(MeshArgs a)
{
  const uint32_t t = blockIdx.x * MESH_WORDS + threadIdx.x;
  if (t >= a.n_words) return;
  const uint32_t col = t / a.nw, w = t - col * a.nw;
  const int32_t x = (int32_t)(col / (uint32_t)a.box.ey), y = (int32_t)(col - (uint32_t)x * (uint32_t)a.box.ey);
  mu64 A = 0;
  if (x + 1 < a.box.ex && y + 1 < a.box.ey)
  {
    const bool more = w + 1 < a.nw;
    mu64 V = ~0ull, any = 0, all = ~0ull, Vn = ~0ull, anyn = 0, alln = ~0ull; // of the four corner columns; *n: the next word
#pragma unroll
    for (int c = 0; c < 4; ++c)
    {
      const uint32_t tt = t + ((c >> 1) * (uint32_t)a.box.ey + (c & 1)) * a.nw;
      const mu64 v = a.valid[tt], i = a.inside[tt];
      const mu64 vn = more ? a.valid[tt + 1] : 0ull, in = more ? a.inside[tt + 1] : 0ull;
      V &= v, any |= i, all &= i;
      Vn &= vn, anyn |= in, alln &= in;
    }
    // cell z: voxels z and z + 1 of the four columns (no valid bit at z >= ez: the column's last voxel starts no cell)
    const mu64 cv = V & shift_down(V, Vn), ca = any | shift_down(any, anyn), cl = all & shift_down(all, alln);
    A = cv & ca & ~cl;
  }
  a.act[t] = A;
}

// the quads owned by the voxels of word t (column c = (x, y), 64 z from 64 w): an edge from voxel a along axis k that crosses the
// surface, and whose four cells are active (a valid cell at a crossing edge is active, an active cell is valid with valid corners)
struct QuadWords
{
  mu64 q[3];  // per axis
  mu64 A[4];  // active cells of the cell columns c, c - (0,1), c - (1,0), c - (1,1)
  mu64 I;     // inside bits of the voxel column
};
__device__ __forceinline__ void quad_words(const MeshArgs &a, uint32_t t, uint32_t w, int32_t x, int32_t y, mu64 Ac, QuadWords &o)
{
  const uint32_t dy = a.nw, dx = (uint32_t)a.box.ey * a.nw;
  const bool hx = x > 0, hy = y > 0, hw = w > 0;
  o.A[0] = Ac;
  o.A[1] = hy ? a.act[t - dy] : 0ull;
  o.A[2] = hx ? a.act[t - dx] : 0ull;
  o.A[3] = hx && hy ? a.act[t - dx - dy] : 0ull;
  // the cells one below: bit z = cell z - 1
  const mu64 m0 = (o.A[0] << 1) | (hw ? a.act[t - 1] >> 63 : 0ull);
  const mu64 m1 = (o.A[1] << 1) | (hw && hy ? a.act[t - dy - 1] >> 63 : 0ull);
  const mu64 m2 = (o.A[2] << 1) | (hw && hx ? a.act[t - dx - 1] >> 63 : 0ull);
  // Ac != 0: the columns x + 1 and y + 1 are in the box
  const mu64 I = a.inside[t], Ix = a.inside[t + dx], Iy = a.inside[t + dy], In = w + 1 < a.nw ? a.inside[t + 1] : 0ull;
  o.I = I;
  o.q[0] = (I ^ Ix) & o.A[0] & o.A[1] & m0 & m1;                  // cells (x, y-1, z-1) (x, y, z-1) (x, y, z) (x, y-1, z)
  o.q[1] = (I ^ Iy) & o.A[0] & o.A[2] & m0 & m2;                  // cells (x-1, y, z-1) (x-1, y, z) (x, y, z) (x, y, z-1)
  o.q[2] = (I ^ shift_down(I, In)) & o.A[0] & o.A[1] & o.A[2] & o.A[3]; // cells (x-1, y-1, z) (x, y-1, z) (x, y, z) (x-1, y, z)
}

__global__ __launch_bounds__(256) void mesh_quads_kernel(MeshArgs a)
{
  const uint32_t t = blockIdx.x * MESH_WORDS + threadIdx.x;
  uint32_t nv = 0, nq = 0;
  if (t < a.n_words)
  {
    const mu64 Ac = a.act[t];
    if (Ac)
    {
      const uint32_t col = t / a.nw, w = t - col * a.nw;
      const int32_t x = (int32_t)(col / (uint32_t)a.box.ey), y = (int32_t)(col - (uint32_t)x * (uint32_t)a.box.ey);
      QuadWords q;
      quad_words(a, t, w, x, y, Ac, q);
      nv = (uint32_t)__popcll(Ac);
      nq = (uint32_t)(__popcll(q.q[0]) + __popcll(q.q[1]) + __popcll(q.q[2]));
    }
    a.qcnt[t] = (uint8_t)nq;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
  {
    nv += __shfl_xor(nv, d, 64);
    nq += __shfl_xor(nq, d, 64);
  }
  __shared__ uint32_t wv[4], wq[4];
  if ((threadIdx.x & 63) == 0)
  {
    wv[threadIdx.x >> 6] = nv;
    wq[threadIdx.x >> 6] = nq;
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    a.vtot[blockIdx.x] = wv[0] + wv[1] + wv[2] + wv[3];
    a.qtot[blockIdx.x] = wq[0] + wq[1] + wq[2] + wq[3];
  }
}

// ---- exclusive scans of the workgroup totals: workgroup 0 the vertices, workgroup 1 the quads; every thread a contiguous piece
__global__ __launch_bounds__(1024) void mesh_scan_kernel(MeshArgs a, uint32_t n)
{
  scan_block_totals(blockIdx.x ? a.qtot : a.vtot, blockIdx.x ? a.qoff : a.voff, n, a.totals + blockIdx.x);
}

// exclusive scan of one value per thread over the workgroup (256 threads)
__device__ __forceinline__ uint32_t block_scan_256(uint32_t c, uint32_t *wsum /* [4] shared */)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t pre = 0;
  for (int k = 0; k < wave; ++k) pre += wsum[k];
  return pre + inc - c;
}

// offset of the crossing from voxel a towards b, in mm: (2 |va| res + m) / (2 m), m = |va| + |vb| >= 1 (floor of non-negative
// numbers below 2^53: one double division is exact, ws_device.h)
__device__ __forceinline__ int64_t crossing(int32_t va, int32_t vb, int32_t res)
{
  const int64_t ua = va < 0 ? -(int64_t)va : (int64_t)va, ub = vb < 0 ? -(int64_t)vb : (int64_t)vb, m = ua + ub;
  return div_trunc_i64(2 * ua * (int64_t)res + m, 2 * m);
}

// ---- pass 3a: vertices
__global__ __launch_bounds__(256) void mesh_vertex_kernel(MeshArgs a)
{
  __shared__ mu64 sA[MESH_WORDS];
  __shared__ uint32_t sB[MESH_WORDS];
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * MESH_WORDS, t = t0 + threadIdx.x;
  const mu64 At = t < a.n_words ? a.act[t] : 0ull;
  const uint32_t c = (uint32_t)__popcll(At);
  const uint32_t base = (uint32_t)a.voff[blockIdx.x] + block_scan_256(c, wsum); // (the host launches this only if the total fits 32 bits)
  if (t < a.n_words) a.vbase[t] = base;
  sA[threadIdx.x] = At;
  sB[threadIdx.x] = base;
  __syncthreads();
  const int32_t sz = a.box.mp.size[2], sy = a.box.mp.size[1];
  const int32_t res = a.res;
  for (int i = 0; i < 64; ++i) // the wave's 64 words, one after the other; lane = z inside the word
  {
    const int idx = wave * 64 + i;
    const mu64 A = sA[idx];
    if (!((A >> lane) & 1ull)) continue; // (most words have no active cell)
    const uint32_t tt = t0 + (uint32_t)idx, col = tt / a.nw, w = tt - col * a.nw;
    const int32_t z = (int32_t)w * 64 + lane;
    const mu64 out = (mu64)sB[idx] + popc_below(A, lane);
    // the eight corners: storage columns of x, x + 1 and y, y + 1, storage z of z and z + 1 (each one step along the ring)
    int32_t x, y, xi0, yi0, zs0; // x, y: of the world
    box_column_xy(a.box, col, x, y, xi0, yi0, zs0);
    const int32_t xi1 = xi0 + 1 == a.box.mp.size[0] ? 0 : xi0 + 1, yi1 = yi0 + 1 == sy ? 0 : yi0 + 1;
    int32_t zi0 = zs0 + z;
    if (zi0 >= sz) zi0 -= sz;
    const int32_t zi1 = zi0 + 1 == sz ? 0 : zi0 + 1;
    int32_t v[8];
    uint32_t wmin = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < 8; ++k) // k = dx * 4 + dy * 2 + dz
    {
      const int32_t xi = (k & 4) ? xi1 : xi0, yi = (k & 2) ? yi1 : yi0, zi = (k & 1) ? zi1 : zi0;
      const uint32_t raw = a.box.data[(int64_t)(xi * sy + yi) * (int64_t)sz + zi];
      v[k] = entry_value(raw);
      wmin = min(wmin, (uint32_t)iabs32(entry_weight(raw))); // (weights are positive unless WS_MESH_ANY_WEIGHT admits negative ones)
    }
    // the crossing edges: four per axis, from the corner without the axis' bit to the one with it
    int64_t s[3] = {0, 0, 0};
    int32_t n = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
    {
      const int bit = 4 >> ax;
#pragma unroll
      for (int k = 0; k < 8; ++k)
      {
        if (k & bit) continue;
        const int32_t va = v[k], vb = v[k | bit];
        if ((va < 0) == (vb < 0)) continue;
        ++n;
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] += d == ax ? crossing(va, vb, res) : ((k & (4 >> d)) ? (int64_t)res : 0);
      }
    }
    if (out < a.vcap) // (the count pass sized the buffer; a map that changed in between must not write beyond it)
    {
      const int32_t c3[3] = {x, y, a.box.lo[2] + z};
      int32_t p[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) p[d] = c3[d] * res + res / 2 + (int32_t)div_trunc_i64(s[d], n > 0 ? n : 1); // fits: the host checked the box
      const mi32x4 r = {p[0], p[1], p[2], (int32_t)wmin};
      a.vert[out] = r;
    }
  }
}

// ---- pass 3b: faces
__device__ __forceinline__ void put_quad(const MeshArgs &a, mu64 quad, uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, bool inside)
{
  if (quad >= a.qcap) return;
  mu32x2 *f = reinterpret_cast<mu32x2 *>(a.face + quad * 6ull); // 24 bytes per quad: 8-byte aligned
  const uint32_t b = inside ? q1 : q2, c = inside ? q2 : q1, d = inside ? q2 : q3, e = inside ? q3 : q2;
  const mu32x2 f0 = {q0, b}, f1 = {c, q0}, f2 = {d, e};
  f[0] = f0; // (q0, q1, q2) (q0, q2, q3) if a is inside, else (q0, q2, q1) (q0, q3, q2)
  f[1] = f1;
  f[2] = f2;
}

__global__ __launch_bounds__(256) void mesh_face_kernel(MeshArgs a)
{
  __shared__ uint32_t sQ[MESH_WORDS];
  __shared__ mu64 sF[MESH_WORDS];
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * MESH_WORDS, t = t0 + threadIdx.x;
  const uint32_t c = t < a.n_words ? a.qcnt[t] : 0u;
  const uint32_t pre = block_scan_256(c, wsum);
  sQ[threadIdx.x] = c;
  sF[threadIdx.x] = a.qoff[blockIdx.x] + pre;
  __syncthreads();
  const uint32_t dy = a.nw, dx = (uint32_t)a.box.ey * a.nw;
  for (int i = 0; i < 64; ++i)
  {
    const int idx = wave * 64 + i;
    if (sQ[idx] == 0u) continue; // (the same for the whole wave)
    const uint32_t tt = t0 + (uint32_t)idx, col = tt / a.nw, w = tt - col * a.nw;
    const int32_t x = (int32_t)(col / (uint32_t)a.box.ey), y = (int32_t)(col - (uint32_t)x * (uint32_t)a.box.ey);
    QuadWords q;
    quad_words(a, tt, w, x, y, a.act[tt], q);
    const bool k0 = (q.q[0] >> lane) & 1ull, k1 = (q.q[1] >> lane) & 1ull, k2 = (q.q[2] >> lane) & 1ull;
    if (!(k0 || k1 || k2)) continue;
    // index of cell z of a column: the word's first vertex plus the active cells below; of cell z - 1 (active): one less
    const uint32_t r0 = a.vbase[tt] + popc_below(q.A[0], lane);
    const uint32_t r1 = y > 0 ? a.vbase[tt - dy] + popc_below(q.A[1], lane) : 0u;
    const uint32_t r2 = x > 0 ? a.vbase[tt - dx] + popc_below(q.A[2], lane) : 0u;
    const uint32_t r3 = x > 0 && y > 0 ? a.vbase[tt - dx - dy] + popc_below(q.A[3], lane) : 0u;
    const bool in = (q.I >> lane) & 1ull;
    mu64 o = sF[idx] + popc_below(q.q[0], lane) + popc_below(q.q[1], lane) + popc_below(q.q[2], lane);
    if (k0) put_quad(a, o++, r1 - 1u, r0 - 1u, r0, r1, in);
    if (k1) put_quad(a, o++, r2 - 1u, r2, r0, r0 - 1u, in);
    if (k2) put_quad(a, o++, r3, r1, r0, r2, in);
  }
}

// ---- host side
static uint32_t mesh_blocks(uint32_t n_words) { return (n_words + MESH_WORDS - 1) / MESH_WORDS; }
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t mesh_scratch_bytes(uint64_t n_words)
{
  const size_t nwd = (size_t)n_words, nb = mesh_blocks((uint32_t)n_words);
  return 3 * up256(nwd * 8) + up256(nwd * 4) + up256(nwd) + 2 * up256(nb * 4) + 2 * up256(nb * 8) + 256;
}

static MeshArgs mesh_args(const ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], uint32_t flags, mu64 vcap, mu64 qcap)
{
  MeshArgs a;
  a.box = box_args(m, which, lo, ext);
  a.nw = (uint32_t)((ext[2] + 63) / 64);
  a.n_words = a.box.n_cols * a.nw;
  a.res = m->res;
  a.any_weight = (flags & WS_MESH_ANY_WEIGHT) ? 1u : 0u;
  const size_t nwd = a.n_words, nb = mesh_blocks(a.n_words);
  char *p = static_cast<char *>(m->mesh.scratch.p);
  auto take = [&p](size_t bytes) {
    char *r = p;
    p += up256(bytes);
    return r;
  };
  a.valid = reinterpret_cast<mu64 *>(take(nwd * 8));
  a.inside = reinterpret_cast<mu64 *>(take(nwd * 8));
  a.act = reinterpret_cast<mu64 *>(take(nwd * 8));
  a.vbase = reinterpret_cast<uint32_t *>(take(nwd * 4));
  a.qcnt = reinterpret_cast<uint8_t *>(take(nwd));
  a.vtot = reinterpret_cast<uint32_t *>(take(nb * 4));
  a.qtot = reinterpret_cast<uint32_t *>(take(nb * 4));
  a.voff = reinterpret_cast<mu64 *>(take(nb * 8));
  a.qoff = reinterpret_cast<mu64 *>(take(nb * 8));
  a.totals = reinterpret_cast<mu64 *>(take(16));
  a.vert = static_cast<mi32x4 *>(m->mesh.vert.p);
  a.face = static_cast<uint32_t *>(m->mesh.face.p);
  a.vcap = vcap;
  a.qcap = qcap;
  return a;
}

// bits, cells, quads and the scans; the two totals arrive in m->mesh.total.host (pinned) once the stream has been synchronised
int launch_mesh_count(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], uint32_t flags)
{
  const MeshArgs a = mesh_args(m, which, lo, ext, flags, 0, 0);
  const uint32_t blocks = mesh_blocks(a.n_words);
  hipStream_t s = m->ctx->stream;
  QueryTimer &t = m->mesh.timer;
  t.mark(0, s);
  hipLaunchKernelGGL(mesh_bits_kernel, dim3((a.box.n_cols + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(mesh_cells_kernel, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(mesh_quads_kernel, dim3(blocks), dim3(256), 0, s, a);
  t.mark(1, s);
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(2), dim3(1024), 0, s, a, blocks);
  t.mark(2, s);
  WS_HIP(hipGetLastError());
  return m->mesh.total.fetch(s, 2, a.totals);
}

// vertices, then faces (which read the vertex pass's vbase)
int launch_mesh_emit(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], uint32_t flags)
{
  const MeshArgs a = mesh_args(m, which, lo, ext, flags, m->mesh.vert.cap, m->mesh.face.cap / 2);
  const uint32_t blocks = mesh_blocks(a.n_words);
  hipStream_t s = m->ctx->stream;
  m->mesh.timer.mark(3, s);
  hipLaunchKernelGGL(mesh_vertex_kernel, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(mesh_face_kernel, dim3(blocks), dim3(256), 0, s, a);
  m->mesh.timer.mark(4, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
