// ws_mesh.h — the word-level rules of the surface-nets mesh (stated in include/warpsense_hip.h at ws_map_mesh), shared by the mesh of a
// window (map_mesh.hip) and the mesh of the chunk store (store_mesh.hip).  Both turn every (x, y) voxel column into 64-bit words of
// valid / inside bits in world z order, index the words so that the index ascends like the output order, and run the same six
// passes over them.  What differs is what a word index means and where a neighbouring word lies; everything that decides a bit, a
// vertex or a face is here, once, and takes the words (or the eight corner entries) as values.
#pragma once

#include "ws_device.h"

namespace ws
{
typedef unsigned long long mu64;
typedef uint32_t mu32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t MESH_WORDS = 256; // words per workgroup of the word passes (one per thread)

// the scratch of the passes and the two outputs: 29 bytes per word, plus 24 bytes per 256 words (mesh_scratch_bytes, map_mesh.hip)
struct MeshBuffers
{
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

inline uint32_t mesh_blocks(uint32_t n_words) { return (n_words + MESH_WORDS - 1) / MESH_WORDS; }
inline size_t mesh_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the scratch pointers of `n_words` words inside one allocation of mesh_scratch_bytes(n_words)
inline void mesh_take_scratch(MeshBuffers &a, void *scratch, size_t n_words)
{
  const size_t nb = mesh_blocks((uint32_t)n_words);
  char *p = static_cast<char *>(scratch);
  auto take = [&p](size_t bytes) {
    char *r = p;
    p += mesh_up256(bytes);
    return r;
  };
  a.valid = reinterpret_cast<mu64 *>(take(n_words * 8));
  a.inside = reinterpret_cast<mu64 *>(take(n_words * 8));
  a.act = reinterpret_cast<mu64 *>(take(n_words * 8));
  a.vbase = reinterpret_cast<uint32_t *>(take(n_words * 4));
  a.qcnt = reinterpret_cast<uint8_t *>(take(n_words));
  a.vtot = reinterpret_cast<uint32_t *>(take(nb * 4));
  a.qtot = reinterpret_cast<uint32_t *>(take(nb * 4));
  a.voff = reinterpret_cast<mu64 *>(take(nb * 8));
  a.qoff = reinterpret_cast<mu64 *>(take(nb * 8));
  a.totals = reinterpret_cast<mu64 *>(take(16));
}

// the scratch of `n_words` words and the outputs of a result holder.  The count passes write no output and are given no capacity
inline void mesh_bind(MeshBuffers &a, const MeshResult &q, size_t n_words, bool emit)
{
  mesh_take_scratch(a, q.scratch.p, n_words);
  a.vert = static_cast<mi32x4 *>(q.vert.p);
  a.face = static_cast<uint32_t *>(q.face.p);
  a.vcap = emit ? q.vert.cap : 0;
  a.qcap = emit ? q.face.cap / 2 : 0;
}

// The two launch sequences, whatever a word index means: `Args` is the including file's MeshBuffers with n_words, the kernels are its six.
// bits, cells, quads and the scans; the two totals arrive in q.total.host (pinned) once the stream has been synchronised
template <typename Args>
int mesh_launch_count(MeshResult &q, hipStream_t s, const Args &a, uint32_t bits_blocks, void (*bits)(Args), void (*cells)(Args), void (*quads)(Args),
                      void (*scan)(Args, uint32_t))
{
  const uint32_t blocks = mesh_blocks(a.n_words);
  q.timer.mark(0, s);
  hipLaunchKernelGGL(bits, dim3(bits_blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cells, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(quads, dim3(blocks), dim3(256), 0, s, a);
  q.timer.mark(1, s);
  hipLaunchKernelGGL(scan, dim3(2), dim3(1024), 0, s, a, blocks);
  q.timer.mark(2, s);
  WS_HIP(hipGetLastError());
  return q.total.fetch(s, 2, a.totals);
}
// vertices, then faces (which read the vertex pass's vbase)
template <typename Args> int mesh_launch_emit(MeshResult &q, hipStream_t s, const Args &a, void (*vertex)(Args), void (*face)(Args))
{
  const uint32_t blocks = mesh_blocks(a.n_words);
  q.timer.mark(3, s);
  hipLaunchKernelGGL(vertex, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(face, dim3(blocks), dim3(256), 0, s, a);
  q.timer.mark(4, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

__device__ __forceinline__ mu64 shift_down(mu64 cur, mu64 next) { return (cur >> 1) | (next << 63); } // bit z := bit z + 1
__device__ __forceinline__ uint32_t popc_below(mu64 mask, int lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); }

// ---- pass 1: the two bits of a voxel, as ballots over a wave whose lanes are 64 consecutive z (raw 0: not valid, not inside)
__device__ __forceinline__ void mesh_ballots(uint32_t raw, uint32_t any_weight, mu64 &valid, mu64 &inside)
{
  const int32_t wt = entry_weight(raw);
  valid = __ballot(any_weight ? wt != 0 : wt > 0);
  inside = __ballot(entry_value(raw) < 0);
}

// ---- pass 2: the active cells of a cell column from the words of its four corner columns (x, y) (x, y+1) (x+1, y) (x+1, y+1);
// *n: the next word up of the same column, zero where there is none
__device__ __forceinline__ mu64 mesh_active_cells(const mu64 v[4], const mu64 i[4], const mu64 vn[4], const mu64 in[4])
{
  mu64 V = ~0ull, any = 0, all = ~0ull, Vn = ~0ull, anyn = 0, alln = ~0ull;
#pragma unroll
  for (int c = 0; c < 4; ++c)
  {
    V &= v[c], any |= i[c], all &= i[c];
    Vn &= vn[c], anyn |= in[c], alln &= in[c];
  }
  // cell z: voxels z and z + 1 of the four columns (no valid bit beyond the last voxel: the column's last voxel starts no cell)
  const mu64 cv = V & shift_down(V, Vn), ca = any | shift_down(any, anyn), cl = all & shift_down(all, alln);
  return cv & ca & ~cl;
}

// the quads owned by the voxels of a word (column c = (x, y), 64 z): an edge from voxel a along axis k that crosses the surface, and
// whose four cells are active (a valid cell at a crossing edge is active, an active cell is valid with valid corners)
struct QuadWords
{
  mu64 q[3];  // per axis
  mu64 A[4];  // active cells of the cell columns c, c - (0,1), c - (1,0), c - (1,1)
  mu64 I;     // inside bits of the voxel column
};
// A: as QuadWords::A (zero where there is no such column); below[k]: the active cells of the word under A[k], k < 3 (zero where
// there is none); I, Ix, Iy: the inside bits of the column and of its +x and +y neighbours; In: of the word above I
__device__ __forceinline__ void mesh_quad_masks(QuadWords &o, const mu64 A[4], const mu64 below[3], mu64 I, mu64 Ix, mu64 Iy, mu64 In)
{
#pragma unroll
  for (int k = 0; k < 4; ++k) o.A[k] = A[k];
  // the cells one below: bit z = cell z - 1
  const mu64 m0 = (A[0] << 1) | (below[0] >> 63), m1 = (A[1] << 1) | (below[1] >> 63), m2 = (A[2] << 1) | (below[2] >> 63);
  o.I = I;
  o.q[0] = (I ^ Ix) & A[0] & A[1] & m0 & m1;                   // cells (x, y-1, z-1) (x, y, z-1) (x, y, z) (x, y-1, z)
  o.q[1] = (I ^ Iy) & A[0] & A[2] & m0 & m2;                   // cells (x-1, y, z-1) (x-1, y, z) (x, y, z) (x, y, z-1)
  o.q[2] = (I ^ shift_down(I, In)) & A[0] & A[1] & A[2] & A[3]; // cells (x-1, y-1, z) (x, y-1, z) (x, y, z) (x-1, y, z)
}
__device__ __forceinline__ uint32_t mesh_quad_count(const QuadWords &q) { return (uint32_t)(__popcll(q.q[0]) + __popcll(q.q[1]) + __popcll(q.q[2])); }

// ---- pass 3: a workgroup's (256 threads) numbers of vertices and quads
__device__ __forceinline__ void mesh_block_totals(uint32_t nv, uint32_t nq, uint32_t *vtot, uint32_t *qtot)
{
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
    vtot[blockIdx.x] = wv[0] + wv[1] + wv[2] + wv[3];
    qtot[blockIdx.x] = wq[0] + wq[1] + wq[2] + wq[3];
  }
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

// ---- the vertex of an active cell c3 from its eight corner entries, k = dx * 4 + dy * 2 + dz
__device__ __forceinline__ mi32x4 mesh_vertex(const uint32_t raw[8], const int32_t c3[3], int32_t res)
{
  int32_t v[8];
  uint32_t wmin = 0xffffffffu;
#pragma unroll
  for (int k = 0; k < 8; ++k)
  {
    v[k] = entry_value(raw[k]);
    wmin = min(wmin, (uint32_t)iabs32(entry_weight(raw[k]))); // (weights are positive unless WS_MESH_ANY_WEIGHT admits negative ones)
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
  int32_t p[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) p[d] = c3[d] * res + res / 2 + (int32_t)div_trunc_i64(s[d], n > 0 ? n : 1); // fits: the host checked the box
  const mi32x4 r = {p[0], p[1], p[2], (int32_t)wmin};
  return r;
}

// ---- faces
__device__ __forceinline__ void put_quad(uint32_t *face, mu64 qcap, mu64 quad, uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, bool inside)
{
  if (quad >= qcap) return;
  mu32x2 *f = reinterpret_cast<mu32x2 *>(face + quad * 6ull); // 24 bytes per quad: 8-byte aligned
  const uint32_t b = inside ? q1 : q2, c = inside ? q2 : q1, d = inside ? q2 : q3, e = inside ? q3 : q2;
  const mu32x2 f0 = {q0, b}, f1 = {c, q0}, f2 = {d, e};
  f[0] = f0; // (q0, q1, q2) (q0, q2, q3) if a is inside, else (q0, q2, q1) (q0, q3, q2)
  f[1] = f1;
  f[2] = f2;
}

// the quads of voxel `lane` of a word.  vb[k]: index of the first vertex of the word of cell column k (as QuadWords::A; anything
// where that column does not exist: its A is zero and no quad refers to it); first: index of the word's first quad
__device__ __forceinline__ void mesh_emit_quads(const QuadWords &q, int lane, const uint32_t vb[4], mu64 first, uint32_t *face, mu64 qcap)
{
  const bool k0 = (q.q[0] >> lane) & 1ull, k1 = (q.q[1] >> lane) & 1ull, k2 = (q.q[2] >> lane) & 1ull;
  if (!(k0 || k1 || k2)) return;
  // index of cell z of a column: the word's first vertex plus the active cells below; of cell z - 1 (active): one less
  const uint32_t r0 = vb[0] + popc_below(q.A[0], lane), r1 = vb[1] + popc_below(q.A[1], lane);
  const uint32_t r2 = vb[2] + popc_below(q.A[2], lane), r3 = vb[3] + popc_below(q.A[3], lane);
  const bool in = (q.I >> lane) & 1ull;
  mu64 o = first + popc_below(q.q[0], lane) + popc_below(q.q[1], lane) + popc_below(q.q[2], lane);
  if (k0) put_quad(face, qcap, o++, r1 - 1u, r0 - 1u, r0, r1, in);
  if (k1) put_quad(face, qcap, o++, r2 - 1u, r2, r0, r0 - 1u, in);
  if (k2) put_quad(face, qcap, o++, r3, r1, r0, r2, in);
}

} // namespace ws
