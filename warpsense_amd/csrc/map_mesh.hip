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
#include "ws_mesh.h"

namespace ws
{
// the word-level rules (bits, active cells, quads, vertices, faces) are in ws_mesh.h, shared with store_mesh.hip; here a word index
// is t = column of the box * nw + w, and the neighbouring words lie at fixed distances
struct MeshArgs : MeshBuffers
{
  BoxArgs box;
  uint32_t nw, n_words; // words per column, box.n_cols * nw (< 2^31)
  int32_t res;
  uint32_t any_weight;
};

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
      mu64 bv, bi;
      mesh_ballots(raw[j], a.any_weight, bv, bi);
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
    mu64 v[4], i[4], vn[4], in[4]; // of the four corner columns; *n: the next word
#pragma unroll
    for (int c = 0; c < 4; ++c)
    {
      const uint32_t tt = t + ((c >> 1) * (uint32_t)a.box.ey + (c & 1)) * a.nw;
      v[c] = a.valid[tt], i[c] = a.inside[tt];
      vn[c] = more ? a.valid[tt + 1] : 0ull, in[c] = more ? a.inside[tt + 1] : 0ull;
    }
    A = mesh_active_cells(v, i, vn, in);
  }
  a.act[t] = A;
}

__device__ __forceinline__ void quad_words(const MeshArgs &a, uint32_t t, uint32_t w, int32_t x, int32_t y, mu64 Ac, QuadWords &o)
{
  const uint32_t dy = a.nw, dx = (uint32_t)a.box.ey * a.nw;
  const bool hx = x > 0, hy = y > 0, hw = w > 0;
  const mu64 A[4] = {Ac, hy ? a.act[t - dy] : 0ull, hx ? a.act[t - dx] : 0ull, hx && hy ? a.act[t - dx - dy] : 0ull};
  const mu64 below[3] = {hw ? a.act[t - 1] : 0ull, hw && hy ? a.act[t - dy - 1] : 0ull, hw && hx ? a.act[t - dx - 1] : 0ull};
  // Ac != 0: the columns x + 1 and y + 1 are in the box
  mesh_quad_masks(o, A, below, a.inside[t], a.inside[t + dx], a.inside[t + dy], w + 1 < a.nw ? a.inside[t + 1] : 0ull);
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
      nq = mesh_quad_count(q);
    }
    a.qcnt[t] = (uint8_t)nq;
  }
  mesh_block_totals(nv, nq, a.vtot, a.qtot);
}

// ---- exclusive scans of the workgroup totals: workgroup 0 the vertices, workgroup 1 the quads; every thread a contiguous piece
__global__ __launch_bounds__(1024) void mesh_scan_kernel(MeshArgs a, uint32_t n)
{
  scan_block_totals(blockIdx.x ? a.qtot : a.vtot, blockIdx.x ? a.qoff : a.voff, n, a.totals + blockIdx.x);
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
    uint32_t raw[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) // k = dx * 4 + dy * 2 + dz
    {
      const int32_t xi = (k & 4) ? xi1 : xi0, yi = (k & 2) ? yi1 : yi0, zi = (k & 1) ? zi1 : zi0;
      raw[k] = a.box.data[(int64_t)(xi * sy + yi) * (int64_t)sz + zi];
    }
    if (out < a.vcap) // (the count pass sized the buffer; a map that changed in between must not write beyond it)
    {
      const int32_t c3[3] = {x, y, a.box.lo[2] + z};
      a.vert[out] = mesh_vertex(raw, c3, a.res);
    }
  }
}

// ---- pass 3b: faces
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
    if (!(((q.q[0] | q.q[1] | q.q[2]) >> lane) & 1ull)) continue;
    const uint32_t vb[4] = {a.vbase[tt], y > 0 ? a.vbase[tt - dy] : 0u, x > 0 ? a.vbase[tt - dx] : 0u, x > 0 && y > 0 ? a.vbase[tt - dx - dy] : 0u};
    mesh_emit_quads(q, lane, vb, sF[idx], a.face, a.qcap);
  }
}

// ---- host side
size_t mesh_scratch_bytes(uint64_t n_words)
{
  const size_t nwd = (size_t)n_words, nb = mesh_blocks((uint32_t)n_words);
  return 3 * mesh_up256(nwd * 8) + mesh_up256(nwd * 4) + mesh_up256(nwd) + 2 * mesh_up256(nb * 4) + 2 * mesh_up256(nb * 8) + 256;
}

static MeshArgs mesh_args(const ws_map *m, const MeshResult &q, int which, const int32_t lo[3], const int32_t ext[3], uint32_t flags, bool emit)
{
  MeshArgs a;
  a.box = box_args(m, which, lo, ext);
  a.nw = (uint32_t)((ext[2] + 63) / 64);
  a.n_words = a.box.n_cols * a.nw;
  a.res = m->res;
  a.any_weight = (flags & WS_MESH_ANY_WEIGHT) ? 1u : 0u;
  mesh_bind(a, q, a.n_words, emit);
  return a;
}

int launch_mesh_count(ws_map *m, MeshResult &q, int which, const int32_t lo[3], const int32_t ext[3], uint32_t flags)
{
  const MeshArgs a = mesh_args(m, q, which, lo, ext, flags, false);
  return mesh_launch_count(q, m->ctx->stream, a, (a.box.n_cols + 3) / 4, mesh_bits_kernel, mesh_cells_kernel, mesh_quads_kernel, mesh_scan_kernel);
}

int launch_mesh_emit(ws_map *m, MeshResult &q, int which, const int32_t lo[3], const int32_t ext[3], uint32_t flags)
{
  return mesh_launch_emit(q, m->ctx->stream, mesh_args(m, q, which, lo, ext, flags, true), mesh_vertex_kernel, mesh_face_kernel);
}

} // namespace ws
