// store_mesh.hip — the mesh of the chunk store (ws_store_mesh, include/warpsense_hip.h): the surface nets of map_mesh.hip over the
// 64^3 chunks of the global map in device memory, in the output order of ws_map_mesh, across chunk borders.  The rules of a bit, a
// vertex and a face are those of ws_mesh.h; what is new is the SPARSE word space.
//
// A chunk is 64 voxels tall and z is fastest, so one (x, y) column of a chunk is exactly one 64-bit word and one aligned 256-byte
// load; there is no ring and no seam.  Only the chunks the call lists -- the present chunks the box overlaps, ascending (cx, cy, cz),
// known to the host before anything is launched -- have words: 4096 per chunk, 29 bytes of scratch each, whatever box they span.
//
// World order of the word (chunk (cx, cy, cz), lx, ly) is the lexicographic order of (cx, lx, cy, ly, cz) = (x, y, cz).  With, over the
// listed chunks, N = those that share cx and B those with a smaller cx, n = those that share (cx, cy) and P those of the same cx with
// a smaller cy, r = those of the same (cx, cy) with a smaller cz, the word's index is
//
//     t = 4096 B + lx 64 N + 64 P + ly n + r
//
// and ascends exactly like the output order, so the ONE flat scan of map_mesh.hip places every vertex and face.  The list is sorted,
// so chunk i has r = i - B - P, and the way back needs no search: the chunk at list position t / 4096 has the word's cx (the words of
// one cx are 4096 N consecutive indices from 4096 B), which gives B, N and lx; the chunk at position B + v / 64 of the remainder v
// has the word's (cx, cy), which gives P, n, ly and r (StoreWord::find, in ws_store_words.h: the store's surface cloud walks the same
// word space).
//
//   store_mesh_bits_kernel     one wave per four chunk columns, lane = z: the words of the listed chunks, bits outside the box cleared
//   store_mesh_cells_kernel    |
//   store_mesh_quads_kernel    |  one thread per word, the passes of map_mesh.hip; a neighbouring word beyond lx, ly = 0 / 63 or the
//   store_mesh_scan_kernel     |  word's z end is found through the chunk's neighbour entries (list positions, NONE where the
//   store_mesh_vertex_kernel   |  neighbour is absent or not listed: a zero word); the vertex pass gathers the eight corners from up
//   store_mesh_face_kernel     |  to eight chunks through the segment table
//
// Tables per call (the host's, store_mesh_tables in api_store_query.hip): per listed chunk {B, N, P, n}, {cx, cy, cz, slot} and 27 neighbour
// entries (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1), of which the passes use (0,0,0), the seven of {0,1}^3 and the seven of {0,-1}^3.
#include "ws_mesh.h"
#include "ws_store_words.h"

namespace ws
{
struct StoreMeshArgs : MeshBuffers, StoreWords
{
  int32_t res;
  uint32_t any_weight;
  int32_t lo[3], hi[3];       // the box, inclusive world voxels
  const uint32_t *nb;         // [n_chunks][27] list position of the neighbour chunk, or SM_NONE
};

__device__ __forceinline__ mu64 sm_load(const mu64 *words, uint32_t t) { return t == SM_NONE ? 0ull : words[t]; }

// ---- pass 1: the chunks, once.  A workgroup takes 16 columns of one x plane of a chunk, a wave four of them: four aligned 256-byte
// loads in flight per lane, one contiguous kilobyte per wave
__global__ __launch_bounds__(256) void store_mesh_bits_kernel(StoreMeshArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x >> 8, lx = (blockIdx.x >> 2) & 63u, ly0 = (blockIdx.x & 3u) * 16u + (uint32_t)wave * 4u;
  if (i >= a.n_chunks) return;
  const su32x4 g = a.grp[i];
  const mi32x4 k = a.key[i];
  const uint32_t *column = sm_chunk(a, i) + (lx * (uint32_t)(STORE_CS * STORE_CS) + ly0 * (uint32_t)STORE_CS);
  const int32_t x = k.x * STORE_CS + (int32_t)lx, y0 = k.y * STORE_CS + (int32_t)ly0, z = k.z * STORE_CS + lane;
  const bool in_xz = x >= a.lo[0] && x <= a.hi[0] && z >= a.lo[2] && z <= a.hi[2];
  uint32_t raw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    raw[j] = 0u; // outside the box: not valid, not inside
    if (in_xz && y0 + j >= a.lo[1] && y0 + j <= a.hi[1]) raw[j] = __builtin_nontemporal_load(column + j * STORE_CS + lane);
  }
  const uint32_t t0 = sm_word(g, i, lx, ly0);
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    mu64 bv, bi;
    mesh_ballots(raw[j], a.any_weight, bv, bi);
    if (lane == j)
    {
      a.valid[t0 + (uint32_t)j * g.w] = bv;
      a.inside[t0 + (uint32_t)j * g.w] = bi;
    }
  }
}

// ---- pass 2: active cells, 64 per thread
__global__ __launch_bounds__(256) void store_mesh_cells_kernel(StoreMeshArgs a)
{
  const uint32_t t = blockIdx.x * MESH_WORDS + threadIdx.x;
  if (t >= a.n_words) return;
  StoreWord p;
  p.find(a, t);
  mu64 v[4], i[4], vn[4], in[4]; // of the four corner columns; *n: the word of the chunk above
#pragma unroll
  for (int c = 0; c < 4; ++c)
  {
    const uint32_t tt = c ? p.at(a, c >> 1, c & 1, 0) : t, tn = p.at(a, c >> 1, c & 1, 1);
    v[c] = sm_load(a.valid, tt), i[c] = sm_load(a.inside, tt);
    vn[c] = sm_load(a.valid, tn), in[c] = sm_load(a.inside, tn);
  }
  a.act[t] = mesh_active_cells(v, i, vn, in);
}

// the word indices the quads of word p (index t) are made of
struct StoreQuadAt
{
  uint32_t c[4]; // the cell columns c, c - (0,1), c - (1,0), c - (1,1)
};
__device__ __forceinline__ void store_quad_words(const StoreMeshArgs &a, const StoreWord &p, uint32_t t, mu64 Ac, QuadWords &o, StoreQuadAt &at)
{
  at.c[0] = t, at.c[1] = p.at(a, 0, -1, 0), at.c[2] = p.at(a, -1, 0, 0), at.c[3] = p.at(a, -1, -1, 0);
  const mu64 A[4] = {Ac, sm_load(a.act, at.c[1]), sm_load(a.act, at.c[2]), sm_load(a.act, at.c[3])};
  const mu64 below[3] = {sm_load(a.act, p.at(a, 0, 0, -1)), sm_load(a.act, p.at(a, 0, -1, -1)), sm_load(a.act, p.at(a, -1, 0, -1))};
  mesh_quad_masks(o, A, below, a.inside[t], sm_load(a.inside, p.at(a, 1, 0, 0)), sm_load(a.inside, p.at(a, 0, 1, 0)), sm_load(a.inside, p.at(a, 0, 0, 1)));
}

__global__ __launch_bounds__(256) void store_mesh_quads_kernel(StoreMeshArgs a)
{
  const uint32_t t = blockIdx.x * MESH_WORDS + threadIdx.x;
  uint32_t nv = 0, nq = 0;
  if (t < a.n_words)
  {
    const mu64 Ac = a.act[t];
    if (Ac)
    {
      StoreWord p;
      p.find(a, t);
      QuadWords q;
      StoreQuadAt at;
      store_quad_words(a, p, t, Ac, q, at);
      nv = (uint32_t)__popcll(Ac);
      nq = mesh_quad_count(q);
    }
    a.qcnt[t] = (uint8_t)nq;
  }
  mesh_block_totals(nv, nq, a.vtot, a.qtot);
}

__global__ __launch_bounds__(1024) void store_mesh_scan_kernel(StoreMeshArgs a, uint32_t n)
{
  scan_block_totals(blockIdx.x ? a.qtot : a.vtot, blockIdx.x ? a.qoff : a.voff, n, a.totals + blockIdx.x);
}

// ---- pass 3a: vertices
__global__ __launch_bounds__(256) void store_mesh_vertex_kernel(StoreMeshArgs a)
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
  for (int w = 0; w < 64; ++w) // the wave's 64 words, one after the other; lane = z inside the word
  {
    const int idx = wave * 64 + w;
    const mu64 A = sA[idx];
    if (A == 0ull) continue; // (most words have no active cell; the same for the whole wave)
    StoreWord p;
    p.find(a, t0 + (uint32_t)idx);
    const mi32x4 k = a.key[p.i];
    // the eight corners: columns lx, lx + 1 and ly, ly + 1, each in its chunk and in the chunk above it (lane 63's upper corners).
    // An active cell has eight valid corners, which lie in present chunks; a missing chunk reads as entry 0 all the same.
    uint32_t raw[8];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
    {
      const int nx = (int)p.lx + (cc >> 1), ny = (int)p.ly + (cc & 1);
      const uint32_t code = (uint32_t)(((nx >> 6) + 1) * 9 + ((ny >> 6) + 1) * 3 + 1);
      const uint32_t j0 = cc && code != 13u ? a.nb[(size_t)p.i * 27u + code] : p.i, j1 = a.nb[(size_t)p.i * 27u + code + 1u];
      const uint32_t off = (uint32_t)(nx & 63) * (uint32_t)(STORE_CS * STORE_CS) + (uint32_t)(ny & 63) * (uint32_t)STORE_CS;
#pragma unroll
      for (int dz = 0; dz < 2; ++dz)
      {
        const int zz = lane + dz;
        const uint32_t j = zz < STORE_CS ? j0 : j1;
        uint32_t r = 0u;
        if (((A >> lane) & 1ull) && j != SM_NONE) r = sm_chunk(a, j)[off + (uint32_t)(zz & 63)];
        raw[cc * 2 + dz] = r;
      }
    }
    if (!((A >> lane) & 1ull)) continue;
    const mu64 out = (mu64)sB[idx] + popc_below(A, lane);
    if (out < a.vcap) // (the count pass sized the buffer; a store that changed in between must not write beyond it)
    {
      const int32_t c3[3] = {k.x * STORE_CS + (int32_t)p.lx, k.y * STORE_CS + (int32_t)p.ly, k.z * STORE_CS + lane};
      a.vert[out] = mesh_vertex(raw, c3, a.res);
    }
  }
}

// ---- pass 3b: faces
__global__ __launch_bounds__(256) void store_mesh_face_kernel(StoreMeshArgs a)
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
  for (int w = 0; w < 64; ++w)
  {
    const int idx = wave * 64 + w;
    if (sQ[idx] == 0u) continue; // (the same for the whole wave)
    const uint32_t tt = t0 + (uint32_t)idx;
    StoreWord p;
    p.find(a, tt);
    QuadWords q;
    StoreQuadAt at;
    store_quad_words(a, p, tt, a.act[tt], q, at);
    if (!(((q.q[0] | q.q[1] | q.q[2]) >> lane) & 1ull)) continue;
    uint32_t vb[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) vb[kk] = at.c[kk] == SM_NONE ? 0u : a.vbase[at.c[kk]];
    mesh_emit_quads(q, lane, vb, sF[idx], a.face, a.qcap);
  }
}

// ---- host side
size_t store_mesh_table_bytes(size_t n_chunks) { return store_word_table_bytes(n_chunks) + n_chunks * 27 * 4; }

static StoreMeshArgs store_mesh_args(const ws_store *st, const ws_store::Mesh &q, const StoreMeshCall &c, bool emit)
{
  StoreMeshArgs a;
  a.res = c.res;
  a.any_weight = (c.flags & WS_MESH_ANY_WEIGHT) ? 1u : 0u;
  for (int k = 0; k < 3; ++k) a.lo[k] = c.lo[k], a.hi[k] = c.hi[k];
  const char *tab = static_cast<const char *>(q.table_dev.p);
  store_words_bind(a, st, tab, c.n_chunks);
  a.nb = reinterpret_cast<const uint32_t *>(tab + store_word_table_bytes(c.n_chunks));
  mesh_bind(a, q, a.n_words, emit);
  return a;
}

// the tables' upload, then the count passes
int launch_store_mesh_count(ws_store *st, ws_store::Mesh &q, const StoreMeshCall &c)
{
  hipStream_t s = st->ctx->stream;
  WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_mesh_table_bytes(c.n_chunks), hipMemcpyHostToDevice, s));
  return mesh_launch_count(q, s, store_mesh_args(st, q, c, false), c.n_chunks * 256u, store_mesh_bits_kernel, store_mesh_cells_kernel,
                           store_mesh_quads_kernel, store_mesh_scan_kernel);
}

int launch_store_mesh_emit(ws_store *st, ws_store::Mesh &q, const StoreMeshCall &c)
{
  return mesh_launch_emit(q, st->ctx->stream, store_mesh_args(st, q, c, true), store_mesh_vertex_kernel, store_mesh_face_kernel);
}

} // namespace ws
