// store_frontier.hip — the frontier of the chunk store (ws_store_frontier, include/warpsense_hip.h): the ordered stream compaction of
// store_surface.hip over the 64^3 chunks of the global map in device memory with the 7-point rule of ws_frontier.h, in the output order
// of ws_map_frontier, across chunk borders.  The word space is that of the store's mesh and surface cloud (ws_store_words.h): one
// (x, y) column of a listed chunk is one 64-voxel word, and the word index t ascends exactly like the output order.  Only the chunks
// the call lists have words: 4096 per chunk, 8 bytes of scratch each.  A neighbour across a chunk face is read through the call's
// table of face neighbours; a missing neighbour chunk inside the box is UNKNOWN, a neighbour outside the box is not looked at.
//
//   store_frontier_count_kernel    chunk order, one wave per four chunk columns, lane = z: the ballot of "frontier voxel" is the word's
//                                  mask at t.  Only a lane whose voxel is FREE reads its six neighbours
//   store_frontier_totals_kernel   word order: the masks' popcounts per 256 consecutive words
//   store_frontier_scan_kernel     exclusive scan of those totals (one workgroup; 64-bit offsets, the last element is the total)
//   store_frontier_emit_kernel     word order, 256 consecutive words per workgroup: a block scan of the popcounts places every word; a
//                                  wave takes its 64 words one after the other, skips zero masks, finds the chunk (StoreWord::find),
//                                  and a lane of a set bit forms its record's mask again and writes the record to (workgroup base +
//                                  words before + set bits below the lane)
//
// Plain launches on the context's stream, nothing waits for another workgroup, no atomics.  The clustering of the records is
// frontier_clusters (map_frontier.hip).
#include "ws_frontier.h"
#include "ws_mesh.h" // block_scan_256, popc_below
#include "ws_store_words.h"

namespace ws
{
constexpr uint32_t SFR_WORDS = 256; // words per workgroup of the word passes (one per thread)

struct StoreFrArgs : StoreWords
{
  int32_t min_value;
  uint32_t any_weight;
  int32_t lo[3], hi[3];  // the box, inclusive world voxels
  const uint32_t *nb;    // [n_chunks][6] list position of the chunk at -x +x -y +y -z +z, SM_NONE: not listed
  mu64 *mask;            // [n_words]
  uint32_t *blk_tot;     // [n_words / 256]
  const mu64 *blk_off;   // [n_words / 256] exclusive scan of blk_tot
  su32x4 *rec;           // x, y, z, mask
  mu64 cap;              // records the output buffer holds
};

// The mask of the FREE voxel (l[0], l[1], l[2]) of listed chunk i, whose words are at `chunk` and whose world coordinates are p.  The
// voxel lies in the box: a neighbour is outside the box iff the voxel lies on that face (no coordinate is formed that could overflow)
__device__ __forceinline__ uint32_t store_fr_mask(const StoreFrArgs &a, uint32_t i, const uint32_t *chunk, const int32_t l[3], const int32_t p[3])
{
  const bool any_weight = a.any_weight != 0;
  uint32_t mask = 0u;
#pragma unroll
  for (int d = 0; d < 6; ++d)
  {
    const int axis = d >> 1;
    const bool up = d & 1;
    if (p[axis] == (up ? a.hi[axis] : a.lo[axis])) continue; // outside the box: neither known nor unknown
    int32_t n[3] = {l[0], l[1], l[2]};
    n[axis] += up ? 1 : -1;
    const uint32_t *src = chunk;
    if (n[axis] < 0 || n[axis] >= STORE_CS)
    {
      const uint32_t j = a.nb[(size_t)i * 6u + (uint32_t)d];
      if (j == SM_NONE) // an absent chunk inside the box
      {
        mask |= 1u << d;
        continue;
      }
      src = sm_chunk(a, j);
      n[axis] &= STORE_CS - 1;
    }
    if (fr_unknown(src[n[0] * (STORE_CS * STORE_CS) + n[1] * STORE_CS + n[2]], any_weight)) mask |= 1u << d;
  }
  return mask;
}

// ---- pass 1: the chunks, once.  A workgroup takes 16 columns of one x plane of a chunk, a wave four of them (the shape of
// store_surface_count_kernel)
__global__ __launch_bounds__(256) void store_frontier_count_kernel(StoreFrArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x >> 8, lx = (blockIdx.x >> 2) & 63u, ly0 = (blockIdx.x & 3u) * 16u + (uint32_t)wave * 4u;
  if (i >= a.n_chunks) return;
  const su32x4 g = a.grp[i];
  const mi32x4 k = a.key[i];
  const uint32_t *chunk = sm_chunk(a, i);
  const uint32_t *column = chunk + (lx * (uint32_t)(STORE_CS * STORE_CS) + ly0 * (uint32_t)STORE_CS);
  const int32_t x = k.x * STORE_CS + (int32_t)lx, y0 = k.y * STORE_CS + (int32_t)ly0, z = k.z * STORE_CS + lane;
  const bool in_xz = x >= a.lo[0] && x <= a.hi[0] && z >= a.lo[2] && z <= a.hi[2];
  const uint32_t t0 = sm_word(g, i, lx, ly0);
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    uint32_t raw = 0u; // outside the box: weight 0, not free
    if (in_xz && y0 + j >= a.lo[1] && y0 + j <= a.hi[1]) raw = __builtin_nontemporal_load(column + j * STORE_CS + lane);
    bool q = false;
    if (fr_free(raw, a.any_weight != 0, a.min_value))
    {
      const int32_t l[3] = {(int32_t)lx, (int32_t)ly0 + j, lane}, p[3] = {x, y0 + j, z};
      q = store_fr_mask(a, i, chunk, l, p) != 0u;
    }
    const mu64 b = __ballot(q);
    if (lane == j) a.mask[t0 + (uint32_t)j * g.w] = b;
  }
}

// ---- pass 1b: frontier voxels per workgroup of the emit pass (n_words is a multiple of 4096: every thread has a word)
__global__ __launch_bounds__(256) void store_frontier_totals_kernel(StoreFrArgs a)
{
  uint32_t c = (uint32_t)__popcll(a.mask[blockIdx.x * SFR_WORDS + threadIdx.x]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
  __shared__ uint32_t wtot[4];
  if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) a.blk_tot[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

// ---- pass 2
__global__ __launch_bounds__(1024) void store_frontier_scan_kernel(const uint32_t *tot, mu64 *off, uint32_t n, mu64 *total)
{
  scan_block_totals(tot, off, n, total);
}

// ---- pass 3: the records, in word order
__global__ __launch_bounds__(256) void store_frontier_emit_kernel(StoreFrArgs a)
{
  __shared__ mu64 sM[SFR_WORDS];
  __shared__ uint32_t sB[SFR_WORDS];
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * SFR_WORDS;
  const mu64 Mt = a.mask[t0 + threadIdx.x];
  sM[threadIdx.x] = Mt;
  sB[threadIdx.x] = block_scan_256((uint32_t)__popcll(Mt), wsum);
  __syncthreads();
  const mu64 base = a.blk_off[blockIdx.x];
  for (int w = 0; w < 64; ++w) // the wave's 64 words, one after the other; lane = z inside the word
  {
    const int idx = wave * 64 + w;
    const mu64 M = sM[idx];
    if (M == 0ull) continue; // (most words hold no frontier; the same for the whole wave)
    StoreWord p;
    p.find(a, t0 + (uint32_t)idx);
    if (!((M >> lane) & 1ull)) continue;
    const mu64 o = base + sB[idx] + popc_below(M, lane);
    if (o >= a.cap) continue; // (the count pass sized the buffer; a store that changed in between must not write beyond it)
    const mi32x4 k = a.key[p.i];
    const int32_t l[3] = {(int32_t)p.lx, (int32_t)p.ly, lane};
    const int32_t q[3] = {k.x * STORE_CS + l[0], k.y * STORE_CS + l[1], k.z * STORE_CS + l[2]};
    fr_put_record(a.rec, o, q[0], q[1], q[2], store_fr_mask(a, p.i, sm_chunk(a, p.i), l, q));
  }
}

// ---- host side: the workgroups of the emit pass are those of the surface cloud (store_surface_blocks)
static uint32_t store_fr_blocks(uint32_t n_chunks) { return n_chunks * (4096u / SFR_WORDS); }

static StoreFrArgs store_fr_args(const ws_store *st, const ws_store::Frontier &q, const StoreFrontierCall &c, size_t cap)
{
  StoreFrArgs a;
  const char *tab = static_cast<const char *>(q.table_dev.p);
  store_words_bind(a, st, tab, c.n_chunks);
  a.nb = reinterpret_cast<const uint32_t *>(tab + store_word_table_bytes(c.n_chunks));
  a.min_value = c.min_value;
  a.any_weight = (c.flags & WS_FRONTIER_ANY_WEIGHT) ? 1u : 0u;
  for (int k = 0; k < 3; ++k) a.lo[k] = c.lo[k], a.hi[k] = c.hi[k];
  a.mask = static_cast<mu64 *>(q.mask.p);
  a.blk_tot = static_cast<uint32_t *>(q.blk_tot.p);
  a.blk_off = static_cast<const mu64 *>(q.blk_off.p);
  a.rec = static_cast<su32x4 *>(q.rec.p);
  a.cap = cap;
  return a;
}

// the tables' upload, then passes 1 and 2; the total arrives in q.total.host (pinned) once the stream has been synchronised
int launch_store_frontier_count(ws_store *st, ws_store::Frontier &q, const StoreFrontierCall &c)
{
  hipStream_t s = st->ctx->stream;
  WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_frontier_table_bytes(c.n_chunks), hipMemcpyHostToDevice, s));
  const StoreFrArgs a = store_fr_args(st, q, c, 0);
  const uint32_t blocks = store_fr_blocks(c.n_chunks);
  q.timer.mark(0, s);
  hipLaunchKernelGGL(store_frontier_count_kernel, dim3(c.n_chunks * 256u), dim3(256), 0, s, a);
  hipLaunchKernelGGL(store_frontier_totals_kernel, dim3(blocks), dim3(256), 0, s, a);
  q.timer.mark(1, s);
  hipLaunchKernelGGL(store_frontier_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)a.blk_tot, static_cast<mu64 *>(q.blk_off.p), blocks, q.total.dev);
  q.timer.mark(2, s);
  WS_HIP(hipGetLastError());
  return q.total.fetch(s);
}

// pass 3: no record at or beyond `cap` is written
int launch_store_frontier_emit(ws_store *st, ws_store::Frontier &q, const StoreFrontierCall &c, size_t cap)
{
  const StoreFrArgs a = store_fr_args(st, q, c, cap);
  hipStream_t s = st->ctx->stream;
  q.timer.mark(3, s);
  hipLaunchKernelGGL(store_frontier_emit_kernel, dim3(store_fr_blocks(c.n_chunks)), dim3(256), 0, s, a);
  q.timer.mark(4, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
