// store_surface.hip — the surface cloud of the chunk store (ws_store_surface, include/warpsense_hip.h): the ordered stream compaction
// of map_surface.hip over the 64^3 chunks of the global map in device memory, in the output order of ws_map_surface, across chunk
// borders.  Which voxel qualifies, its record and its marker are the rules of ws_surface.h; the word space is that of the store's mesh
// (ws_store_words.h): one (x, y) column of a listed chunk is one 64-voxel word and one aligned 256-byte load, and the word index t
// ascends exactly like the output order.  Only the chunks the call lists have words: 4096 per chunk, 8 bytes of scratch each.
//
//   store_surface_count_kernel    chunk order, one wave per four chunk columns, lane = z: the ballot of the predicate, bits outside
//                                 the box cleared, is the word's mask at t
//   store_surface_totals_kernel   word order: the masks' popcounts per 256 consecutive words
//   store_surface_scan_kernel     exclusive scan of those totals (one workgroup; 64-bit offsets, the last element is the total)
//   store_surface_emit_kernel     word order, 256 consecutive words per workgroup: a block scan of the popcounts places every word; a
//                                 wave takes its 64 words one after the other, skips zero masks -- an empty column is never read
//                                 again --, finds the chunk (StoreWord::find), loads the column, and a lane writes its record to
//                                 (workgroup base + words before + set bits below the lane)
//
// Plain launches on the context's stream, nothing waits for another workgroup, no atomics.
#include "ws_mesh.h" // block_scan_256, popc_below
#include "ws_store_words.h"
#include "ws_surface.h"

namespace ws
{
constexpr uint32_t SSURF_WORDS = 256; // words per workgroup of the word passes (one per thread)

struct StoreSurfArgs : StoreWords
{
  int32_t band, tau, res;
  int32_t lo[3], hi[3];  // the box, inclusive world voxels
  mu64 *mask;            // [n_words]
  uint32_t *blk_tot;     // [n_words / 256]
  const mu64 *blk_off;   // [n_words / 256] exclusive scan of blk_tot
  su32x4 *rec;           // x, y, z, raw
  float *marker;         // 7 floats per record: x y z (metres) r g b a
  mu64 cap;              // records the output buffers hold
};

// ---- pass 1: the chunks, once.  A workgroup takes 16 columns of one x plane of a chunk, a wave four of them: four aligned 256-byte
// loads in flight per lane, one contiguous kilobyte per wave (the shape of store_mesh_bits_kernel)
__global__ __launch_bounds__(256) void store_surface_count_kernel(StoreSurfArgs a)
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
    raw[j] = 0u; // outside the box: weight 0, does not qualify
    if (in_xz && y0 + j >= a.lo[1] && y0 + j <= a.hi[1]) raw[j] = __builtin_nontemporal_load(column + j * STORE_CS + lane);
  }
  const uint32_t t0 = sm_word(g, i, lx, ly0);
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    const mu64 q = __ballot(surf_pred(raw[j], a.band));
    if (lane == j) a.mask[t0 + (uint32_t)j * g.w] = q;
  }
}

// ---- pass 1b: qualifying voxels per workgroup of the emit pass (n_words is a multiple of 4096: every thread has a word)
__global__ __launch_bounds__(256) void store_surface_totals_kernel(StoreSurfArgs a)
{
  uint32_t c = (uint32_t)__popcll(a.mask[blockIdx.x * SSURF_WORDS + threadIdx.x]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
  __shared__ uint32_t wtot[4];
  if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) a.blk_tot[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

// ---- pass 2
__global__ __launch_bounds__(1024) void store_surface_scan_kernel(const uint32_t *tot, mu64 *off, uint32_t n, mu64 *total)
{
  scan_block_totals(tot, off, n, total);
}

// ---- pass 3: the records, in word order
template <bool MARKER>
__global__ __launch_bounds__(256) void store_surface_emit_kernel(StoreSurfArgs a)
{
  __shared__ mu64 sM[SSURF_WORDS];
  __shared__ uint32_t sB[SSURF_WORDS];
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * SSURF_WORDS;
  const mu64 Mt = a.mask[t0 + threadIdx.x];
  sM[threadIdx.x] = Mt;
  sB[threadIdx.x] = block_scan_256((uint32_t)__popcll(Mt), wsum);
  __syncthreads();
  const mu64 base = a.blk_off[blockIdx.x];
  const float fres = (float)a.res, ftau = (float)a.tau;
  for (int w = 0; w < 64; ++w) // the wave's 64 words, one after the other; lane = z inside the word
  {
    const int idx = wave * 64 + w;
    const mu64 M = sM[idx];
    if (M == 0ull) continue; // (most words hold no surface; the same for the whole wave)
    StoreWord p;
    p.find(a, t0 + (uint32_t)idx);
    const mi32x4 k = a.key[p.i];
    const uint32_t raw = __builtin_nontemporal_load(sm_chunk(a, p.i) + (p.lx * (uint32_t)(STORE_CS * STORE_CS) + p.ly * (uint32_t)STORE_CS + (uint32_t)lane));
    if (!((M >> lane) & 1ull)) continue;
    const mu64 o = base + sB[idx] + popc_below(M, lane);
    if (o < a.cap) // (the count pass sized the buffers; a store that changed in between must not write beyond them)
    {
      const int32_t x = k.x * STORE_CS + (int32_t)p.lx, y = k.y * STORE_CS + (int32_t)p.ly, z = k.z * STORE_CS + lane;
      surf_put_record(a.rec, o, x, y, z, raw);
      if (MARKER) surf_put_marker(a.marker, o, surf_metres(x, fres), surf_metres(y, fres), z, raw, fres, ftau);
    }
  }
}

// ---- host side
size_t store_surface_blocks(uint32_t n_chunks) { return (size_t)n_chunks * (4096u / SSURF_WORDS); }

static StoreSurfArgs store_surf_args(const ws_store *st, const ws_store::Surface &q, const StoreSurfCall &c, size_t cap)
{
  StoreSurfArgs a;
  store_words_bind(a, st, static_cast<const char *>(q.table_dev.p), c.n_chunks);
  a.band = c.band, a.tau = c.tau, a.res = c.res;
  for (int k = 0; k < 3; ++k) a.lo[k] = c.lo[k], a.hi[k] = c.hi[k];
  a.mask = static_cast<mu64 *>(q.mask.p);
  a.blk_tot = static_cast<uint32_t *>(q.blk_tot.p);
  a.blk_off = static_cast<const mu64 *>(q.blk_off.p);
  a.rec = static_cast<su32x4 *>(q.rec.p);
  a.marker = static_cast<float *>(q.marker.p);
  a.cap = cap;
  return a;
}

// the tables' upload, then passes 1 and 2; the total arrives in q.total.host (pinned) once the stream has been synchronised
int launch_store_surface_count(ws_store *st, ws_store::Surface &q, const StoreSurfCall &c)
{
  hipStream_t s = st->ctx->stream;
  WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_word_table_bytes(c.n_chunks), hipMemcpyHostToDevice, s));
  const StoreSurfArgs a = store_surf_args(st, q, c, 0);
  const uint32_t blocks = (uint32_t)store_surface_blocks(c.n_chunks);
  q.timer.mark(0, s);
  hipLaunchKernelGGL(store_surface_count_kernel, dim3(c.n_chunks * 256u), dim3(256), 0, s, a);
  hipLaunchKernelGGL(store_surface_totals_kernel, dim3(blocks), dim3(256), 0, s, a);
  q.timer.mark(1, s);
  hipLaunchKernelGGL(store_surface_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)a.blk_tot, static_cast<mu64 *>(q.blk_off.p), blocks, q.total.dev);
  q.timer.mark(2, s);
  WS_HIP(hipGetLastError());
  return q.total.fetch(s);
}

// pass 3: no record at or beyond `cap` is written
int launch_store_surface_emit(ws_store *st, ws_store::Surface &q, const StoreSurfCall &c, bool marker, size_t cap)
{
  const StoreSurfArgs a = store_surf_args(st, q, c, cap);
  const uint32_t blocks = (uint32_t)store_surface_blocks(c.n_chunks);
  hipStream_t s = st->ctx->stream;
  q.timer.mark(3, s);
  if (marker)
    hipLaunchKernelGGL((store_surface_emit_kernel<true>), dim3(blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((store_surface_emit_kernel<false>), dim3(blocks), dim3(256), 0, s, a);
  q.timer.mark(4, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
