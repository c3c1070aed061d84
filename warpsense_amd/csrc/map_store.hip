// map_store.hip — the two kernels of the chunk store (ws_store_*, include/warpsense_hip.h): a box of a map's window into the 64^3
// chunks of the global map in device memory (save) and back (load), LocalMap._area(save = True / False) of the host route.
//
// z is fastest in the ring AND in the chunk.  The (x, y) column of chunk-and-box is at most 64 consecutive words of the chunk, and in
// the ring at most two contiguous pieces, split at the seam.  One wave takes one such column, lane = z inside the chunk: 256 bytes per
// access on both sides.  Everything but z is the same for the whole wave -- the chunk, its slot and segment, the column, the x and y
// parts of get_index (ws_device.h) -- and is computed once per column; a lane adds its z and subtracts the ring's size once if it is
// beyond the seam.  No division per voxel (box_copy_kernel, tsdf_integrate.hip, has three), ring offsets in 64 bits.
//
// Grid: blockIdx.y strides over the chunks the box overlaps (the call's dense slot table, x major), blockIdx.x over the x planes of a
// chunk, the four waves of a workgroup over its y rows.
//   save: a chunk flagged STORE_NEW is written WHOLE, the box's voxel inside the box and fill outside, so a new chunk is written once;
//         of an existing chunk only chunk-and-box is touched.
//   load: only chunk-and-box; a chunk the store does not hold (STORE_ABSENT) is a wave-uniform branch that stores fill.
#include <algorithm>

#include "ws_device.h"

namespace ws
{
struct StoreArgs
{
  uint32_t *ring;          // the map's voxels
  MapParams mp;            // its window when this launch runs
  int32_t lo[3], hi[3];    // the box, inclusive world voxels, inside the window
  int32_t c0[3], nc[3];    // first key and number of the chunks it overlaps, per axis
  uint32_t n_chunks;       // nc[0] * nc[1] * nc[2]
  const uint32_t *table;   // [n_chunks] slot | STORE_NEW, or STORE_ABSENT
  uint32_t *const *segs;   // base pointers of the store's segments
  uint32_t seg_shift;      // a segment holds 1 << seg_shift chunks
  uint32_t fill;
};

template <bool SAVE>
__global__ __launch_bounds__(256) void store_copy_kernel(StoreArgs a)
{
  const int32_t lane = (int32_t)(threadIdx.x & 63u);
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const uint32_t plane = (uint32_t)a.nc[1] * (uint32_t)a.nc[2];
  for (uint32_t c = blockIdx.y; c < a.n_chunks; c += gridDim.y)
  {
    const uint32_t word = a.table[c];
    const bool absent = word == STORE_ABSENT; // (a load's table only: the host never puts it into a save's, store_enqueue in api_store.hip)
    const bool whole = SAVE && (word & STORE_NEW) != 0;
    uint32_t *chunk = nullptr;
    if (!absent)
    {
      const uint32_t slot = word & ~STORE_NEW;
      chunk = a.segs[slot >> a.seg_shift] + (size_t)(slot & ((1u << a.seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
    }
    // the chunk's key offsets in the table (once per chunk and workgroup), its first world voxel, and chunk-and-box relative to it
    const uint32_t ci = c / plane, r = c - ci * plane;
    const uint32_t cj = r / (uint32_t)a.nc[2], ck = r - cj * (uint32_t)a.nc[2];
    const int32_t bx = (a.c0[0] + (int32_t)ci) * STORE_CS, by = (a.c0[1] + (int32_t)cj) * STORE_CS, bz = (a.c0[2] + (int32_t)ck) * STORE_CS;
    const int32_t xa = max(a.lo[0], bx) - bx, xb = min(a.hi[0], bx + STORE_CS - 1) - bx;
    const int32_t ya = max(a.lo[1], by) - by, yb = min(a.hi[1], by + STORE_CS - 1) - by;
    const int32_t za = max(a.lo[2], bz) - bz, zb = min(a.hi[2], bz + STORE_CS - 1) - bz;
    // storage z of the column's first voxel inside the box: the lanes follow it, one subtraction beyond the seam
    const int32_t zs0 = ring(bz + za - a.mp.pos[2] + a.mp.offset[2] + a.mp.size[2], a.mp.size[2]);
    int32_t zi = zs0 + (lane - za);
    if (zi >= a.mp.size[2]) zi -= a.mp.size[2];
    const bool in_z = lane >= za && lane <= zb;
    const int32_t x_first = whole ? 0 : xa, x_last = whole ? STORE_CS - 1 : xb;
    const int32_t y_first = whole ? 0 : ya, y_last = whole ? STORE_CS - 1 : yb;
    for (int32_t lx = x_first + (int32_t)blockIdx.x; lx <= x_last; lx += (int32_t)gridDim.x)
    {
      const bool in_x = lx >= xa && lx <= xb;
      const int32_t xi = in_x ? ring(bx + lx - a.mp.pos[0] + a.mp.offset[0] + a.mp.size[0], a.mp.size[0]) : 0;
      for (int32_t ly = y_first + wave; ly <= y_last; ly += 4)
      {
        const bool in_col = in_x && ly >= ya && ly <= yb;
        const int32_t yi = in_col ? ring(by + ly - a.mp.pos[1] + a.mp.offset[1] + a.mp.size[1], a.mp.size[1]) : 0;
        // size[0] * size[1] < 2^31 (ws_map_create); the row's offset is 64-bit: a 2049^3 window has 8.6 G voxels
        uint32_t *row = a.ring + (int64_t)(xi * a.mp.size[1] + yi) * (int64_t)a.mp.size[2];
        uint32_t *col = chunk + (lx * (STORE_CS * STORE_CS) + ly * STORE_CS);
        const bool in_box = in_col && in_z;
        if (SAVE)
        {
          uint32_t v = a.fill;
          if (in_box) v = row[zi];
          if (whole || in_box) col[lane] = v;
        }
        else if (in_box)
          row[zi] = absent ? a.fill : col[lane];
      }
    }
  }
}

int launch_store_copy(ws_store *st, ws_map *m, const MapParams &par, int which, const int32_t lo[3], const int32_t hi[3], const int32_t c0[3],
                      const int32_t nc[3], const uint32_t *table_dev, bool save, bool any_new, hipStream_t stream)
{
  StoreArgs a;
  a.ring = m->data[which].as<uint32_t>();
  a.mp = par;
  for (int k = 0; k < 3; ++k) a.lo[k] = lo[k], a.hi[k] = hi[k], a.c0[k] = c0[k], a.nc[k] = nc[k];
  a.n_chunks = (uint32_t)((int64_t)nc[0] * nc[1] * nc[2]);
  a.table = table_dev;
  a.segs = st->seg_tab.as<uint32_t *>();
  a.seg_shift = st->seg_shift;
  a.fill = st->fill;
  // x planes per chunk the launch can have work for: all 64 where a new chunk is written whole, else no more than the box is thick
  const int64_t ex = (int64_t)hi[0] - lo[0] + 1;
  const unsigned gx = save && any_new ? (unsigned)STORE_CS : (unsigned)std::min<int64_t>(STORE_CS, ex);
  const dim3 grid(gx, std::min<uint32_t>(a.n_chunks, 65535u));
  if (save)
    hipLaunchKernelGGL((store_copy_kernel<true>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((store_copy_kernel<false>), grid, dim3(256), 0, stream, a);
  WS_HIP(hipGetLastError());
  return WS_OK;
}
} // namespace ws
