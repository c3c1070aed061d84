// store_distance.hip — pass 0 of the distance field of the chunk store (ws_store_distance, include/warpsense_hip.h): the classes and
// g0 of map_distance.hip, read straight out of the 64^3 chunks of the global map in device memory, wherever they lie.  The line
// passes behind it are those of map_distance.hip (dist_passes), on the same records and planes.
//
//   store_dist_classify_kernel   a wave per (x, y) column of the box, four columns of consecutive y per workgroup.  The wave walks z
//                                in chunk-aligned steps of 64: a chunk row of 64 z voxels is ONE wave-wide, 256-byte aligned load, and
//                                the four rows of a workgroup are one 1 KB run of a chunk (while y stays inside it).  The first and
//                                the last step of a column are cut by the box: lanes outside it stay idle.
//                                <COLUMNS>: the same walk, reduced with ballots to one class and one g0 per column
//
// A voxel of an absent chunk is unknown, whatever the store's fill entry is.  The chunk under a step is the same for the whole wave:
// one lookup per step through the open-addressing table key -> slot of store_raycast.hip (ws_internal.h), which the host has filled
// with the present chunks the box overlaps.  For an absent chunk nothing is read.
// <COLUMNS> does not walk where no listed chunk lies: the host passes the z range of the listed chunks cut to the box, the walk keeps
// to it, and a column whose box range reaches beyond it holds unknown voxels.  That is what bounds a column of 2^32 voxels over a
// handful of chunks by the chunks.  The dense walk of the 3-D form writes every record of the box.
// Integers only, plain launches on the context's stream; the one atomic is the site counter (one add per wave).
#include "ws_device.h"

namespace ws
{
struct StoreDistArgs
{
  int32_t lo[3];
  int32_t hi_z;
  int32_t zlo, zhi;       // the z range of the listed chunks, cut to the box (zlo > zhi: none)
  uint32_t ny;
  uint32_t col0, n_cols;  // first column of this launch, columns of the box
  uint32_t r2;
  uint32_t flags;
  uint32_t *rec;
  uint16_t *plane;
  unsigned long long *sites;
  const StoreRaySlot *table;
  uint32_t mask;          // table places - 1
  uint32_t *const *segs;  // base pointers of the store's segments
  uint32_t seg_shift;
};

template <bool COLUMNS>
__global__ __launch_bounds__(256) void store_dist_classify_kernel(StoreDistArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t col64 = (uint64_t)a.col0 + (uint64_t)blockIdx.x * 4u + (uint64_t)wave;
  if (col64 >= (uint64_t)a.n_cols) return; // (the same for the whole wave)
  const uint32_t col = (uint32_t)col64;
  const bool any_weight = (a.flags & WS_DISTANCE_ANY_WEIGHT) != 0, unknown_occ = (a.flags & WS_DISTANCE_UNKNOWN_OCCUPIED) != 0;
  const uint32_t xr = col / a.ny, yr = col - xr * a.ny;
  const int32_t x = (int32_t)((int64_t)a.lo[0] + (int64_t)xr), y = (int32_t)((int64_t)a.lo[1] + (int64_t)yr); // voxels of the box
  const int32_t cx = x >> 6, cy = y >> 6;
  const uint32_t row = ((uint32_t)x & 63u) * (uint32_t)(STORE_CS * STORE_CS) + ((uint32_t)y & 63u) * (uint32_t)STORE_CS;
  const int32_t lo_z = a.lo[2], hi_z = a.hi_z;
  const bool listed = a.zlo <= a.zhi;
  // the z range the wave walks: the box (every record is written), or under COLUMNS the part of it that listed chunks can cover
  const int32_t w_lo = COLUMNS ? a.zlo : lo_z, w_hi = COLUMNS ? a.zhi : hi_z;
  const uint64_t out0 = (uint64_t)col * ((uint64_t)((int64_t)hi_z - (int64_t)lo_z) + 1ull);
  uint32_t n_sites = 0;
  bool occ = false, fre = false;
  bool unk = !listed || lo_z < a.zlo || hi_z > a.zhi; // COLUMNS: voxels of the column beyond every listed chunk
  if (w_lo <= w_hi)
  {
    const int32_t c_hi = w_hi >> 6;
    for (int32_t cz = w_lo >> 6;; ++cz)
    {
      const int32_t z = cz * STORE_CS + lane; // (keys are floor(int32 / 64): 64 k + 63 fits)
      const bool in = z >= w_lo && z <= w_hi;
      const uint32_t slot = listed ? store_ray_find(a.table, a.mask, cx, cy, cz) : STORE_ABSENT; // (uniform)
      uint32_t cls = 0u;
      if (slot != STORE_ABSENT)
      {
        const uint32_t *p = a.segs[slot >> a.seg_shift] + (size_t)(slot & ((1u << a.seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS + row;
        if (in) cls = dist_class(p[lane], any_weight);
      }
      const bool site = in && (cls == 2u || (unknown_occ && cls == 0u));
      if (COLUMNS)
      {
        occ = occ || __ballot(in && cls == 2u) != 0ull;
        unk = unk || __ballot(in && cls == 0u) != 0ull;
        fre = fre || __ballot(in && cls == 1u) != 0ull;
      }
      else
      {
        if (in)
        {
          const uint64_t at = out0 + (uint64_t)((int64_t)z - (int64_t)lo_z);
          a.rec[at] = cls << 30;
          a.plane[at] = (uint16_t)(site ? 0u : a.r2);
        }
        n_sites += (uint32_t)__popcll(__ballot(site));
      }
      if (cz == c_hi) break;
    }
  }
  if (COLUMNS)
  {
    const bool site = occ || (unknown_occ && unk);
    const uint32_t cls = occ ? 2u : (site ? 0u : (fre ? 1u : 0u));
    if (lane == 0)
    {
      a.rec[col] = cls << 30;
      a.plane[col] = (uint16_t)(site ? 0u : a.r2);
    }
    n_sites = site ? 1u : 0u;
  }
  if (lane == 0 && n_sites) atomicAdd(a.sites, (unsigned long long)n_sites);
}

// the table's upload, the site counter's clearing, then pass 0 (events 0, 1) in launches of at most 2^24 columns
int launch_store_dist_classify(ws_store *st, ws_store::Dist &q, const StoreDistCall &c, int32_t R, uint32_t flags)
{
  StoreDistArgs a;
  for (int k = 0; k < 3; ++k) a.lo[k] = c.lo[k];
  a.hi_z = c.hi[2];
  a.zlo = c.zlo, a.zhi = c.zhi;
  a.ny = c.ny;
  a.n_cols = c.nx * c.ny;
  a.r2 = (uint32_t)(R * R);
  a.flags = flags;
  a.rec = q.rec.as<uint32_t>();
  a.plane = q.plane.as<uint16_t>();
  a.sites = q.sites.dev;
  a.table = q.table_dev.as<StoreRaySlot>();
  a.mask = (uint32_t)store_ray_table_slots(c.n_chunks) - 1u;
  a.segs = st->seg_tab.as<uint32_t *>();
  a.seg_shift = st->seg_shift;
  hipStream_t s = st->ctx->stream;
  if (c.n_chunks)
    WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_ray_table_slots(c.n_chunks) * sizeof(StoreRaySlot), hipMemcpyHostToDevice, s));
  WS_HIP(hipMemsetAsync(a.sites, 0, sizeof(unsigned long long), s));
  q.timer.mark(0, s);
  const uint32_t per_launch = 1u << 24;
  for (uint64_t c0 = 0; c0 < (uint64_t)a.n_cols; c0 += per_launch)
  {
    a.col0 = (uint32_t)c0;
    const uint32_t cols = (uint32_t)std::min<uint64_t>((uint64_t)a.n_cols - c0, per_launch);
    if (flags & WS_DISTANCE_COLUMNS)
      hipLaunchKernelGGL((store_dist_classify_kernel<true>), dim3((cols + 3u) / 4u), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((store_dist_classify_kernel<false>), dim3((cols + 3u) / 4u), dim3(256), 0, s, a);
  }
  q.timer.mark(1, s);
  return WS_OK;
}

} // namespace ws
