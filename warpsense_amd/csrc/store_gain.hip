// store_gain.hip — the view gain of the chunk store (ws_store_view_gain, include/warpsense_hip.h): the walk of ws_gain.h over the 64^3
// chunks of the global map in device memory, wherever they lie.  The rules of a sample, a class and a record are those of ws_gain.h;
// what is new is the SPARSE field: a voxel of the box in an absent chunk is UNKNOWN, it counts and blocks nothing.
//
//   store_gain_prep_kernel   one lane per direction of the fan
//   store_gain_kernel        grid (ceil(n / 64), m): one wave per 64 rays of a view, one lane per ray
//   store_gain_best_kernel   the largest unknown_k2
//
// Chunk lookup: the open-addressing table of the ray cast (StoreField::lookup), which lists the present chunks the box overlaps.  A
// lane keeps the chunk of its last voxel (key and pointer, the cache of StoreField) and looks a chunk up again only when the voxel's
// chunk changes: one probe per 64 voxels along an axis.  The walk passes an absent chunk sample by sample, without a load.
#include "ws_field_store.h"
#include "ws_gain.h"

namespace ws
{
struct StoreGainArgs
{
  StoreRayArgs s; // the table and the segments (its RayCommon and its boxes are not used)
  GainCommon c;
};

// the chunks as the field of ws_gain.h: StoreField's lookup behind its one-chunk cache
struct StoreGainField
{
  StoreField f;
  __device__ __forceinline__ explicit StoreGainField(const StoreRayArgs &args) : f(args) {}
  __device__ __forceinline__ bool entry(const int32_t v[3], uint32_t &raw)
  {
    if (f.a.n_chunks == 0u) return false; // (no table at all)
    const int32_t cx = v[0] >> 6, cy = v[1] >> 6, cz = v[2] >> 6;
    if (cx != f.ck[0] || cy != f.ck[1] || cz != f.ck[2])
    {
      f.cp = f.lookup(cx, cy, cz);
      f.ck[0] = cx, f.ck[1] = cy, f.ck[2] = cz;
    }
    if (!f.cp) return false;
    raw = f.cp[((uint32_t)v[0] & 63u) * (uint32_t)(STORE_CS * STORE_CS) + ((uint32_t)v[1] & 63u) * (uint32_t)STORE_CS + ((uint32_t)v[2] & 63u)];
    return true;
  }
};

__global__ __launch_bounds__(256) void store_gain_prep_kernel(StoreGainArgs a)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < a.c.n) gain_prep(a.c, i);
}

__global__ __launch_bounds__(64) void store_gain_kernel(StoreGainArgs a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x, view = blockIdx.y;
  const bool active = i < a.c.n;
  GainLane r;
  if (active)
  {
    StoreGainField fld(a.s);
    const int32_t o[3] = {a.c.origins[3 * (size_t)view], a.c.origins[3 * (size_t)view + 1], a.c.origins[3 * (size_t)view + 2]};
    r = gain_march(a.c, fld, o, a.c.prep[i]);
  }
  gain_reduce(a.c, view, i, active, r);
}

__global__ __launch_bounds__(256) void store_gain_best_kernel(StoreGainArgs a) { gain_best(a.c); }

// the table's upload, then the launch sequence
int launch_store_gain(ws_store *st, ws_store::Gain &q, const GainCall &c, uint32_t n_chunks)
{
  StoreGainArgs a;
  a.s = StoreRayArgs{};
  a.s.n_chunks = n_chunks;
  a.s.table = q.table_dev.as<StoreRaySlot>();
  a.s.mask = (uint32_t)store_ray_table_slots(n_chunks) - 1u;
  a.s.segs = st->seg_tab.as<uint32_t *>();
  a.s.seg_shift = st->seg_shift;
  a.c = gain_common(q, c);
  hipStream_t s = st->ctx->stream;
  if (n_chunks) WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_ray_table_slots(n_chunks) * sizeof(StoreRaySlot), hipMemcpyHostToDevice, s));
  return gain_launch(q, s, a, store_gain_prep_kernel, store_gain_kernel, store_gain_best_kernel);
}

} // namespace ws
