// store_sample.hip — the point sample of the chunk store (ws_store_sample, include/warpsense_hip.h): the body of ws_sample.h over the
// 64^3 chunks of the global map in device memory.  The field is that of the store's ray cast (ws_field_store.h): a voxel is valid only
// in the box and in a chunk the call lists, found through the open-addressing table key -> slot that the host has written.
//
//   store_sample_kernel        one lane per point: the cell (one lookup; more where it straddles a chunk face), the record, the gradient
//   store_sample_scan_kernel   exclusive scan of the workgroups' selected counts (one workgroup)
//   store_sample_emit_kernel   the selected points in input order
#include "ws_field_store.h"
#include "ws_sample.h"

namespace ws
{
struct StoreSampleArgs
{
  StoreRayArgs f; // the chunks (its RayCommon is not read)
  SampleCommon s;
};

__global__ __launch_bounds__(SAMPLE_WG) void store_sample_kernel(StoreSampleArgs a)
{
  const uint32_t i = blockIdx.x * SAMPLE_WG + threadIdx.x;
  uint32_t cls = 4u;
  if (i < a.s.n) // (n <= the capacity of the record buffer: sample_run grows it first)
  {
    StoreField fld(a.f);
    cls = sample_body(a.s, fld, a.f.n_chunks != 0u, i);
  }
  sample_tally(a.s, cls);
}

__global__ __launch_bounds__(1024) void store_sample_scan_kernel(StoreSampleArgs a, uint32_t blocks) { sample_scan(a.s, blocks); }

__global__ __launch_bounds__(SAMPLE_WG) void store_sample_emit_kernel(StoreSampleArgs a) { sample_emit(a.s); }

// the table's upload, then the launch sequence
int launch_store_sample(ws_store *st, ws_store::Sample &q, const StoreRayCall &c, const int32_t *pts_dev, size_t n, int32_t band, uint32_t flags)
{
  StoreSampleArgs a;
  std::memset(&a.f.c, 0, sizeof(a.f.c));
  a.s = sample_common(q, pts_dev, n, c.res, band, flags);
  for (int k = 0; k < 3; ++k) a.f.lo[k] = c.lo[k], a.f.hi[k] = c.hi[k], a.f.blo[k] = c.blo[k], a.f.bhi[k] = c.bhi[k];
  a.f.n_chunks = c.n_chunks;
  a.f.table = q.table_dev.as<StoreRaySlot>();
  a.f.mask = (uint32_t)store_ray_table_slots(c.n_chunks) - 1u;
  a.f.segs = st->seg_tab.as<uint32_t *>();
  a.f.seg_shift = st->seg_shift;
  hipStream_t s = st->ctx->stream;
  if (c.n_chunks)
    WS_HIP(hipMemcpyAsync(q.table_dev.p, q.table_host.p, store_ray_table_slots(c.n_chunks) * sizeof(StoreRaySlot), hipMemcpyHostToDevice, s));
  return sample_launch(q, s, a, store_sample_kernel, store_sample_scan_kernel, store_sample_emit_kernel);
}

} // namespace ws
