// map_sample.hip — the point sample of a device map (gfx950): what the map says at N given points -- the interpolated signed
// distance, the smallest weight of the cell, the class against a band and the nearest voxel's entry, and on request the TSDF gradient
// there and the ordered selection of the points of some classes.  The rules are stated in warpsense_hip.h at ws_map_sample;
// ws_sample.h applies them, and this file gives it the window (ws_field_window.h: the ring addressing, the z-pair loads):
//
//   sample_kernel        one lane per point: the cell, the record, the gradient; the class counts of the workgroup
//   sample_scan_kernel   exclusive scan of the workgroups' selected counts (one workgroup)
//   sample_emit_kernel   the selected points in input order
//
// Plain launches on the context's stream.  The only atomics are the class counters (integer sums, one add per class and workgroup).
#include "ws_field_window.h"
#include "ws_sample.h"

namespace ws
{
struct SampleArgs
{
  RayArgs f; // the window (its RayCommon is not read)
  SampleCommon s;
};

__global__ __launch_bounds__(SAMPLE_WG) void sample_kernel(SampleArgs a)
{
  const uint32_t i = blockIdx.x * SAMPLE_WG + threadIdx.x;
  uint32_t cls = 4u;
  if (i < a.s.n) // (n <= the capacity of the record buffer: sample_run grows it first)
  {
    WindowField fld(a.f);
    cls = sample_body(a.s, fld, true, i);
  }
  sample_tally(a.s, cls);
}

__global__ __launch_bounds__(1024) void sample_scan_kernel(SampleArgs a, uint32_t blocks) { sample_scan(a.s, blocks); }

__global__ __launch_bounds__(SAMPLE_WG) void sample_emit_kernel(SampleArgs a) { sample_emit(a.s); }

int launch_sample(ws_map *m, SampleResult &q, int which, const int32_t *pts_dev, size_t n, int32_t band, uint32_t flags)
{
  SampleArgs a;
  std::memset(&a.f.c, 0, sizeof(a.f.c));
  a.f.data = m->data[which].as<uint32_t>();
  a.f.mp = m->par[which];
  for (int k = 0; k < 3; ++k)
  {
    a.f.wlo[k] = a.f.mp.pos[k] - a.f.mp.size[k] / 2;
    a.f.whi[k] = a.f.wlo[k] + a.f.mp.size[k] - 1;
  }
  a.s = sample_common(q, pts_dev, n, m->res, band, flags);
  return sample_launch(q, m->ctx->stream, a, sample_kernel, sample_scan_kernel, sample_emit_kernel);
}

} // namespace ws
