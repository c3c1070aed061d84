// map_gain.hip — view gain of a device map (gfx950): what the sensor would see from m candidate origins along one fan of n directions,
// as counts and k^2-weighted sums of UNKNOWN and FREE samples per view, in one launch.  The rules are stated in warpsense_hip.h at
// ws_map_view_gain; ws_gain.h walks them, and this file gives it the window: the ring addressing of WindowField::entry.
//
//   map_gain_prep_kernel   one lane per direction of the fan
//   map_gain_kernel        grid (ceil(n / 64), m): one wave per 64 rays of a view, one lane per ray; the wave's sums go into the view's
//                          record with one integer atomic add per field
//   map_gain_best_kernel   the largest unknown_k2
//
// A sample reads ONE entry (a class lookup), where the ray cast gathers eight corners and interpolates.
#include "ws_field_window.h"
#include "ws_gain.h"

namespace ws
{
struct MapGainArgs
{
  RayArgs w; // data and ring parameters (its RayCommon is not used)
  GainCommon c;
};

__global__ __launch_bounds__(256) void map_gain_prep_kernel(MapGainArgs a)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < a.c.n) gain_prep(a.c, i);
}

__global__ __launch_bounds__(64) void map_gain_kernel(MapGainArgs a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x, view = blockIdx.y;
  const bool active = i < a.c.n;
  GainLane r;
  if (active)
  {
    WindowField fld(a.w);
    const int32_t o[3] = {a.c.origins[3 * (size_t)view], a.c.origins[3 * (size_t)view + 1], a.c.origins[3 * (size_t)view + 2]};
    r = gain_march(a.c, fld, o, a.c.prep[i]);
  }
  gain_reduce(a.c, view, i, active, r);
}

__global__ __launch_bounds__(256) void map_gain_best_kernel(MapGainArgs a) { gain_best(a.c); }

int launch_map_gain(ws_map *m, GainResult &q, int which, const GainCall &c)
{
  MapGainArgs a;
  a.w.data = m->data[which].as<uint32_t>();
  a.w.mp = m->par[which];
  for (int k = 0; k < 3; ++k) a.w.wlo[k] = c.lo[k], a.w.whi[k] = c.hi[k];
  a.w.c = RayCommon{};
  a.c = gain_common(q, c);
  return gain_launch(q, m->ctx->stream, a, map_gain_prep_kernel, map_gain_kernel, map_gain_best_kernel);
}

} // namespace ws
