// view_gain_dropin.cpp — MappingNode::view_gain / global_view_gain, DeviceGlobalMap::view_gain and warpsense::local_map_view_gain /
// global_map_view_gain (include/warpsense_hip/app.hpp, visualization.hpp) from C++: scans along a walk of the window through the device
// global map, then the view gain of the window and of the store over the C ABI, and digests of their bytes for
// tests/test_gpu_view_gain_dropin.py.
//   view_gain_dropin scans.bin n_points edge resolution tau max_weight segment_chunks views.bin m dirs.bin n max_range x0 y0 z0 [x1 y1 z1 ...]
// scans.bin: one scan of n_points x 3 int32 (map frame, mm) per window position, in order; views.bin, dirs.bin: m x 3 and n x 3 int32
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::ViewGain &g)
{
  printf("%s %zu %zu %llu %016llx %016llx\n", name, g.records.size(), g.rays.size(), (unsigned long long)g.best_unknown_k2,
         g.records.empty() ? 0ull : fnv1a(g.records.data(), g.records.size() * sizeof(warpsense::ViewGainRecord)),
         g.rays.empty() ? 0ull : fnv1a(g.rays.data(), g.rays.size() * sizeof(warpsense::ViewGainRay)));
}

static bool read_points(const char *path, size_t n, std::vector<rmagine::Pointi> &out)
{
  out.resize(n);
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(out.data(), sizeof(rmagine::Pointi), n, f);
  fclose(f);
  return got == n;
}

int main(int argc, char **argv)
{
  if (argc < 16 || (argc - 13) % 3 != 0) return 2;
  const size_t n = (size_t)atoll(argv[2]);
  const int edge = atoi(argv[3]), steps = (argc - 13) / 3;
  cuda::HotPathParams hot;
  hot.map_resolution = atoi(argv[4]);
  hot.tau = atoi(argv[5]);
  hot.max_weight = atoi(argv[6]);
  std::vector<rmagine::Pointi> views, dirs;
  if (!read_points(argv[8], (size_t)atoll(argv[9]), views) || !read_points(argv[10], (size_t)atoll(argv[11]), dirs)) return 2;
  const int32_t range = atoi(argv[12]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;

  warpsense::GlobalMap global((int16_t)hot.tau, 0);
  warpsense::LocalMap local(edge, edge, edge, global);
  warpsense::MappingNode node(hot, local);
  warpsense::DeviceGlobalMap store(global.get_default_tsdf_entry(), 0, (uint32_t)atoi(argv[7]));
  node.attach(&store);
  std::vector<rmagine::Pointi> scan(n);
  rmagine::Pointi pos(0, 0, 0);
  for (int k = 0; k < steps; ++k)
  {
    pos = rmagine::Pointi(atoi(argv[13 + 3 * k]), atoi(argv[14 + 3 * k]), atoi(argv[15 + 3 * k]));
    if (fread(scan.data(), sizeof(rmagine::Pointi), n, f) != n) return 3;
    if (k) node.shift_map_device(pos);
    node.gpu().tsdf().update_tsdf(scan, pos, rmagine::Pointi(0, 0, 32768));
  }
  fclose(f);
  report("window", node.view_gain(views, dirs, range));
  report("window_rays", node.view_gain(views, dirs, range, hot.tau, false, true));
  const rmagine::Pointi wlo(pos.x - 10, pos.y - 20, pos.z - 5), whi(pos.x + 25, pos.y + 12, pos.z + 9); // a box of the last window
  report("window_box", warpsense::local_map_view_gain(node.gpu().tsdf(), views, dirs, range, WS_MAP_AVG, 0, true, true, &wlo, &whi));
  report("global", node.global_view_gain(views, dirs, range, 0, false, true)); // the bounding box of the chunks
  printf("chunks %zu\n", store.count());
  report("store_tau", store.view_gain(hot.map_resolution, views, dirs, range, hot.tau));
  const rmagine::Pointi lo(-20, -40, -30), hi(70, 10, 30); // a box that is in no window of the walk
  report("box", warpsense::global_map_view_gain(store, hot.map_resolution, views, dirs, range, 0, true, true, &lo, &hi));
  report("empty", warpsense::global_map_view_gain(store, hot.map_resolution, views, std::vector<rmagine::Pointi>(), range));
  return 0;
}
