// frontier_dropin.cpp — MappingNode::frontier / global_frontier, DeviceGlobalMap::frontier and warpsense::local_map_frontier /
// global_map_frontier (include/warpsense_hip/app.hpp, visualization.hpp) from C++: scans along a walk of the window through the device
// global map, then the frontier of the window and of the store over the C ABI, and digests of their bytes for
// tests/test_gpu_frontier_dropin.py.
//   frontier_dropin scans.bin n_points edge resolution tau max_weight segment_chunks x0 y0 z0 [x1 y1 z1 ...]
// scans.bin: one scan of n_points x 3 int32 (map frame, mm) per window position, in order
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::Frontier &f)
{
  printf("%s %zu %zu %016llx %016llx %016llx\n", name, f.records.size(), f.clusters.size(),
         fnv1a(f.records.data(), f.records.size() * sizeof(warpsense::FrontierRecord)),
         f.labels.empty() ? 0ull : fnv1a(f.labels.data(), f.labels.size() * sizeof(uint32_t)),
         f.clusters.empty() ? 0ull : fnv1a(f.clusters.data(), f.clusters.size() * sizeof(warpsense::FrontierCluster)));
}

int main(int argc, char **argv)
{
  if (argc < 11 || (argc - 8) % 3 != 0) return 2;
  const size_t n = (size_t)atoll(argv[2]);
  const int edge = atoi(argv[3]), steps = (argc - 8) / 3;
  cuda::HotPathParams hot;
  hot.map_resolution = atoi(argv[4]);
  hot.tau = atoi(argv[5]);
  hot.max_weight = atoi(argv[6]);
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
    pos = rmagine::Pointi(atoi(argv[8 + 3 * k]), atoi(argv[9 + 3 * k]), atoi(argv[10 + 3 * k]));
    if (fread(scan.data(), sizeof(rmagine::Pointi), n, f) != n) return 3;
    if (k) node.shift_map_device(pos);
    node.gpu().tsdf().update_tsdf(scan, pos, rmagine::Pointi(0, 0, 32768));
  }
  fclose(f);
  report("window", node.frontier());
  report("window_tau", node.frontier(true, hot.tau));
  const rmagine::Pointi wlo(pos.x - 10, pos.y - 20, pos.z - 5), whi(pos.x + 25, pos.y + 12, pos.z + 9); // a box of the last window
  report("window_box", warpsense::local_map_frontier(node.gpu().tsdf(), WS_MAP_AVG, false, 0, true, &wlo, &whi));
  report("global", node.global_frontier()); // the bounding box of the chunks grown by one voxel
  printf("chunks %zu\n", store.count());
  report("bounds", store.frontier(true, hot.tau)); // the bounding box itself
  const rmagine::Pointi lo(-20, -40, -30), hi(70, 10, 30); // a box that is in no window of the walk
  report("box", warpsense::global_map_frontier(store, true, 0, false, &lo, &hi));
  return 0;
}
