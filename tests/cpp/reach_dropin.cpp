// reach_dropin.cpp — MappingNode::reach / global_reach, DeviceGlobalMap::reach / reach_paths and warpsense::local_map_reach /
// local_map_reach_paths / global_map_reach / global_map_reach_paths (include/warpsense_hip/app.hpp, visualization.hpp) from C++: scans
// along a walk of the window through the device global map, then the reach of the window and of the store over the C ABI, and digests
// of their bytes for tests/test_gpu_reach_dropin.py.
//   reach_dropin scans.bin n_points edge resolution tau max_weight segment_chunks x0 y0 z0 [x1 y1 z1 ...]
// scans.bin: one scan of n_points x 3 int32 (map frame, mm) per window position, in order
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::ReachField &f)
{
  printf("%s %zu %zu %zu %u %u %u %d %016llx\n", name, f.cost.size(), f.seeded, f.reached, f.ext[0], f.ext[1], f.ext[2], f.columns ? 1 : 0,
         f.cost.empty() ? 0ull : fnv1a(f.cost.data(), f.cost.size() * sizeof(uint32_t)));
}

static void report(const char *name, const warpsense::ReachPaths &p)
{
  printf("%s %zu %016llx %016llx\n", name, p.headers.size(), fnv1a(p.headers.data(), p.headers.size() * sizeof(warpsense::ReachPathHeader)),
         p.records.empty() ? 0ull : fnv1a(p.records.data(), p.records.size() * sizeof(warpsense::ReachPathRecord)));
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
  // the sensor and six voxels around it as seeds; goals near by, far off in the window and outside it
  std::vector<rmagine::Pointi> seeds = {pos};
  for (int k = 0; k < 3; ++k)
    for (int d : {-2, 2})
    {
      rmagine::Pointi s = pos;
      (&s.x)[k] += d;
      seeds.push_back(s);
    }
  const std::vector<rmagine::Pointi> goals = {rmagine::Pointi(pos.x + 5, pos.y + 5, pos.z), rmagine::Pointi(pos.x - 8, pos.y + 3, pos.z + 1),
                                              rmagine::Pointi(pos.x, pos.y - 12, pos.z + 2), rmagine::Pointi(pos.x + 1000, pos.y, pos.z), pos};
  report("window", node.reach(seeds, 1));
  report("window_paths", warpsense::local_map_reach_paths(node.gpu().tsdf(), goals, 48));
  report("window_costs", warpsense::local_map_reach_paths(node.gpu().tsdf(), goals, 0));
  const rmagine::Pointi wlo(pos.x - 20, pos.y - 20, pos.z - 3), whi(pos.x + 25, pos.y + 12, pos.z + 3); // a height band of the last window
  report("window_columns", node.reach(seeds, 0, true, &wlo, &whi, true));
  report("window_again", warpsense::local_map_reach(node.gpu().tsdf(), seeds, 0, false)); // on the column map that is still there
  const rmagine::Pointi lo(pos.x - 30, pos.y - 30, pos.z - 12), hi(pos.x + 40, pos.y + 30, pos.z + 12); // beyond the window at +x
  report("global", node.global_reach(seeds, 1, false, &lo, &hi));
  printf("chunks %zu\n", store.count());
  report("global_paths", store.reach_paths(goals, 48));
  report("global_free", warpsense::global_map_reach(store, seeds, 0, true));
  report("global_free_paths", warpsense::global_map_reach_paths(store, goals, 16));
  return 0;
}
