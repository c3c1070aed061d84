// clearance_dropin.cpp — MappingNode::score_trajectories / global_score_trajectories, DeviceGlobalMap::clearance and
// warpsense::local_map_clearance / global_map_clearance (include/warpsense_hip/app.hpp, visualization.hpp) from C++: scans along a walk
// of the window through the device global map, then the clearance of the window and of the store over the C ABI, and digests of their
// bytes for tests/test_gpu_clearance_dropin.py.
//   clearance_dropin scans.bin n_points edge resolution tau max_weight segment_chunks poses.bin t p body.bin k soft x0 y0 z0 [x1 y1 z1 ...]
// scans.bin: one scan of n_points x 3 int32 (map frame, mm) per window position, in order; poses.bin: t x p x 12 int32; body.bin: k x 4 int32
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::Clearance &c)
{
  printf("%s %zu %zu %lld %016llx %016llx\n", name, c.records.size(), c.poses.size(), (long long)c.best,
         c.records.empty() ? 0ull : fnv1a(c.records.data(), c.records.size() * sizeof(warpsense::ClearanceRecord)),
         c.poses.empty() ? 0ull : fnv1a(c.poses.data(), c.poses.size() * sizeof(warpsense::ClearancePose)));
}

int main(int argc, char **argv)
{
  if (argc < 18 || (argc - 15) % 3 != 0) return 2;
  const size_t n = (size_t)atoll(argv[2]), t = (size_t)atoll(argv[9]), p = (size_t)atoll(argv[10]);
  const int edge = atoi(argv[3]), steps = (argc - 15) / 3;
  cuda::HotPathParams hot;
  hot.map_resolution = atoi(argv[4]);
  hot.tau = atoi(argv[5]);
  hot.max_weight = atoi(argv[6]);
  std::vector<warpsense::ClearanceInput> poses(t * p);
  std::vector<warpsense::ClearanceSphere> body((size_t)atoll(argv[12]));
  if (!read_all(argv[8], poses) || !read_all(argv[11], body)) return 2;
  const int32_t soft = atoi(argv[13]), range = atoi(argv[14]);
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
    pos = rmagine::Pointi(atoi(argv[15 + 3 * k]), atoi(argv[16 + 3 * k]), atoi(argv[17 + 3 * k]));
    if (fread(scan.data(), sizeof(rmagine::Pointi), n, f) != n) return 3;
    if (k) node.shift_map_device(pos);
    node.gpu().tsdf().update_tsdf(scan, pos, rmagine::Pointi(0, 0, 32768));
  }
  fclose(f);
  report("window", node.score_trajectories(poses, p, body, soft));                                  // columns, the default range
  report("window_volume", node.score_trajectories(poses, p, body, soft, false, true, true, range)); // a volume, pose records, outside_ok
  report("window_again", warpsense::local_map_clearance(node.gpu().tsdf(), poses, p, body, 0));      // on the distance result that is there
  report("global", node.global_score_trajectories(poses, p, body, soft, true, true));               // the bounding box of the chunks
  printf("chunks %zu\n", store.count());
  const rmagine::Pointi lo(-20, -40, -30), hi(70, 10, 30); // a box that is in no window of the walk
  (void)store.distance(range, true, false, false, &lo, &hi);
  report("store_box", store.clearance(hot.map_resolution, poses, p, body, soft, true));
  report("store_ok", warpsense::global_map_clearance(store, hot.map_resolution, poses, p, body, soft, false, true));
  report("empty", warpsense::global_map_clearance(store, hot.map_resolution, std::vector<warpsense::ClearanceInput>(), p, body, soft));
  return 0;
}
