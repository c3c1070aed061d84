// store_raycast_dropin.cpp — MappingNode::global_raycast and warpsense::global_map_raycast (include/warpsense_hip/app.hpp,
// visualization.hpp) from C++: scans along a walk of the window through the device global map, then the ray cast of the store over
// the C ABI from the first position of the walk, and digests of its bytes for tests/test_gpu_store_raycast_dropin.py.
//   store_raycast_dropin scans.bin n_points dirs.bin n_dirs max_range edge resolution tau max_weight segment_chunks x0 y0 z0 [x1 y1 z1 ...]
// scans.bin: one scan of n_points x 3 int32 (map frame, mm) per window position, in order; dirs.bin: n_dirs x 3 int32 directions
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::RayCast &r)
{
  printf("%s %zu %zu %016llx ", name, r.records.size(), r.hits, fnv1a(r.records.data(), r.records.size() * sizeof(warpsense::RayHit)));
  if (r.gradient.empty())
    printf("-\n");
  else
    printf("%016llx\n", fnv1a(r.gradient.data(), r.gradient.size() * sizeof(rmagine::Pointi)));
}

int main(int argc, char **argv)
{
  if (argc < 14 || (argc - 11) % 3 != 0) return 2;
  const size_t n = (size_t)atoll(argv[2]), n_dirs = (size_t)atoll(argv[4]);
  const int32_t max_range = atoi(argv[5]);
  const int edge = atoi(argv[6]), steps = (argc - 11) / 3;
  cuda::HotPathParams hot;
  hot.map_resolution = atoi(argv[7]);
  hot.tau = atoi(argv[8]);
  hot.max_weight = atoi(argv[9]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<rmagine::Pointi> dirs(n_dirs);
  FILE *fd = fopen(argv[3], "rb");
  if (!fd || fread(dirs.data(), sizeof(rmagine::Pointi), n_dirs, fd) != n_dirs) return 3;
  fclose(fd);

  warpsense::GlobalMap global((int16_t)hot.tau, 0);
  warpsense::LocalMap local(edge, edge, edge, global);
  warpsense::MappingNode node(hot, local);
  warpsense::DeviceGlobalMap store(global.get_default_tsdf_entry(), 0, (uint32_t)atoi(argv[10]));
  node.attach(&store);
  std::vector<rmagine::Pointi> scan(n);
  rmagine::Pointi origin(0, 0, 0);
  for (int k = 0; k < steps; ++k)
  {
    const rmagine::Pointi pos(atoi(argv[11 + 3 * k]), atoi(argv[12 + 3 * k]), atoi(argv[13 + 3 * k]));
    if (k == 0) origin = rmagine::Pointi(pos.x * hot.map_resolution, pos.y * hot.map_resolution, pos.z * hot.map_resolution);
    if (fread(scan.data(), sizeof(rmagine::Pointi), n, f) != n) return 3;
    if (k) node.shift_map_device(pos);
    node.gpu().tsdf().update_tsdf(scan, pos, rmagine::Pointi(0, 0, 32768));
  }
  fclose(f);
  report("global", node.global_raycast(origin, dirs, max_range, false, true));
  printf("chunks %zu\n", store.count());
  report("any_weight", node.global_raycast(origin, dirs, max_range, true, false));
  const rmagine::Pointi lo(-20, -40, -30), hi(70, 10, 30); // a box that is in no window of the walk
  report("box", warpsense::global_map_raycast(store, hot.map_resolution, origin, dirs, max_range, false, true, &lo, &hi));
  return 0;
}
