// distance_dropin.cpp — warpsense::local_map_distance (include/warpsense_hip/visualization.hpp) from C++: one scan into a fresh map,
// the distance field of avg_map over the C ABI, and digests of its bytes for tests/test_gpu_distance.py.
//   distance_dropin scan.bin n_points edge resolution tau max_weight
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::DistanceField &f)
{
  printf("%s %d %d %d %zu %016llx\n", name, f.extent[0], f.extent[1], f.extent[2], f.sites, fnv1a(f.records.data(), f.records.size() * sizeof(uint32_t)));
}

int main(int argc, char **argv)
{
  if (argc < 7) return 2;
  const size_t n = (size_t)atoll(argv[2]);
  const int edge = atoi(argv[3]), res = atoi(argv[4]), tau = atoi(argv[5]), mw = atoi(argv[6]);
  std::vector<rmagine::Pointi> scan(n);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(scan.data(), sizeof(rmagine::Pointi), n, f) != n) return 2;
  fclose(f);
  int size[3] = {edge, edge, edge}, off[3] = {edge / 2, edge / 2, edge / 2}, zero[3] = {0, 0, 0};
  std::vector<TSDFEntry> voxels((size_t)edge * edge * edge, TSDFEntry((int16_t)tau, 0));
  cuda::DeviceMap view(size, off, voxels.data(), zero);
  cuda::TSDFCuda tsdf(view, tau, mw, res);
  tsdf.update_tsdf(scan, rmagine::Pointi(0, 0, 0), rmagine::Pointi(0, 0, 32768));
  report("window", warpsense::local_map_distance(tsdf, 20));
  const rmagine::Pointi lo(-edge / 4, -3, -6), hi(edge / 4, edge / 3, 5);
  report("box", warpsense::local_map_distance(tsdf, 7, true, false, true, &lo, &hi));
  report("columns", warpsense::local_map_distance(tsdf, 40, false, true, false, &lo, &hi));
  return 0;
}
