// raycast_dropin.cpp — warpsense::local_map_raycast (include/warpsense_hip/visualization.hpp) from C++: one scan into a fresh map,
// the ray cast of avg_map over the C ABI, and digests of its bytes for tests/test_gpu_raycast.py.
//   raycast_dropin scan.bin n_points edge resolution tau max_weight
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

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
  const warpsense::RayCast a = warpsense::local_map_raycast(tsdf, rmagine::Pointi(0, 0, 0), scan, 3000, true); // the scan's points as directions
  printf("dirs %zu %zu %016llx %016llx\n", a.records.size(), a.hits, fnv1a(a.records.data(), a.records.size() * sizeof(warpsense::RayHit)),
         fnv1a(a.gradient.data(), a.gradient.size() * sizeof(rmagine::Pointi)));
  const warpsense::RayCast b = warpsense::local_map_raycast(tsdf, rmagine::Pointi(10, -20, 5), scan, 3000, false, true, true);
  printf("targets %zu %zu %016llx -\n", b.records.size(), b.hits, fnv1a(b.records.data(), b.records.size() * sizeof(warpsense::RayHit)));
  return 0;
}
