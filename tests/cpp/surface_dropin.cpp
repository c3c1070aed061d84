// surface_dropin.cpp — warpsense::local_map_cloud / local_map_skeleton (include/warpsense_hip/visualization.hpp) from C++:
// one scan into a fresh map, the surface cloud of avg_map over the C ABI, and a digest of its bytes for tests/test_gpu_surface.py.
//   surface_dropin scan.bin n_points edge resolution tau max_weight px py pz
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

int main(int argc, char **argv)
{
  if (argc < 10) return 2;
  const size_t n = (size_t)atoll(argv[2]);
  const int edge = atoi(argv[3]), res = atoi(argv[4]), tau = atoi(argv[5]), mw = atoi(argv[6]);
  int pos[3] = {atoi(argv[7]), atoi(argv[8]), atoi(argv[9])};
  std::vector<rmagine::Pointi> scan(n);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(scan.data(), sizeof(rmagine::Pointi), n, f) != n) return 2;
  fclose(f);
  int size[3] = {edge, edge, edge}, off[3] = {edge / 2, edge / 2, edge / 2}, zero[3] = {0, 0, 0};
  std::vector<TSDFEntry> voxels((size_t)edge * edge * edge, TSDFEntry((int16_t)tau, 0));
  cuda::DeviceMap view(size, off, voxels.data(), zero);
  cuda::TSDFCuda tsdf(view, tau, mw, res);
  {
    // (both device maps start as copies of the host map: new_map is already the default map)
    tsdf.update_tsdf(scan, rmagine::Pointi(0, 0, 0), rmagine::Pointi(0, 0, 32768));
  }
  const warpsense::SurfaceCloud all = warpsense::local_map_cloud(tsdf);
  printf("cloud %zu %016llx %016llx\n", all.records.size(), fnv1a(all.records.data(), all.records.size() * sizeof(warpsense::SurfaceRecord)),
         fnv1a(all.marker.data(), all.marker.size() * sizeof(float)));
  const rmagine::Pointi lo(-edge / 4, -3, -edge / 2), hi(edge / 4, edge / 3, 5);
  const warpsense::SurfaceCloud box = warpsense::local_map_cloud(tsdf, WS_MAP_AVG, false, &lo, &hi, tau / 2);
  printf("box %zu %016llx %zu\n", box.records.size(), fnv1a(box.records.data(), box.records.size() * sizeof(warpsense::SurfaceRecord)), box.marker.size());
  const auto sk = warpsense::local_map_skeleton(size, pos, res);
  printf("skeleton %zu", sk.size());
  for (const auto &p : sk) printf(" %.17g %.17g %.17g", p[0], p[1], p[2]);
  printf("\n");
  return 0;
}
