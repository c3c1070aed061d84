// mesh_dropin.cpp — warpsense::local_map_mesh (include/warpsense_hip/visualization.hpp) from C++: one scan into a fresh map, the
// mesh of avg_map over the C ABI, and digests of its bytes for tests/test_gpu_mesh.py.
//   mesh_dropin scan.bin n_points edge resolution tau max_weight
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::SurfaceMesh &m)
{
  printf("%s %zu %zu %016llx %016llx\n", name, m.vertices.size(), m.faces.size(), fnv1a(m.vertices.data(), m.vertices.size() * sizeof(warpsense::MeshVertex)),
         fnv1a(m.faces.data(), m.faces.size() * sizeof(warpsense::MeshFace)));
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
  report("mesh", warpsense::local_map_mesh(tsdf));
  const rmagine::Pointi lo(5, -30, -25), hi(32, 30, 25); // the room's +x wall
  report("box", warpsense::local_map_mesh(tsdf, WS_MAP_AVG, true, &lo, &hi));
  return 0;
}
