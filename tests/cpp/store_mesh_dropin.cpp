// store_mesh_dropin.cpp — MappingNode::global_mesh and warpsense::global_map_mesh (include/warpsense_hip/app.hpp, visualization.hpp)
// from C++: scans along a walk of the window through the device global map, then the mesh of the store over the C ABI, and digests
// of its bytes for tests/test_gpu_store_mesh_dropin.py.
//   store_mesh_dropin scans.bin n_points edge resolution tau max_weight segment_chunks x0 y0 z0 [x1 y1 z1 ...]
// scans.bin: one scan of n_points x 3 int32 (map frame, mm) per window position, in order
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
  for (int k = 0; k < steps; ++k)
  {
    const rmagine::Pointi pos(atoi(argv[8 + 3 * k]), atoi(argv[9 + 3 * k]), atoi(argv[10 + 3 * k]));
    if (fread(scan.data(), sizeof(rmagine::Pointi), n, f) != n) return 3;
    if (k) node.shift_map_device(pos);
    node.gpu().tsdf().update_tsdf(scan, pos, rmagine::Pointi(0, 0, 32768));
  }
  fclose(f);
  report("global", node.global_mesh());
  printf("chunks %zu\n", store.count());
  report("any_weight", node.global_mesh(true));
  const rmagine::Pointi lo(-20, -40, -30), hi(70, 10, 30); // a box that is in no window of the walk
  report("box", warpsense::global_map_mesh(store, hot.map_resolution, false, &lo, &hi));
  return 0;
}
