// sample_dropin.cpp — warpsense::local_map_sample / global_map_sample / DeviceGlobalMap::sample (include/warpsense_hip/visualization.hpp,
// app.hpp) and AppParams::reject_dynamic from C++, as digests and counts for tests/test_gpu_sample_dropin.py.
//   sample_dropin sample scan.bin n_points edge resolution tau max_weight points.bin m_points
//   sample_dropin app clouds.bin scans points_per_scan edge resolution tau max_weight shift_m poses_out.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static bool read_points(const char *path, std::vector<rmagine::Pointi> &out)
{
  FILE *f = fopen(path, "rb");
  const bool ok = f && fread(out.data(), sizeof(rmagine::Pointi), out.size(), f) == out.size();
  if (f) fclose(f);
  return ok;
}

static void print(const char *name, const warpsense::PointSample &s)
{
  printf("%s %zu %llu %llu %llu %llu %016llx %016llx %zu %016llx\n", name, s.records.size(), (unsigned long long)s.counts[0], (unsigned long long)s.counts[1],
         (unsigned long long)s.counts[2], (unsigned long long)s.counts[3], fnv1a(s.records.data(), s.records.size() * sizeof(warpsense::SampleRecord)),
         fnv1a(s.gradient.data(), s.gradient.size() * sizeof(rmagine::Pointi)), s.selected.size(), fnv1a(s.selected.data(), s.selected.size() * sizeof(rmagine::Pointi)));
}

static int run_sample(char **argv)
{
  const size_t n = (size_t)atoll(argv[3]), m = (size_t)atoll(argv[9]);
  const int edge = atoi(argv[4]), res = atoi(argv[5]), tau = atoi(argv[6]), mw = atoi(argv[7]);
  std::vector<rmagine::Pointi> scan(n), points(m);
  if (!read_points(argv[2], scan) || !read_points(argv[8], points)) return 2;
  int size[3] = {edge, edge, edge}, off[3] = {edge / 2, edge / 2, edge / 2}, zero[3] = {0, 0, 0};
  std::vector<TSDFEntry> voxels((size_t)edge * edge * edge, TSDFEntry((int16_t)tau, 0));
  cuda::DeviceMap view(size, off, voxels.data(), zero);
  cuda::TSDFCuda tsdf(view, tau, mw, res);
  tsdf.update_tsdf(scan, rmagine::Pointi(0, 0, 0), rmagine::Pointi(0, 0, 32768));
  const uint32_t free_and_unknown = (1u << WS_SAMPLE_FREE) | (1u << WS_SAMPLE_UNKNOWN);
  print("window", warpsense::local_map_sample(tsdf, points, tau / 2, false, true, free_and_unknown));
  print("window_any", warpsense::local_map_sample(tsdf, points, 0, true, false, 1u << WS_SAMPLE_SURFACE));
  // the window into the chunks of a store, then the same questions of the store
  warpsense::DeviceGlobalMap store(TSDFEntry((int16_t)tau, 0));
  const rmagine::Pointi lo(-(edge / 2), -(edge / 2), -(edge / 2)), hi(edge / 2, edge / 2, edge / 2);
  WS_CHECK(ws_store_save_box(store.handle(), tsdf.handle(), WS_MAP_AVG, &lo.x, &hi.x));
  print("store", warpsense::global_map_sample(store, res, points, tau / 2, false, true, free_and_unknown));
  print("store_box", store.sample(res, points, tau, true, false, 1u << WS_SAMPLE_SURFACE, &lo, &hi));
  return 0;
}

static int run_app(char **argv)
{
  const size_t scans = (size_t)atoll(argv[3]), n = (size_t)atoll(argv[4]);
  warpsense::AppParams p;
  const int edge = atoi(argv[5]);
  p.map_size[0] = p.map_size[1] = edge;
  p.map_size[2] = edge / 2;
  p.hot.map_resolution = atoi(argv[6]);
  p.hot.tau = atoi(argv[7]);
  p.hot.max_weight = atoi(argv[8]);
  p.max_distance = (float)p.hot.tau / 1000.f;
  p.shift = (float)atof(argv[9]);
  p.reject_dynamic = true;
  std::vector<float> clouds(scans * n * 3);
  std::ifstream f(argv[2], std::ios::binary);
  f.read(reinterpret_cast<char *>(clouds.data()), (std::streamsize)(clouds.size() * sizeof(float)));
  if (!f) return 2;
  warpsense::App app(p, "", n);
  std::ofstream poses(argv[10], std::ios::binary);
  for (size_t k = 0; k < scans; ++k)
  {
    const rmagine::Matrix4x4f &pose = app.cloud_callback(&clouds[k * n * 3], n, 3);
    poses.write(reinterpret_cast<const char *>(&pose.data[0][0]), 16 * sizeof(float));
    printf("scan %zu points %zu rejected %zu iterations %d updates %d\n", k, app.last_points(), app.last_rejected(), app.last_iterations(), app.n_updates());
  }
  // MappingNode::sample through the app's node: the origin of the first scan
  const std::vector<rmagine::Pointi> probe = {rmagine::Pointi(25, 25, 25), rmagine::Pointi(1 << 30, 0, 0)};
  print("node", app.node().sample(probe, 0, false, true, 15u));
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 10 && !strcmp(argv[1], "sample")) return run_sample(argv);
  if (argc == 11 && !strcmp(argv[1], "app")) return run_app(argv);
  return 2;
}
