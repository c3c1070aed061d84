// ground_dropin.cpp — warpsense::global_map_ground / global_map_ground_distance, DeviceGlobalMap::ground / ground_distance and
// warpsense::local_map_ground / local_map_ground_distance (include/warpsense_hip/visualization.hpp, app.hpp) from C++: chunks read from
// a file into a device global map, the ground layer of the store and the column distance field over it, then the same of a window
// that the store fills, and digests of their bytes for tests/test_gpu_ground_dropin.py.
//   ground_dropin chunks.bin n_chunks tau segment_chunks lox loy loz hix hiy hiz
// chunks.bin: per chunk 3 int32 (its key), then 262 144 uint32
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::GroundLayer &g)
{
  printf("%s %d %d %d %u %u %llu %llu %llu %llu %016llx\n", name, g.lo[0], g.lo[1], g.lo[2], g.extent[0], g.extent[1], (unsigned long long)g.counts[0],
         (unsigned long long)g.counts[1], (unsigned long long)g.counts[2], (unsigned long long)g.counts[3],
         fnv1a(g.records.data(), g.records.size() * sizeof(warpsense::GroundLayer::Record)));
}

static void report(const char *name, const warpsense::DistanceField &d)
{
  printf("%s %d %d %d %zu %016llx\n", name, d.extent[0], d.extent[1], d.extent[2], d.sites, fnv1a(d.records.data(), d.records.size() * sizeof(uint32_t)));
}

int main(int argc, char **argv)
{
  if (argc != 11) return 2;
  const int n_chunks = atoi(argv[2]), tau = atoi(argv[3]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  warpsense::GlobalMap global((int16_t)tau, 0);
  warpsense::DeviceGlobalMap store(global.get_default_tsdf_entry(), 0, (uint32_t)atoi(argv[4]));
  std::vector<TSDFEntry::RawType> data(warpsense::DeviceGlobalMap::CHUNK_WORDS);
  for (int i = 0; i < n_chunks; ++i)
  {
    int32_t key[3];
    if (fread(key, sizeof(int32_t), 3, f) != 3 || fread(data.data(), sizeof(data[0]), data.size(), f) != data.size()) return 3;
    store.put_chunk(warpsense::DeviceGlobalMap::Key{key[0], key[1], key[2]}, data);
  }
  fclose(f);
  printf("chunks %zu\n", store.count());
  const rmagine::Pointi lo(atoi(argv[5]), atoi(argv[6]), atoi(argv[7])), hi(atoi(argv[8]), atoi(argv[9]), atoi(argv[10]));
  report("store", warpsense::global_map_ground(store.handle(), 3, false, false, false, &lo, &hi));
  report("store_distance", warpsense::global_map_ground_distance(store.handle(), 300, 5));
  report("store_flags", store.ground(20, true, true, true, &lo, &hi));
  report("store_flags_distance", store.ground_distance(65535, 40, true));
  report("bounding", store.ground(64));
  // a rotated window that the store fills: the box of it that the store's call was given
  int size[3] = {32, 32, 150}, off[3] = {5, 7, 11}, pos[3] = {0, 0, 80};
  std::vector<TSDFEntry> voxels((size_t)size[0] * size[1] * size[2], TSDFEntry((int16_t)tau, 0));
  cuda::DeviceMap view(size, off, voxels.data(), pos);
  cuda::TSDFCuda tsdf(view, tau, 640, 50);
  const int32_t wlo[3] = {pos[0] - size[0] / 2, pos[1] - size[1] / 2, pos[2] - size[2] / 2};
  const int32_t whi[3] = {wlo[0] + size[0] - 1, wlo[1] + size[1] - 1, wlo[2] + size[2] - 1};
  WS_CHECK(ws_store_load_box(store.handle(), tsdf.handle(), WS_MAP_AVG, wlo, whi));
  const rmagine::Pointi a(lo.x, lo.y, wlo[2]), b(hi.x, hi.y, whi[2]);
  report("window", warpsense::local_map_ground(tsdf, 3, false, false, false, &a, &b));
  report("window_distance", warpsense::local_map_ground_distance(tsdf, 300, 5));
  report("window_flags", warpsense::local_map_ground(tsdf, 20, true, true, true, &a, &b));
  report("window_whole", warpsense::local_map_ground(tsdf, 64, false, true));
  return 0;
}
