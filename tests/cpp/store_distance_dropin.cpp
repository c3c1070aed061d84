// store_distance_dropin.cpp — warpsense::global_map_distance and DeviceGlobalMap::distance (include/warpsense_hip/visualization.hpp,
// app.hpp) from C++: chunks read from a file into a device global map, then the distance field of the store over the C ABI, and digests
// of its bytes for tests/test_gpu_store_distance_dropin.py.
//   store_distance_dropin chunks.bin n_chunks tau segment_chunks lox loy loz hix hiy hiz
// chunks.bin: per chunk 3 int32 (its key), then 262 144 uint32
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static void report(const char *name, const warpsense::DistanceField &d)
{
  printf("%s %d %d %d %zu %016llx\n", name, d.extent[0], d.extent[1], d.extent[2], d.sites, fnv1a(d.records.data(), d.records.size() * sizeof(uint32_t)));
}

int main(int argc, char **argv)
{
  if (argc != 11) return 2;
  const int n_chunks = atoi(argv[2]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  warpsense::GlobalMap global((int16_t)atoi(argv[3]), 0);
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
  report("bounding", warpsense::global_map_distance(store.handle(), 7));
  const rmagine::Pointi lo(atoi(argv[5]), atoi(argv[6]), atoi(argv[7])), hi(atoi(argv[8]), atoi(argv[9]), atoi(argv[10]));
  report("box", warpsense::global_map_distance(store.handle(), 40, true, false, true, &lo, &hi));
  report("columns", store.distance(20, false, true, false, &lo, &hi));
  return 0;
}
