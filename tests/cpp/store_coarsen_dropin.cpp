// store_coarsen_dropin.cpp — warpsense::parents_of, DeviceGlobalMap::coarsen and MapPyramid (include/warpsense_hip/mapping.hpp, app.hpp)
// from C++: a store from a file of chunks, a pyramid rebuilt over it, one chunk replaced and the pyramid refreshed over its box, with
// the statistics and digests of every chunk of every level for tests/test_gpu_store_coarsen_dropin.py.
//   store_coarsen_dropin base.bin changed.bin levels min_observed resolution tau
// base.bin / changed.bin: int32 n, then per chunk 3 int32 (key) and 64^3 uint32; the chunks of changed.bin replace those of the base
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

using Key = warpsense::DeviceGlobalMap::Key;

static bool load(const char *path, warpsense::DeviceGlobalMap &store, std::vector<Key> &keys)
{
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  int32_t n = 0;
  bool ok = fread(&n, sizeof n, 1, f) == 1;
  std::vector<uint32_t> data(warpsense::DeviceGlobalMap::CHUNK_WORDS);
  for (int32_t i = 0; ok && i < n; ++i)
  {
    int32_t key[3];
    ok = fread(key, sizeof(int32_t), 3, f) == 3 && fread(data.data(), sizeof(uint32_t), data.size(), f) == data.size();
    if (ok) store.put_chunk({key[0], key[1], key[2]}, data), keys.push_back({key[0], key[1], key[2]});
  }
  fclose(f);
  return ok;
}

static void report(const char *name, warpsense::MapPyramid &p, const std::vector<warpsense::CoarsenStats> &stats)
{
  std::vector<uint32_t> data;
  for (int l = 1; l <= p.levels(); ++l)
  {
    const warpsense::CoarsenStats &s = stats[(size_t)l - 1];
    printf("%s level %d resolution %d stats %llu %llu %llu %llu\n", name, l, p.resolution(l), (unsigned long long)s.chunks, (unsigned long long)s.created,
           (unsigned long long)s.valued, (unsigned long long)s.short_of);
    for (const Key &key : p.store(l).keys())
    {
      p.store(l).chunk(key, data);
      printf("chunk %d %d %d %016llx\n", key[0], key[1], key[2], fnv1a(data.data(), data.size() * sizeof(uint32_t)));
    }
  }
}

int main(int argc, char **argv)
{
  if (argc != 7) return 2;
  const int levels = atoi(argv[3]), min_observed = atoi(argv[4]), res = atoi(argv[5]);
  const TSDFEntry fill((int16_t)atoi(argv[6]), 0);
  warpsense::DeviceGlobalMap base(fill, 0, 2);
  std::vector<Key> keys, changed;
  if (!load(argv[1], base, keys)) return 3;
  printf("parents");
  for (const Key &k : warpsense::parents_of(keys)) printf(" %d %d %d", k[0], k[1], k[2]);
  printf("\n");
  warpsense::MapPyramid p(base, levels, res, fill, min_observed, 2);
  report("rebuild", p, p.rebuild());
  if (!load(argv[2], base, changed) || changed.empty()) return 3;
  rmagine::Pointi lo(changed[0][0] * 64, changed[0][1] * 64, changed[0][2] * 64), hi = lo;
  for (const Key &k : changed)
  {
    lo = rmagine::Pointi(std::min(lo.x, k[0] * 64), std::min(lo.y, k[1] * 64), std::min(lo.z, k[2] * 64));
    hi = rmagine::Pointi(std::max(hi.x, k[0] * 64 + 63), std::max(hi.y, k[1] * 64 + 63), std::max(hi.z, k[2] * 64 + 63));
  }
  report("refresh", p, p.refresh(lo, hi));
  return 0;
}
