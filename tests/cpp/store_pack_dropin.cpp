// store_pack_dropin.cpp — DeviceGlobalMap::pack, clone and unpack (include/warpsense_hip/app.hpp) from C++: a store from a file of
// chunks, packed whole and as a subset, cloned on the device and unpacked into a store with another default and chunks of its own; the
// statistics and digests of headers, payload and the resulting chunks for tests/test_gpu_store_pack_dropin.py.
//   store_pack_dropin src.bin own.bin tau
// src.bin / own.bin: int32 n, then per chunk 3 int32 (key) and 64^3 uint32
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "dropin_common.hpp"

static bool load(const char *path, warpsense::DeviceGlobalMap &store)
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
    if (ok) store.put_chunk({key[0], key[1], key[2]}, data);
  }
  fclose(f);
  return ok;
}

static void report(const char *name, const warpsense::PackedMap &p)
{
  printf("%s %zu %llu %llu %llu %llu %llu %.9g\n", name, p.n_chunks(), (unsigned long long)p.payload_words, (unsigned long long)p.default_bricks,
         (unsigned long long)p.uniform_bricks, (unsigned long long)p.dense_bricks, (unsigned long long)p.bytes, p.ratio());
  printf("%s_digests %016llx %016llx\n", name, fnv1a(p.headers.data(), p.headers.size() * sizeof(uint32_t)), fnv1a(p.payload.data(), p.payload.size() * sizeof(uint32_t)));
}

static void chunks(const char *name, warpsense::DeviceGlobalMap &store)
{
  std::vector<uint32_t> data;
  for (const auto &k : store.keys())
  {
    store.chunk(k, data);
    printf("%s %d %d %d %016llx\n", name, k[0], k[1], k[2], fnv1a(data.data(), data.size() * sizeof(uint32_t)));
  }
}

int main(int argc, char **argv)
{
  if (argc != 4) return 2;
  const TSDFEntry fill((int16_t)atoi(argv[3]), 0);
  warpsense::DeviceGlobalMap src(fill, 0, 2), dst(TSDFEntry((int16_t)-7, 5), 0, 1);
  if (!load(argv[1], src) || !load(argv[2], dst)) return 3;
  const warpsense::PackedMap all = src.pack();
  all.check();
  report("all", all);
  std::vector<warpsense::DeviceGlobalMap::Key> some;
  const auto keys = src.keys();
  for (size_t i = keys.size(); i-- > 0;)
    if (i % 2 == 0) some.push_back(keys[i]); // every second key, descending
  const warpsense::PackedMap part = src.pack(&some);
  report("part", part);
  const auto copy = src.clone();
  chunks("clone", *copy);
  dst.unpack(part);
  chunks("unpacked", dst);
  // the host statement of the rule on the first chunk of the subset
  const std::vector<uint32_t> first = part.chunk(0);
  printf("expanded %016llx\n", fnv1a(first.data(), first.size() * sizeof(uint32_t)));
  return 0;
}
