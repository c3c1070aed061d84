// store_changes_dropin.cpp — DeviceGlobalMap::changes (include/warpsense_hip/app.hpp) from C++: two stores from files of chunks, the
// pull transform of a 4 x 4 double, the call over the C ABI with clusters, then with APPEARED alone, and the statistics and digests of
// records, labels and cluster table for tests/test_gpu_changes_dropin.py.
//   store_changes_dropin cur.bin ref.bin pose.bin resolution band free_value min_weight tau
// cur.bin / ref.bin: int32 n, then per chunk 3 int32 (key) and 64^3 uint32; pose.bin: 16 doubles (row-major T_ref_to_cur), 3 doubles (pivot_ref)
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

static void report(const char *name, const warpsense::Changes &c, int resolution)
{
  const warpsense::ChangeStats &s = c.stats;
  printf("%s %llu %llu %llu %llu %llu %llu\n", name, (unsigned long long)s.chunks, (unsigned long long)s.known_both, (unsigned long long)s.appeared,
         (unsigned long long)s.vanished, (unsigned long long)s.new_ground, (unsigned long long)s.sum_abs_diff);
  printf("%s_sizes %zu %zu %zu %.9g\n", name, c.records.size(), c.labels.size(), c.clusters.size(), s.changed_volume_m3(resolution));
  printf("%s_digests %016llx %016llx %016llx\n", name, fnv1a(c.records.data(), c.records.size() * sizeof(warpsense::ChangeRecord)),
         fnv1a(c.labels.data(), c.labels.size() * sizeof(uint32_t)), fnv1a(c.clusters.data(), c.clusters.size() * sizeof(warpsense::FrontierCluster)));
}

int main(int argc, char **argv)
{
  if (argc != 9) return 2;
  const int res = atoi(argv[4]), band = atoi(argv[5]), free_value = atoi(argv[6]), min_weight = atoi(argv[7]);
  const TSDFEntry fill((int16_t)atoi(argv[8]), 0);
  warpsense::DeviceGlobalMap cur(fill, 0, 2), ref(fill, 0, 2);
  if (!load(argv[1], cur) || !load(argv[2], ref)) return 3;
  double pose[19];
  FILE *f = fopen(argv[3], "rb");
  if (!f || fread(pose, sizeof(double), 19, f) != 19) return 3;
  fclose(f);
  const warpsense::FusePose pull = warpsense::fuse_pose(pose, pose + 16);
  report("both", cur.changes(ref, pull, res, band, free_value, min_weight, WS_CHANGES_DEFAULT, true), res);
  report("appeared", cur.changes(ref, pull, res, band, free_value, min_weight, WS_CHANGES_APPEARED, false), res);
  return 0;
}
