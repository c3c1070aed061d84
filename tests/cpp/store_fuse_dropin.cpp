// store_fuse_dropin.cpp — warpsense::fuse_pose and DeviceGlobalMap::fuse (include/warpsense_hip/mapping.hpp, app.hpp) from C++: two
// stores from files of chunks, the pull transform of a 4 x 4 double, a count-only and a real fuse over the C ABI, and digests of every
// chunk of DST for tests/test_gpu_store_fuse_dropin.py.
//   store_fuse_dropin dst.bin src.bin pose.bin resolution max_weight tau
// dst.bin / src.bin: int32 n, then per chunk 3 int32 (key) and 64^3 uint32; pose.bin: 16 doubles (row-major T_src_to_dst), 3 doubles (pivot_src)
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

static void report(const char *name, const warpsense::FuseStats &s)
{
  printf("%s %llu %llu %llu %llu %llu %llu\n", name, (unsigned long long)s.candidates, (unsigned long long)s.created, (unsigned long long)s.averaged,
         (unsigned long long)s.set, (unsigned long long)s.sum_abs_diff, (unsigned long long)s.sum_min_weight);
}

int main(int argc, char **argv)
{
  if (argc != 7) return 2;
  const int res = atoi(argv[4]), max_weight = atoi(argv[5]);
  const TSDFEntry fill((int16_t)atoi(argv[6]), 0);
  warpsense::DeviceGlobalMap dst(fill, 0, 2), src(fill, 0, 2);
  if (!load(argv[1], dst) || !load(argv[2], src)) return 3;
  double pose[19];
  FILE *f = fopen(argv[3], "rb");
  if (!f || fread(pose, sizeof(double), 19, f) != 19) return 3;
  fclose(f);
  const warpsense::FusePose pull = warpsense::fuse_pose(pose, pose + 16);
  printf("pose");
  for (int k = 0; k < 9; ++k) printf(" %d", pull.rot_q30[k]);
  for (int k = 0; k < 3; ++k) printf(" %d", pull.pivot_dst_mm[k]);
  for (int k = 0; k < 3; ++k) printf(" %d", pull.pivot_src_mm[k]);
  printf("\n");
  report("count", dst.fuse(src, pull, max_weight, true, res));
  report("fuse", dst.fuse(src, pull, max_weight, false, res));
  std::vector<uint32_t> data;
  for (const auto &key : dst.keys())
  {
    dst.chunk(key, data);
    printf("chunk %d %d %d %016llx\n", key[0], key[1], key[2], fnv1a(data.data(), data.size() * sizeof(uint32_t)));
  }
  return 0;
}
