// reg_batch_dropin.cpp — cuda::RegistrationCuda::register_cloud_batch / cuda::TSDFRegistration::register_candidates (include/warpsense_hip)
// from C++: one scan into a fresh map, the moved cloud registered from K start poses in one launch and one by one, the two compared
// bit for bit here, and every result printed for tests/test_gpu_reg_batch_dropin.py to compare with the Python route.
//   reg_batch_dropin scan.bin cloud.bin n_points edge resolution tau max_weight poses.bin k max_iterations
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "warpsense_hip/mapping.hpp"
#include "dropin_common.hpp"

int main(int argc, char **argv)
{
  if (argc < 11) return 2;
  const size_t n = (size_t)atoll(argv[3]), k = (size_t)atoll(argv[9]);
  const int edge = atoi(argv[4]), res = atoi(argv[5]), tau = atoi(argv[6]), mw = atoi(argv[7]), max_it = atoi(argv[10]);
  std::vector<rmagine::Pointi> scan(n), cloud(n);
  std::vector<rmagine::Matrix4x4f> poses(k); // column-major, as the C ABI takes them
  if (!read_all(argv[1], scan) || !read_all(argv[2], cloud) || !read_all(argv[8], poses)) return 2;
  int size[3] = {edge, edge, edge}, off[3] = {edge / 2, edge / 2, edge / 2}, zero[3] = {0, 0, 0};
  std::vector<TSDFEntry> voxels((size_t)edge * edge * edge, TSDFEntry((int16_t)tau, 0));
  cuda::DeviceMap view(size, off, voxels.data(), zero);
  cuda::HotPathParams params;
  params.map_resolution = res;
  params.tau = tau;
  params.max_weight = mw;
  params.max_iterations = max_it;
  cuda::TSDFRegistration reg(params, view);
  reg.tsdf().update_tsdf(scan, rmagine::Pointi(0, 0, 0), rmagine::Pointi(0, 0, 32768));

  const cuda::RegistrationCuda::BatchResult b = reg.register_candidates(cloud, poses);
  if (b.poses.size() != k || b.iterations.size() != k || b.e.size() != k || b.c.size() != k) return 3;
  int differ = 0;
  for (size_t i = 0; i < k; ++i)
  {
    const rmagine::Matrix4x4f T = reg.register_cloud(cloud, poses[i]);
    if (std::memcmp(&T, &b.poses[i], sizeof T) != 0 || reg.last_iterations() != b.iterations[i]) differ += 1;
    unsigned bits[16];
    std::memcpy(bits, &b.poses[i], sizeof bits);
    printf("pose %zu %d %d %d", i, b.iterations[i], b.e[i], b.c[i]);
    for (int w = 0; w < 16; ++w) printf(" %08x", bits[w]);
    printf("\n");
  }
  printf("differ %d\n", differ);
  printf("best %lld\n", warpsense::batch_best(b.e, b.c, (int32_t)(n / 2)));
  const cuda::RegistrationCuda::BatchResult none = reg.register_candidates(cloud, std::vector<rmagine::Matrix4x4f>());
  printf("empty %zu\n", none.poses.size());
  return differ == 0 ? 0 : 1;
}
