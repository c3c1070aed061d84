// sweep_dropin.cpp — warpsense::sweep_poses and cuda::ScanPreprocessor::preprocess_sweep (include/warpsense_hip) from C++: the poses of a
// sweep from its end pose and motion, the cloud pre-processed with them by index and by time, everything written for
// tests/test_gpu_sweep_dropin.py to compare with the Python route byte for byte.
//   sweep_dropin cloud.bin n stride mats.bin k columns ring_major time_field resolution out_prefix
// mats.bin: pose_end and motion, column-major.  Writes <out_prefix>.poses (k x 16 float), <out_prefix>.index and <out_prefix>.time (n x 3 int32).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "warpsense_hip/app.hpp"
#include "warpsense_hip/mapping.hpp"
#include "dropin_common.hpp"

static bool write_all(const std::string &path, const void *p, size_t bytes)
{
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = bytes == 0 || fwrite(p, 1, bytes, f) == bytes;
  fclose(f);
  return ok;
}

int main(int argc, char **argv)
{
  if (argc < 11) return 2;
  const size_t n = (size_t)atoll(argv[2]), stride = (size_t)atoll(argv[3]);
  const uint32_t k = (uint32_t)atoll(argv[5]), columns = (uint32_t)atoll(argv[6]);
  const int ring_major = atoi(argv[7]), time_field = atoi(argv[8]), res = atoi(argv[9]);
  const std::string prefix = argv[10];
  std::vector<float> cloud(n * stride);
  std::vector<rmagine::Matrix4x4f> mats(2);
  if (!read_all(argv[1], cloud) || !read_all(argv[4], mats)) return 2;

  const std::vector<rmagine::Matrix4x4f> poses = warpsense::sweep_poses(mats[0], mats[1], k);
  if (poses.size() != k || !write_all(prefix + ".poses", poses.data(), poses.size() * sizeof(rmagine::Matrix4x4f))) return 3;

  cuda::ScanPreprocessor pre(n);
  size_t m = pre.preprocess_sweep(cloud.data(), n, stride, poses, cuda::ScanPreprocessor::by_index(columns, ring_major != 0), res);
  std::vector<rmagine::Pointi> pts = pre.download();
  if (pts.size() != m || !write_all(prefix + ".index", pts.data(), pts.size() * sizeof(rmagine::Pointi))) return 3;
  printf("index %zu\n", m);

  m = pre.preprocess_sweep(cloud.data(), n, stride, poses, cuda::ScanPreprocessor::by_time(time_field), res);
  pts = pre.download();
  if (pts.size() != m || !write_all(prefix + ".time", pts.data(), pts.size() * sizeof(rmagine::Pointi))) return 3;
  printf("time %zu\n", m);

  // (a refusal ends the process, as every failed WS_CHECK does -- the reference's print-and-exit; tests/test_gpu_sweep.py covers them)
  printf("again %zu\n", pre.preprocess_sweep(cloud.data(), n, stride, poses, cuda::ScanPreprocessor::by_index(columns, ring_major != 0), res));
  return 0;
}
