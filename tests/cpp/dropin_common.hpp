// dropin_common.hpp — what the C++ drop-in programs of this directory share: the digest they print for the Python tests to compare
// with the bytes of the Python route (query_model.fnv1a in tests/), and the reader of a whole binary file into a sized vector.
#pragma once
#include <cstddef>
#include <cstdio>
#include <vector>

static inline unsigned long long fnv1a(const void *data, size_t bytes)
{
  unsigned long long h = 1469598103934665603ull;
  const unsigned char *p = static_cast<const unsigned char *>(data);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

template <typename T>
static bool read_all(const char *path, std::vector<T> &v)
{
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  const bool ok = fread(v.data(), sizeof(T), v.size(), f) == v.size();
  fclose(f);
  return ok;
}
