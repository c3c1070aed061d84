// store_dropin.cpp — warpsense::DeviceGlobalMap and MappingNode::shift_map_device (include/warpsense_hip/app.hpp) from C++: a walk
// read from a file -- boxes written into the window, shifts through the device global map -- then a digest of the window and of
// every chunk in key order, and the same after write_back() into the host global map, for tests/test_gpu_store_dropin.py.
//   store_dropin walk.bin sx sy sz resolution tau max_weight segment_chunks
// walk.bin, int32 words: 1 lo[3] hi[3] words[voxels of the box] | 2 new_pos[3] | 0
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "warpsense_hip/app.hpp"

// position-weighted sum modulo 2^64: a dropped, swapped or misplaced word shows
static unsigned long long digest(const uint32_t *w, size_t n)
{
  unsigned long long h = 0;
  for (size_t i = 0; i < n; ++i) h += (unsigned long long)w[i] * (2ull * i + 1ull);
  return h;
}

int main(int argc, char **argv)
{
  if (argc < 9) return 2;
  const int sx = atoi(argv[2]), sy = atoi(argv[3]), sz = atoi(argv[4]);
  cuda::HotPathParams hot;
  hot.map_resolution = atoi(argv[5]);
  hot.tau = atoi(argv[6]);
  hot.max_weight = atoi(argv[7]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> script;
  for (int32_t v; fread(&v, sizeof v, 1, f) == 1;) script.push_back(v);
  fclose(f);

  warpsense::GlobalMap global((int16_t)hot.tau, 0);
  warpsense::LocalMap local(sx, sy, sz, global);
  warpsense::MappingNode node(hot, local);
  warpsense::DeviceGlobalMap store(global.get_default_tsdf_entry(), 0, (uint32_t)atoi(argv[8]));
  node.attach(&store);
  auto &avg = node.gpu().tsdf().avg_map();
  std::vector<TSDFEntry> box;
  size_t i = 0;
  int shifts = 0;
  while (i < script.size() && script[i] != 0)
  {
    if (script[i] == 1)
    {
      const rmagine::Pointi lo(script[i + 1], script[i + 2], script[i + 3]), hi(script[i + 4], script[i + 5], script[i + 6]);
      const size_t n = (size_t)(hi.x - lo.x + 1) * (size_t)(hi.y - lo.y + 1) * (size_t)(hi.z - lo.z + 1);
      if (i + 7 + n > script.size()) return 3;
      box.resize(n);
      for (size_t k = 0; k < n; ++k) box[k].raw((uint32_t)script[i + 7 + k]);
      avg.insert_box(lo, hi, box);
      i += 7 + n;
    }
    else if (script[i] == 2)
    {
      node.shift_map_device(rmagine::Pointi(script[i + 1], script[i + 2], script[i + 3]));
      ++shifts;
      i += 4;
    }
    else
      return 3;
  }
  node.download();
  const rmagine::Pointi &pos = local.get_pos(), &off = local.get_offset();
  printf("shifts %d\n", shifts);
  printf("window %d %d %d %d %d %d %016llx\n", pos.x, pos.y, pos.z, off.x, off.y, off.z,
         digest(reinterpret_cast<const uint32_t *>(local.data().data()), local.data().size()));
  std::vector<TSDFEntry::RawType> chunk;
  for (const auto &key : store.keys())
  {
    if (!store.chunk(key, chunk)) return 4;
    printf("chunk %d %d %d %016llx\n", key[0], key[1], key[2], digest(chunk.data(), chunk.size()));
  }
  // write_back through the store: the host global map holds the store's chunks, the window's voxels in them
  node.write_back();
  for (const auto &key : store.keys())
  {
    if (!global.has_chunk(key)) return 5;
    printf("host %d %d %d %016llx\n", key[0], key[1], key[2], digest(global.activate_chunk(key).data(), warpsense::DeviceGlobalMap::CHUNK_WORDS));
  }
  printf("host_chunks %zu\n", global.active_chunks());
  return 0;
}
