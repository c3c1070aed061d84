// store_list_units.hip — the chunk-list core of the store's host code (ws_store_list.h) against brute-force restatements: the live
// box and the z range as a min / max over all chunks in 64 bits, the neighbour positions by linear search, the counts {B, N, P, n}
// of the word-space tables by counting, ChunkRange::key by a triple loop.  Host code only: no HIP call, no device needed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ws_internal.h"
#include "ws_store_list.h"

using namespace ws;

#define EXPECT(cond)                                       \
  do                                                       \
  {                                                        \
    if (!(cond))                                           \
    {                                                      \
      printf("%s: %s (line %d)\n", what, #cond, __LINE__); \
      return 1;                                            \
    }                                                      \
  } while (0)

typedef std::vector<StoreRaySlot> List;
static const uint32_t GUARD = 0xdeadbeefu;
static const int32_t KEY_MIN = -33554432, KEY_MAX = 33554431; // floor(INT32_MIN / 64), floor(INT32_MAX / 64)

static int64_t key_of(const StoreRaySlot &e, int k) { return k == 0 ? e.cx : k == 1 ? e.cy : e.cz; }

static int check_boxes(const char *what, const List &l, const int32_t lo[3], const int32_t hi[3])
{
  int64_t mn[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, mx[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (const StoreRaySlot &e : l)
    for (int k = 0; k < 3; ++k) mn[k] = std::min(mn[k], key_of(e, k) * 64), mx[k] = std::max(mx[k], key_of(e, k) * 64 + 63);
  int32_t blo[3], bhi[3];
  store_live_box(l, lo, hi, blo, bhi);
  for (int k = 0; k < 3; ++k)
  {
    EXPECT((int64_t)blo[k] == std::max<int64_t>(mn[k], lo[k]));
    EXPECT((int64_t)bhi[k] == std::min<int64_t>(mx[k], hi[k]));
    if (l.empty()) EXPECT(blo[k] > bhi[k]);
  }
  int32_t zlo = 7, zhi = 7;
  store_z_range(l, lo[2], hi[2], &zlo, &zhi);
  if (l.empty()) EXPECT(zlo == 1 && zhi == 0);
  else EXPECT((int64_t)zlo == std::max<int64_t>(mn[2], lo[2]) && (int64_t)zhi == std::min<int64_t>(mx[2], hi[2]));
  return 0;
}

static int check_tables(const char *what, const List &l)
{
  const size_t n = l.size();
  for (size_t i = 1; i < n; ++i) EXPECT((StoreKey{l[i - 1].cx, l[i - 1].cy, l[i - 1].cz} < StoreKey{l[i].cx, l[i].cy, l[i].cz})); // (the test's own list)
  EXPECT(store_word_table_bytes(n) == 32 * n);
  std::vector<uint32_t> grp(8 * n + 4, GUARD);
  store_word_tables(l, grp.data());
  for (size_t i = 0; i < n; ++i)
  {
    uint32_t B = 0, N = 0, P = 0, m = 0;
    for (size_t j = 0; j < n; ++j)
    {
      B += l[j].cx < l[i].cx;
      N += l[j].cx == l[i].cx;
      P += l[j].cx == l[i].cx && l[j].cy < l[i].cy;
      m += l[j].cx == l[i].cx && l[j].cy == l[i].cy;
    }
    EXPECT(grp[4 * i] == B && grp[4 * i + 1] == N && grp[4 * i + 2] == P && grp[4 * i + 3] == m);
    const uint32_t *key = &grp[4 * n + 4 * i];
    EXPECT((int32_t)key[0] == l[i].cx && (int32_t)key[1] == l[i].cy && (int32_t)key[2] == l[i].cz && key[3] == l[i].slot);
  }
  for (size_t i = 8 * n; i < grp.size(); ++i) EXPECT(grp[i] == GUARD);

  int32_t off27[27][3];
  for (int c = 0; c < 27; ++c) off27[c][0] = c / 9 - 1, off27[c][1] = c / 3 % 3 - 1, off27[c][2] = c % 3 - 1;
  static const int32_t off6[6][3] = {{-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
  for (int pass = 0; pass < 2; ++pass)
  {
    const int n_off = pass ? 6 : 27;
    const int32_t(*off)[3] = pass ? off6 : off27;
    std::vector<uint32_t> nb(n_off * n + 4, GUARD);
    store_neighbour_positions(l, off, n_off, nb.data());
    for (size_t i = 0; i < n; ++i)
      for (int d = 0; d < n_off; ++d)
      {
        uint32_t at = 0xffffffffu;
        for (size_t j = 0; j < n; ++j)
          if (key_of(l[j], 0) == key_of(l[i], 0) + off[d][0] && key_of(l[j], 1) == key_of(l[i], 1) + off[d][1] && key_of(l[j], 2) == key_of(l[i], 2) + off[d][2])
            at = (uint32_t)j;
        EXPECT(nb[n_off * i + d] == at);
      }
    for (size_t i = (size_t)n_off * n; i < nb.size(); ++i) EXPECT(nb[i] == GUARD);
    if (!pass)
      for (size_t i = 0; i < n; ++i) EXPECT(nb[27 * i + 13] == (uint32_t)i); // offset (0, 0, 0): the chunk itself
  }
  return 0;
}

static int check_list(const char *what, const List &l)
{
  if (check_tables(what, l)) return 1;
  const int32_t all_lo[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, all_hi[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
  if (check_boxes(what, l, all_lo, all_hi)) return 1;
  const int32_t some_lo[3] = {-100, -100, -100}, some_hi[3] = {500, 100, 70};
  return check_boxes(what, l, some_lo, some_hi);
}

static int check_range(const char *what)
{
  EXPECT(chunk_of(INT32_MIN) == KEY_MIN && chunk_of(INT32_MAX) == KEY_MAX);
  EXPECT(chunk_of(-65) == -2 && chunk_of(-64) == -1 && chunk_of(-1) == -1 && chunk_of(0) == 0 && chunk_of(63) == 0 && chunk_of(64) == 1);
  const int32_t lo[3] = {-130, -1, -65}, hi[3] = {70, 64, 0};
  const ChunkRange cr(lo, hi);
  EXPECT(cr.c0[0] == -3 && cr.c0[1] == -1 && cr.c0[2] == -2);
  EXPECT(cr.nc[0] == 5 && cr.nc[1] == 3 && cr.nc[2] == 3 && cr.n == 45);
  size_t i = 0;
  for (int32_t x = -3; x <= 1; ++x)
    for (int32_t y = -1; y <= 1; ++y)
      for (int32_t z = -2; z <= 0; ++z, ++i) EXPECT((cr.key(i) == StoreKey{x, y, z}));
  EXPECT(i == cr.n);
  const int32_t all_lo[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, all_hi[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
  const ChunkRange all(all_lo, all_hi);
  EXPECT(all.c0[0] == KEY_MIN && all.nc[0] == 1 << 26);
  return 0;
}

static int check_limit(const char *what)
{
  EXPECT(STORE_LIST_LIMIT == (size_t)1 << 19);
  const size_t places = store_ray_table_slots(STORE_LIST_LIMIT - 1), bytes = places * sizeof(StoreRaySlot);
  EXPECT(places == (size_t)1 << 20 && bytes / sizeof(StoreRaySlot) == places); // no wrap in size_t
  EXPECT(bytes <= 0xffffffffu && (size_t)(uint32_t)places == places && (uint32_t)places - 1u == 0xfffffu);
  EXPECT((uint64_t)(STORE_LIST_LIMIT - 1) * 4096u < ((uint64_t)1 << 31)); // the word space of the listed chunks
  return 0;
}

int main()
{
  if (check_range("ChunkRange") || check_limit("the listing limit")) return 1;

  const List none;
  if (check_list("an empty list", none)) return 1;

  const List one = {{-1, 2, -3, 17}};
  if (check_list("one chunk", one)) return 1;

  List block; // 3 x 3 x 3 around (5, -2, 0) without its centre
  for (int32_t x = 4; x <= 6; ++x)
    for (int32_t y = -3; y <= -1; ++y)
      for (int32_t z = -1; z <= 1; ++z)
        if (x != 5 || y != -2 || z != 0) block.push_back({x, y, z, (uint32_t)block.size() * 3u + 1u});
  if (check_list("a block without its centre", block)) return 1;

  const List runs = {{-1, 0, 0, 9}, {-1, 0, 1, 8}, {-1, 0, 2, 7}, {-1, 3, 7, 6},                                         // cx -1: runs of 3 and 1
                     {4, -2, 0, 5}, {4, -1, 0, 4}, {4, -1, 1, 3}, {4, 5, -9, 2}, {4, 5, -8, 1}, {4, 5, -7, 0}, {4, 5, -6, 40}}; // cx 4: runs of 1, 2 and 4
  if (check_list("two cx groups with unequal runs", runs)) return 1;

  const List ends = {{KEY_MIN, KEY_MIN, KEY_MIN, 0}, {KEY_MIN, KEY_MIN, KEY_MIN + 1, 1}, {KEY_MIN, 0, KEY_MAX, 2}, {KEY_MIN + 1, KEY_MIN, KEY_MIN, 3},
                     {0, 0, 0, 4}, {KEY_MAX - 1, KEY_MAX, KEY_MAX, 5}, {KEY_MAX, KEY_MAX, KEY_MAX - 1, 6}, {KEY_MAX, KEY_MAX, KEY_MAX, 7}};
  if (check_list("both ends of the key domain", ends)) return 1;

  // the block's bounding box is [256, 447] x [-192, -1] x [-64, 127]
  const int32_t cut_lo[3] = {300, -100, -10}, cut_hi[3] = {400, -50, 100};
  if (check_boxes("a box that cuts every side", block, cut_lo, cut_hi)) return 1;
  {
    const char *what = "a box that cuts every side";
    int32_t blo[3], bhi[3];
    store_live_box(block, cut_lo, cut_hi, blo, bhi);
    for (int k = 0; k < 3; ++k) EXPECT(blo[k] == cut_lo[k] && bhi[k] == cut_hi[k]);
  }
  const int32_t miss_lo[3] = {300, 0, -10}, miss_hi[3] = {400, 50, 100}; // y misses [-192, -1]
  if (check_boxes("a box that misses on y", block, miss_lo, miss_hi)) return 1;
  {
    const char *what = "a box that misses on y";
    int32_t blo[3], bhi[3];
    store_live_box(block, miss_lo, miss_hi, blo, bhi);
    EXPECT(blo[0] <= bhi[0] && blo[1] > bhi[1] && blo[2] <= bhi[2]);
  }
  printf("ok\n");
  return 0;
}
