// api_store.hip — the chunk store, the global map in device memory (ws_store_*, ws_shift_device; kernels in map_store.hip): directory,
// segments and slot tables, the box transfers between a map's window and the chunks, and the store's surface cloud, mesh, ray cast and
// distance field, which run the host cores of ws_api.h over the chunks a call lists (store_surface.hip, store_mesh.hip,
// store_raycast.hip, store_distance.hip), the two calls that write one store from another: ws_store_fuse (store_fuse.hip) and
// ws_store_coarsen (store_coarsen.hip), and the call that compares one store with another: ws_store_changes (store_changes.hip).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <functional>
#include <new>
#include <set>

#include "ws_api.h"
#include "ws_changes.h"
#include "ws_coarsen.h"
#include "ws_fuse.h"

using namespace ws;

// ---- the chunk store: the global map in device memory (map_store.hip)
namespace
{
inline int32_t chunk_of(int32_t v) { return v >= 0 ? v / STORE_CS : -((-(int64_t)v + STORE_CS - 1) / STORE_CS); } // floor(v / 64)

// the chunks an inclusive world box overlaps: first key and count per axis
struct ChunkRange
{
  int32_t c0[3], nc[3];
  size_t n;
  ChunkRange(const int32_t lo[3], const int32_t hi[3])
  {
    n = 1;
    for (int k = 0; k < 3; ++k)
    {
      c0[k] = chunk_of(lo[k]);
      nc[k] = chunk_of(hi[k]) - c0[k] + 1;
      n *= (size_t)nc[k];
    }
  }
  StoreKey key(size_t i) const // x major, like the slot table
  {
    const size_t plane = (size_t)nc[1] * (size_t)nc[2];
    return {c0[0] + (int32_t)(i / plane), c0[1] + (int32_t)(i % plane / (size_t)nc[2]), c0[2] + (int32_t)(i % (size_t)nc[2])};
  }
};

uint64_t store_capacity(const ws_store *st) { return (uint64_t)st->segs.size() << st->seg_shift; }

uint32_t *store_slot_ptr(const ws_store *st, uint32_t slot)
{
  return st->seg_ptr[slot >> st->seg_shift] + (size_t)(slot & ((1u << st->seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
}

// Segments for `chunks` chunks in all.  Adding one waits for the stream (the kernels in flight read the old segment table); a failed
// allocation gives back what this call added, so the store is as it was.
int store_grow(ws_store *st, uint64_t chunks)
{
  if (chunks <= store_capacity(st)) return WS_OK;
  if (chunks >= 0x7fffffffull) return invalid("ws_store: more than 2^31 - 1 chunks");
  const size_t had = st->segs.size(), want = (size_t)((chunks + (1ull << st->seg_shift) - 1) >> st->seg_shift);
  WS_HIP(hipStreamSynchronize(st->ctx->stream));
  int rc = WS_OK;
  DevBuf tab;
  for (size_t i = had; i < want && rc == WS_OK; ++i)
  {
    st->segs.emplace_back();
    rc = st->segs.back().alloc((size_t)STORE_CHUNK_WORDS << st->seg_shift, sizeof(uint32_t));
    if (rc == WS_OK) st->seg_ptr.push_back(st->segs.back().as<uint32_t>());
  }
  if (rc == WS_OK) rc = tab.alloc(want, sizeof(uint32_t *));
  if (rc == WS_OK)
  {
    const hipError_t e = hipMemcpy(tab.p, st->seg_ptr.data(), want * sizeof(uint32_t *), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy (segment table)", __FILE__, __LINE__);
  }
  if (rc != WS_OK)
  {
    tab.release();
    for (size_t i = had; i < st->segs.size(); ++i) st->segs[i].release();
    st->segs.resize(had);
    st->seg_ptr.resize(had);
    return rc;
  }
  st->seg_tab.release();
  st->seg_tab = tab; // (DevBuf is a plain pair: the store owns the new table now)
  return WS_OK;
}

// chunks that can still be created without a new segment / at all
uint64_t store_unused(const ws_store *st) { return st->free_slots.size() + (store_capacity(st) - st->next_slot); }

} // namespace

// (declared in ws_api.h: api_pack.hip hands out slots and takes tables by the same rules)
namespace ws
{
// Room for `fresh` more chunks: WS_ERR_CAPACITY beyond max_chunks, segments where they are missing.  Nothing else changes.
int store_make_room(ws_store *st, uint64_t fresh, const char *name)
{
  if (st->max_chunks && st->dir.size() + fresh > st->max_chunks)
  {
    set_error(std::string(name) + ": the store would hold more than max_chunks chunks");
    return WS_ERR_CAPACITY;
  }
  if (fresh <= store_unused(st)) return WS_OK;
  return store_grow(st, (uint64_t)st->next_slot + (fresh - st->free_slots.size()));
}

uint32_t store_take_slot(ws_store *st) // (store_make_room has been asked)
{
  if (!st->free_slots.empty())
  {
    const uint32_t s = st->free_slots.back();
    st->free_slots.pop_back();
    return s;
  }
  return st->next_slot++;
}
} // namespace ws

namespace
{

// room for n words in one slot table (pinned + device) and its event
int store_table_reserve(ws_store::Table &t, size_t n)
{
  if (!t.done) WS_HIP(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  if (n <= t.host.cap) return WS_OK;
  WS_TRY(t.host.alloc(n, sizeof(uint32_t), HostBlock::PINNED));
  return t.dev.alloc(n, sizeof(uint32_t));
}

} // namespace

namespace ws
{
// The next slot table of the ring, for n words: waits only for the launch that read this table STORE_TABLES calls ago.  The tables are
// sized when the store is created (STORE_TABLE_WORDS); a box that overlaps more chunks makes one grow here, which allocates.
int store_table(ws_store *st, size_t n, ws_store::Table **out)
{
  ws_store::Table &t = st->tab[st->tab_next];
  st->tab_next = (st->tab_next + 1) % STORE_TABLES;
  if (t.used) WS_HIP(hipEventSynchronize(t.done));
  t.used = false;
  WS_TRY(store_table_reserve(t, n > t.host.cap ? n + n / 8 : n));
  *out = &t;
  return WS_OK;
}
} // namespace ws

namespace
{

// One launch: the box of `which` (window `par`) into the chunks or back.  The directory already holds every chunk a save needs (a
// save table never holds STORE_ABSENT: the kernel would read that word as slot 2^31 - 1, flagged new).  A chunk this call created
// and nothing has written yet is flagged STORE_NEW by the first save that meets it -- that launch writes it whole -- and is absent
// to a load: a later slab of the same shift will write it.
int store_enqueue(ws_store *st, ws_map *m, const MapParams &par, int which, const int32_t lo[3], const int32_t hi[3], bool save)
{
  const ChunkRange cr(lo, hi);
  ws_store::Table *t = nullptr;
  WS_TRY(store_table(st, cr.n, &t));
  uint32_t *w = t->host.as<uint32_t>();
  bool any_new = false;
  for (size_t i = 0; i < cr.n; ++i)
  {
    const auto it = st->dir.find(cr.key(i));
    if (it == st->dir.end() || (!save && !it->second.written))
    {
      if (save)
      {
        set_error("ws_store: internal error, a save met a chunk without a slot");
        return WS_ERR_INTERNAL;
      }
      w[i] = STORE_ABSENT;
      continue;
    }
    w[i] = it->second.slot | (it->second.written ? 0u : STORE_NEW);
    any_new |= !it->second.written;
    it->second.written = true;
  }
  hipStream_t s = st->ctx->stream;
  WS_HIP(hipMemcpyAsync(t->dev.p, t->host.p, cr.n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  WS_TRY(launch_store_copy(st, m, par, which, lo, hi, cr.c0, cr.nc, t->dev.as<uint32_t>(), save, any_new, s));
  WS_HIP(hipEventRecord(t->done, s));
  t->used = true;
  return WS_OK;
}

// the keys of `lo .. hi` the directory does not hold yet, into `fresh` (a set: each once)
void store_missing(const ws_store *st, const int32_t lo[3], const int32_t hi[3], std::set<StoreKey> &fresh)
{
  const ChunkRange cr(lo, hi);
  for (size_t i = 0; i < cr.n; ++i)
  {
    const StoreKey key = cr.key(i);
    if (!st->dir.count(key)) fresh.insert(key);
  }
}

// gives the chunks of `fresh` their slots (unwritten) / takes them back after a failure half-way
void store_admit(ws_store *st, const std::set<StoreKey> &fresh)
{
  for (const StoreKey &k : fresh) st->dir[k] = ws_store::Entry{store_take_slot(st), false};
}
} // namespace
void ws::store_evict(ws_store *st, const std::set<StoreKey> &fresh)
{
  for (const StoreKey &k : fresh)
  {
    const auto it = st->dir.find(k);
    if (it == st->dir.end()) continue;
    st->free_slots.push_back(it->second.slot);
    st->dir.erase(it);
  }
}
namespace
{

int store_args(const ws_store *st, const ws_map *m, int which, const char *name)
{
  if (!st || !m || (which != WS_MAP_AVG && which != WS_MAP_NEW)) return invalid((std::string(name) + ": bad argument").c_str());
  if (st->ctx != m->ctx) return invalid((std::string(name) + ": the store belongs to another context").c_str());
  return WS_OK;
}
} // namespace

int ws_store_create(ws_context *ctx, uint32_t fill_entry, uint64_t max_chunks, uint32_t segment_chunks, ws_store **out)
{
  if (!ctx || !out) return invalid("ws_store_create: NULL argument");
  if (segment_chunks > (1u << 16)) return invalid("ws_store_create: segment_chunks beyond 65 536 (64 GB per segment)");
  ws_store *st = new (std::nothrow) ws_store();
  if (!st) return invalid("ws_store_create: out of host memory");
  st->ctx = ctx;
  st->fill = fill_entry;
  st->max_chunks = max_chunks;
  // the default: 256 chunks = 256 MB per segment; any other value is rounded up to a power of two (the kernels shift and mask)
  const uint32_t want = segment_chunks ? segment_chunks : 256u;
  while ((1u << st->seg_shift) < want) ++st->seg_shift;
  // the slot tables and their events now: no shift allocates them
  for (ws_store::Table &t : st->tab)
  {
    const int rc = store_table_reserve(t, STORE_TABLE_WORDS);
    if (rc != WS_OK)
    {
      st->release();
      delete st;
      return rc;
    }
  }
  *out = st;
  return WS_OK;
}

int ws_store_destroy(ws_store *st)
{
  if (!st) return WS_OK;
  (void)hipStreamSynchronize(st->ctx->stream);
  st->release();
  delete st;
  return WS_OK;
}

int ws_store_reserve(ws_store *st, uint64_t chunks)
{
  if (!st) return invalid("ws_store_reserve: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  if (st->max_chunks && chunks > st->max_chunks) chunks = st->max_chunks;
  return store_grow(st, chunks);
}

int ws_store_count(const ws_store *st, uint64_t *chunks, uint64_t *capacity_chunks)
{
  if (!st) return invalid("ws_store_count: store is NULL");
  std::lock_guard<std::mutex> lock(const_cast<ws_store *>(st)->mu);
  if (chunks) *chunks = st->dir.size();
  if (capacity_chunks) *capacity_chunks = store_capacity(st);
  return WS_OK;
}

int ws_store_keys(const ws_store *st, int32_t *keys, size_t capacity, size_t *n_out)
{
  if (!st || (!keys && capacity)) return invalid("ws_store_keys: bad argument");
  std::lock_guard<std::mutex> lock(const_cast<ws_store *>(st)->mu);
  size_t i = 0;
  for (const auto &kv : st->dir)
  {
    if (i >= capacity) break;
    for (int k = 0; k < 3; ++k) keys[3 * i + k] = kv.first[k];
    ++i;
  }
  if (n_out) *n_out = st->dir.size();
  return WS_OK;
}

int ws_store_has(const ws_store *st, const int32_t key[3])
{
  if (!st || !key) return 0;
  std::lock_guard<std::mutex> lock(const_cast<ws_store *>(st)->mu);
  return st->dir.count({key[0], key[1], key[2]}) ? 1 : 0;
}

int ws_store_get_chunk(ws_store *st, const int32_t key[3], uint32_t *host, int32_t *found)
{
  if (!st || !key || !host) return invalid("ws_store_get_chunk: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  const auto it = st->dir.find({key[0], key[1], key[2]});
  if (found) *found = it != st->dir.end();
  if (it == st->dir.end()) return WS_OK;
  WS_HIP(hipMemcpyAsync(host, store_slot_ptr(st, it->second.slot), (size_t)STORE_CHUNK_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st->ctx->stream));
  WS_HIP(hipStreamSynchronize(st->ctx->stream));
  return WS_OK;
}

int ws_store_put_chunk(ws_store *st, const int32_t key[3], const uint32_t *host)
{
  if (!st || !key || !host) return invalid("ws_store_put_chunk: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  const StoreKey k = {key[0], key[1], key[2]};
  auto it = st->dir.find(k);
  if (it == st->dir.end())
  {
    WS_TRY(store_make_room(st, 1, "ws_store_put_chunk"));
    it = st->dir.emplace(k, ws_store::Entry{store_take_slot(st), true}).first;
  }
  WS_HIP(hipMemcpyAsync(store_slot_ptr(st, it->second.slot), host, (size_t)STORE_CHUNK_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, st->ctx->stream));
  WS_HIP(hipStreamSynchronize(st->ctx->stream)); // the host buffer may be reused by the caller
  return WS_OK;
}

int ws_store_drop_chunk(ws_store *st, const int32_t key[3])
{
  if (!st || !key) return invalid("ws_store_drop_chunk: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  const auto it = st->dir.find({key[0], key[1], key[2]});
  if (it == st->dir.end()) return invalid("ws_store_drop_chunk: the store has no such chunk");
  // whatever still reads or writes the slot was enqueued before whatever the next owner of the slot enqueues
  st->free_slots.push_back(it->second.slot);
  st->dir.erase(it);
  return WS_OK;
}

const uint32_t *ws_store_chunk_dev(const ws_store *st, const int32_t key[3])
{
  if (!st || !key) return nullptr;
  std::lock_guard<std::mutex> lock(const_cast<ws_store *>(st)->mu);
  const auto it = st->dir.find({key[0], key[1], key[2]});
  return it == st->dir.end() ? nullptr : store_slot_ptr(st, it->second.slot);
}

static int store_box(ws_store *st, ws_map *m, int which, const int32_t lo[3], const int32_t hi[3], bool save, const char *name)
{
  WS_TRY(store_args(st, m, which, name));
  WS_SETTLE(m);
  std::lock_guard<std::mutex> lock(st->mu);
  int32_t l[3], ext[3];
  WS_TRY(resolve_box(m, which, lo, hi, false, name, l, ext));
  WS_TRY(st->timer[0].arm());
  st->timer[1].marked = st->timer[2].marked = 0;
  std::set<StoreKey> fresh;
  if (save)
  {
    store_missing(st, lo, hi, fresh);
    WS_TRY(store_make_room(st, fresh.size(), name));
    store_admit(st, fresh); // (nothing below can fail before the launch is being enqueued)
  }
  st->timer[0].mark(save ? 0 : 1, st->ctx->stream);
  const int rc = store_enqueue(st, m, m->par[which], which, lo, hi, save);
  st->timer[0].mark(save ? 1 : 2, st->ctx->stream);
  if (rc != WS_OK)
  {
    store_evict(st, fresh);
    return rc;
  }
  if (!save && which == WS_MAP_NEW) m->new_is_default = false;
  return WS_OK;
}

int ws_store_save_box(ws_store *st, ws_map *m, int which, const int32_t lo[3], const int32_t hi[3])
{
  return store_box(st, m, which, lo, hi, true, "ws_store_save_box");
}

int ws_store_load_box(ws_store *st, ws_map *m, int which, const int32_t lo[3], const int32_t hi[3])
{
  return store_box(st, m, which, lo, hi, false, "ws_store_load_box");
}

int ws_shift_device(ws_map *m, ws_store *st, const int32_t new_pos[3])
{
  WS_TRY(store_args(st, m, WS_MAP_AVG, "ws_shift_device"));
  if (!new_pos) return invalid("ws_shift_device: new_pos is NULL");
  std::unique_lock<std::mutex> lock(st->mu, std::defer_lock); // taken in ready(), after the refusals, and held to the end of the call
  ws_shift_plan_t plan;
  std::set<StoreKey> fresh; // the chunks this call has created
  hipStream_t s = m->ctx->stream;
  const int rc = run_shift(
      m, new_pos, "ws_shift_device", ": a shift of this map is in flight (ws_shift_end)", plan,
      [&]() -> int {
        lock.lock();
        for (QueryTimer &t : st->timer) WS_TRY(t.arm());
        // every chunk the leaving slabs of ALL axes create, before the first launch: a call that cannot get them changes nothing
        std::set<StoreKey> missing;
        for (int i = 0; i < plan.n; ++i) store_missing(st, plan.leave_lo[i], plan.leave_hi[i], missing);
        WS_TRY(store_make_room(st, missing.size(), "ws_shift_device"));
        store_admit(st, missing);
        fresh.swap(missing);
        return WS_OK;
      },
      [&](int i, const MapParams &par) -> int {
        st->timer[i].mark(0, s);
        const int rc_save = store_enqueue(st, m, par, WS_MAP_AVG, plan.leave_lo[i], plan.leave_hi[i], true);
        st->timer[i].mark(1, s);
        if (rc_save != WS_OK) st->timer[i].mark(2, s); // the step ends here, its load is never enqueued: close its second interval too
        return rc_save;
      },
      [&](int i, const MapParams &par) -> int {
        const int rc_load = store_enqueue(st, m, par, WS_MAP_AVG, plan.enter_lo[i], plan.enter_hi[i], false);
        st->timer[i].mark(2, s);
        return rc_load;
      },
      []() -> int { return WS_OK; });
  if (rc != WS_OK) store_evict(st, fresh); // (after a refusal, which holds no lock, `fresh` is empty)
  return rc;
}

int ws_store_chunks_of_box(const int32_t lo[3], const int32_t hi[3], int32_t *keys, size_t capacity, size_t *n_out)
{
  if (!lo || !hi || (!keys && capacity)) return invalid("ws_store_chunks_of_box: bad argument");
  for (int k = 0; k < 3; ++k)
    if (hi[k] < lo[k]) return invalid("ws_store_chunks_of_box: hi < lo");
  const ChunkRange cr(lo, hi);
  for (size_t i = 0; i < cr.n && i < capacity; ++i)
  {
    const StoreKey key = cr.key(i); // x major, z fastest: ascending (cx, cy, cz)
    for (int k = 0; k < 3; ++k) keys[3 * i + k] = key[k];
  }
  if (n_out) *n_out = cr.n;
  return WS_OK;
}

int ws_debug_store_timing(ws_store *st, int32_t enable, float ms_out[2])
{
  if (!st) return invalid("ws_debug_store_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  static const int pairs[2][2] = {{0, 1}, {1, 2}};
  float sum[2] = {0.f, 0.f};
  for (QueryTimer &t : st->timer)
  {
    float ms[2] = {0.f, 0.f};
    WS_TRY(t.read(ms_out ? ms : nullptr, pairs, 2, st->ctx->stream));
    sum[0] += ms[0], sum[1] += ms[1];
    t.set(enable);
  }
  if (ms_out) ms_out[0] = sum[0], ms_out[1] = sum[1];
  return WS_OK;
}

// ---- the surface cloud, the mesh, the ray cast and the distance field of the store: the rules and the host flow of ws_map_surface,
// ws_map_mesh, ws_map_raycast and ws_map_distance over the chunks, store_surface.hip, store_mesh.hip, store_raycast.hip and
// store_distance.hip (the semantics are stated in warpsense_hip.h)
namespace
{
// The box of a query, into l and h.  First the refusal of a box whose hi < lo, in the name of the entry point; then the store's lock,
// into `lock` for the rest of the call; then the box: the call's, or without one all of int32 where `everything` (a ray cast), else
// the bounding box of the present chunks (keys are floor(int32 / 64): 64 k + 63 fits), which leaves l > h in an empty store.
// (ws_store_raycast calls this among its argument checks: its later refusals return with the lock held until then.)
int store_query_box(ws_store *st, const char *name, const int32_t lo[3], const int32_t hi[3], bool everything, std::unique_lock<std::mutex> &lock, int32_t l[3],
                    int32_t h[3])
{
  for (int k = 0; k < 3 && lo; ++k)
    if (hi[k] < lo[k]) return invalid(std::string(name) + ": hi < lo");
  lock = std::unique_lock<std::mutex>(st->mu);
  for (int k = 0; k < 3; ++k) l[k] = lo ? lo[k] : everything ? INT32_MIN : INT32_MAX, h[k] = lo ? hi[k] : everything ? INT32_MAX : INT32_MIN;
  if (!lo && !everything)
    for (const auto &kv : st->dir)
      for (int k = 0; k < 3; ++k) l[k] = std::min(l[k], kv.first[k] * STORE_CS), h[k] = std::max(h[k], kv.first[k] * STORE_CS + STORE_CS - 1);
  return WS_OK;
}

// The written chunks a query lists, {cx, cy, cz, slot} ascending like the directory: those the box overlaps, or without a box
// (lo == NULL) all of them.  The directory is ordered by cx first and only the keys of the box's cx range are visited: nothing here
// follows the volume of the box.
void store_list(const ws_store *st, const int32_t *lo, const int32_t *hi, std::vector<StoreRaySlot> &listed)
{
  const auto put = [&](const StoreKey &key, const ws_store::Entry &e) { listed.push_back(StoreRaySlot{key[0], key[1], key[2], e.slot}); };
  listed.clear();
  if (!lo)
  {
    for (const auto &kv : st->dir)
      if (kv.second.written) put(kv.first, kv.second);
    return;
  }
  const ChunkRange cr(lo, hi);
  for (auto it = st->dir.lower_bound(StoreKey{cr.c0[0], INT32_MIN, INT32_MIN}); it != st->dir.end() && it->first[0] - cr.c0[0] < cr.nc[0]; ++it)
  {
    bool in = it->second.written;
    for (int k = 1; k < 3; ++k) in = in && it->first[k] >= cr.c0[k] && it->first[k] - cr.c0[k] < cr.nc[k];
    if (in) put(it->first, it->second);
  }
}

// The lookup of the listed chunks (store_ray_table_fill) in the pinned table of a ray cast or a distance call: its places, and the
// fill.  A table that is too small is replaced with its device twin: the caller has synchronised the stream then.
size_t store_lookup_places(size_t n) { return n ? store_ray_table_slots(n) : 0; }
int store_lookup_fill(HostBlock &host, DevBuf &dev, const std::vector<StoreRaySlot> &listed)
{
  const size_t places = store_lookup_places(listed.size());
  if (places > host.cap)
  {
    WS_TRY(host.alloc(places, sizeof(StoreRaySlot), HostBlock::PINNED));
    WS_TRY(dev.alloc(places, sizeof(StoreRaySlot)));
  }
  if (!listed.empty()) store_ray_table_fill(listed.data(), listed.size(), host.as<StoreRaySlot>());
  return WS_OK;
}

// The lookup of EVERY written chunk of `src` (store_ray_table_fill), filled into the next slot table of its ring: what a call that
// samples one store on the lattice of another reads it through (ws_store_fuse, ws_store_changes).  `places`: the table's places;
// the caller enqueues the upload of places * sizeof(StoreRaySlot) bytes and records the table's event behind the last launch that
// reads it.  2^19 chunks or more: WS_ERR_RANGE in the name of the entry point, with `too_many`.  An empty store gives a table
// without a chunk: every lookup is absent.
int store_lookup_plan(ws_store *src, const char *name, const char *too_many, ws_store::Table **ts, size_t *places)
{
  std::vector<StoreRaySlot> listed;
  store_list(src, nullptr, nullptr, listed);
  if (listed.size() >= (1u << 19)) return range_error(name, too_many);
  *places = store_ray_table_slots(listed.size());
  WS_TRY(store_table(src, *places * 4, ts));
  store_ray_table_fill(listed.data(), listed.size(), (*ts)->host.as<StoreRaySlot>());
  return WS_OK;
}

// A store call waits for the stream even after a failed enqueue (whose error it reports): the pinned table of the call must be free
// again when the call returns.
int store_enqueued(const ws_store *st, int rc)
{
  if (rc != WS_OK) (void)hipStreamSynchronize(st->ctx->stream);
  return rc;
}

// Room for `need` bytes of chunk tables of a surface or mesh call, pinned and on the device (`want` where they have to grow, which
// waits for the stream: the kernels in flight read the old table)
int store_tables_reserve(ws_store *st, HostBlock &host, DevBuf &dev, size_t need, size_t want)
{
  if (need <= host.cap && need <= dev.cap) return WS_OK; // (both: a failed allocation of the second leaves the first one grown)
  WS_HIP(hipStreamSynchronize(st->ctx->stream));
  WS_TRY(host.alloc(want, 1, HostBlock::PINNED));
  return dev.alloc(want, 1);
}

// The word-space tables of the n listed chunks (0 < n < 2^19) at `grp`, store_word_table_bytes(n): per chunk the four counts
// {B, N, P, n} that place its 4096 words in world order (ws_store_words.h), then its key and slot
void store_word_tables(const std::vector<StoreRaySlot> &listed, uint32_t *grp)
{
  const size_t n = listed.size();
  std::memcpy(grp + 4 * n, listed.data(), n * sizeof(StoreRaySlot)); // {cx, cy, cz, slot} per chunk
  for (size_t b = 0; b < n;) // the chunks of one cx: [b, e)
  {
    size_t e = b;
    while (e < n && listed[e].cx == listed[b].cx) ++e;
    for (size_t p = b; p < e;) // the chunks of one (cx, cy): [p, q)
    {
      size_t q = p;
      while (q < e && listed[q].cy == listed[p].cy) ++q;
      for (size_t i = p; i < q; ++i)
        grp[4 * i + 0] = (uint32_t)b, grp[4 * i + 1] = (uint32_t)(e - b), grp[4 * i + 2] = (uint32_t)(p - b), grp[4 * i + 3] = (uint32_t)(q - p);
      p = q;
    }
    b = e;
  }
}

// The tables of a mesh call over the n listed chunks (0 < n < 2^19), into st->mesh.table_host: the word-space tables, and the list
// positions of every chunk's 26 neighbours.  Everything is O(n log n).
int store_mesh_tables(ws_store *st, const std::vector<StoreRaySlot> &listed)
{
  const size_t n = listed.size();
  WS_TRY(store_tables_reserve(st, st->mesh.table_host, st->mesh.table_dev, store_mesh_table_bytes(n), store_mesh_table_bytes(n + n / 8)));
  uint32_t *grp = st->mesh.table_host.as<uint32_t>();
  uint32_t *nb = grp + 8 * n;
  store_word_tables(listed, grp);
  const auto before = [](const StoreRaySlot &e, const StoreKey &k) { return StoreKey{e.cx, e.cy, e.cz} < k; };
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 27; ++c)
    {
      // (keys are floor(int32 / 64): a step of one cannot overflow)
      const StoreKey k = {listed[i].cx + c / 9 - 1, listed[i].cy + c / 3 % 3 - 1, listed[i].cz + c % 3 - 1};
      const auto it = std::lower_bound(listed.begin(), listed.end(), k, before);
      const bool found = it != listed.end() && it->cx == k[0] && it->cy == k[1] && it->cz == k[2];
      nb[27 * i + c] = found ? (uint32_t)(it - listed.begin()) : 0xffffffffu;
    }
  return WS_OK;
}
} // namespace

int ws_store_surface(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t band, int32_t tau, int32_t map_resolution, uint32_t flags, size_t *n_out)
{
  if (!st || (flags & ~WS_SURFACE_MARKER) || ((lo == nullptr) != (hi == nullptr)) || tau <= 0 || map_resolution <= 0) return invalid("ws_store_surface: bad argument");
  std::unique_lock<std::mutex> lock;
  StoreSurfCall c;
  WS_TRY(store_query_box(st, "ws_store_surface", lo, hi, false, lock, c.lo, c.hi));
  ws_store::Surface &q = st->surf;
  std::vector<StoreRaySlot> listed;
  if (c.lo[0] <= c.hi[0]) store_list(st, c.lo, c.hi, listed); // (else: no box and no chunk)
  if (listed.size() >= (1u << 19)) return range_error("ws_store_surface", ": the box overlaps 2^19 present chunks or more (4096 words each must stay below 2^31)");
  WS_TRY(q.timer.arm());
  if (listed.empty()) // an empty store, or the box meets no present chunk
  {
    q.n = 0, q.has_marker = false;
    if (n_out) *n_out = 0;
    return WS_OK;
  }
  c.n_chunks = (uint32_t)listed.size();
  c.band = band <= 0 ? tau : band, c.tau = tau, c.res = map_resolution;
  const bool marker = (flags & WS_SURFACE_MARKER) != 0;
  const size_t n_words = (size_t)c.n_chunks * 4096u, n = listed.size();
  WS_TRY(store_tables_reserve(st, q.table_host, q.table_dev, store_word_table_bytes(n), store_word_table_bytes(n + n / 8)));
  store_word_tables(listed, q.table_host.as<uint32_t>());
  return surface_run(
      q, st->ctx->stream, store_surface_blocks(c.n_chunks), marker, n_out, n_words > q.mask.cap, [&] { return q.mask.grow(n_words, sizeof(uint64_t)); },
      [&] { return store_enqueued(st, launch_store_surface_count(st, q, c)); },
      [&](size_t cap) { return store_enqueued(st, launch_store_surface_emit(st, q, c, marker, cap)); });
}

const void *ws_store_surface_records_dev(const ws_store *st, size_t *n) { return surface_records_dev(st ? &st->surf : nullptr, n); }

const float *ws_store_surface_marker_dev(const ws_store *st, size_t *n) { return surface_marker_dev(st ? &st->surf : nullptr, n); }

int ws_store_surface_download(ws_store *st, void *records_host, float *marker_host, size_t capacity_points, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_surface_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return surface_download(st->surf, st->ctx->stream, "ws_store_surface_download", "ws_store_surface", records_host, marker_host, capacity_points, n_out);
}

int ws_debug_store_surface_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  if (!st) return invalid("ws_debug_store_surface_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->surf.timer, enable, ms_out, SURF_PAIRS, 3);
}

int ws_store_mesh(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t map_resolution, uint32_t flags, size_t *n_vertices, size_t *n_faces)
{
  if (!st || (flags & ~WS_MESH_ANY_WEIGHT) || ((lo == nullptr) != (hi == nullptr)) || map_resolution <= 0) return invalid("ws_store_mesh: bad argument");
  std::unique_lock<std::mutex> lock;
  StoreMeshCall c;
  WS_TRY(store_query_box(st, "ws_store_mesh", lo, hi, false, lock, c.lo, c.hi));
  ws_store::Mesh &q = st->mesh;
  WS_TRY(q.timer.arm());
  if (c.lo[0] > c.hi[0]) return mesh_publish(q, 0, 0, n_vertices, n_faces); // no box and no chunk
  WS_TRY(mesh_corners_fit(c.lo, c.hi, map_resolution, "ws_store_mesh"));
  if (c.hi[0] == c.lo[0] || c.hi[1] == c.lo[1] || c.hi[2] == c.lo[2]) return mesh_publish(q, 0, 0, n_vertices, n_faces); // one voxel thick along an axis: no cells
  std::vector<StoreRaySlot> listed;
  store_list(st, c.lo, c.hi, listed);
  if (listed.empty()) return mesh_publish(q, 0, 0, n_vertices, n_faces); // the box meets no present chunk
  if (listed.size() >= (1u << 19)) return range_error("ws_store_mesh", ": the box overlaps 2^19 present chunks or more (4096 words each must stay below 2^31)");
  WS_TRY(store_mesh_tables(st, listed));
  c.n_chunks = (uint32_t)listed.size();
  c.res = map_resolution;
  c.flags = flags;
  return mesh_run(
      q, st->ctx->stream, "ws_store_mesh", (uint64_t)c.n_chunks * 4096u, n_vertices, n_faces, [&] { return store_enqueued(st, launch_store_mesh_count(st, q, c)); },
      [&] { return store_enqueued(st, launch_store_mesh_emit(st, q, c)); });
}

const void *ws_store_mesh_vertices_dev(const ws_store *st, size_t *n) { return mesh_vertices_dev(st ? &st->mesh : nullptr, n); }

const uint32_t *ws_store_mesh_faces_dev(const ws_store *st, size_t *n) { return mesh_faces_dev(st ? &st->mesh : nullptr, n); }

int ws_store_mesh_download(ws_store *st, void *vertices_host, uint32_t *faces_host, size_t cap_vertices, size_t cap_faces, size_t *n_vertices, size_t *n_faces)
{
  if (!st || !n_vertices || !n_faces) return invalid("ws_store_mesh_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return mesh_download(st->mesh, st->ctx->stream, vertices_host, faces_host, cap_vertices, cap_faces, n_vertices, n_faces);
}

int ws_debug_store_mesh_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  if (!st) return invalid("ws_debug_store_mesh_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->mesh.timer, enable, ms_out, MESH_PAIRS, 3);
}

static int store_raycast(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin[3], const int32_t *dirs, bool dirs_on_host, size_t n,
                         int32_t max_range, int32_t res, uint32_t flags, size_t *n_hits)
{
  std::unique_lock<std::mutex> lock;
  StoreRayCall c;
  c.res = res;
  WS_TRY(raycast_check("ws_store_raycast", !st || ((lo == nullptr) != (hi == nullptr)), origin, dirs, n, max_range, res, flags, [&] {
    WS_TRY(store_query_box(st, "ws_store_raycast", lo, hi, true, lock, c.lo, c.hi));
    return res <= 0 ? invalid("ws_store_raycast: map_resolution <= 0") : (int)WS_OK;
  }));
  ws_store::Ray &q = st->ray;
  std::vector<StoreRaySlot> listed;
  store_list(st, lo, hi, listed); // (without a box: every written chunk)
  if (listed.size() >= (1u << 19)) return range_error("ws_store_raycast", ": the call lists 2^19 present chunks or more");
  c.n_chunks = (uint32_t)listed.size();
  // the live box: the bounding box of the listed chunks (keys are floor(int32 / 64): 64 k + 63 fits), cut to the box
  for (int k = 0; k < 3; ++k) c.blo[k] = INT32_MAX, c.bhi[k] = INT32_MIN;
  for (const StoreRaySlot &e : listed)
  {
    const int32_t key[3] = {e.cx, e.cy, e.cz};
    for (int k = 0; k < 3; ++k) c.blo[k] = std::min(c.blo[k], key[k] * STORE_CS), c.bhi[k] = std::max(c.bhi[k], key[k] * STORE_CS + STORE_CS - 1);
  }
  for (int k = 0; k < 3; ++k) c.blo[k] = std::max(c.blo[k], c.lo[k]), c.bhi[k] = std::min(c.bhi[k], c.hi[k]);
  // (no listed chunk: the call still launches and answers no-hit for every ray)
  return raycast_run(
      q, st->ctx->stream, dirs, dirs_on_host, n, flags, n_hits, store_lookup_places(listed.size()) > q.table_host.cap,
      [&] { return store_lookup_fill(q.table_host, q.table_dev, listed); },
      [&](const int32_t *dirs_dev) { return store_enqueued(st, launch_store_raycast(st, q, c, origin, dirs_dev, n, max_range, flags)); });
}

int ws_store_raycast(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin_mm[3], const int32_t *dirs_host, size_t n, int32_t max_range_mm,
                     int32_t map_resolution, uint32_t flags, size_t *n_hits)
{
  return store_raycast(st, lo, hi, origin_mm, dirs_host, true, n, max_range_mm, map_resolution, flags, n_hits);
}

int ws_store_raycast_dev(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin_mm[3], const int32_t *dirs_dev, size_t n, int32_t max_range_mm,
                         int32_t map_resolution, uint32_t flags, size_t *n_hits)
{
  return store_raycast(st, lo, hi, origin_mm, dirs_dev, false, n, max_range_mm, map_resolution, flags, n_hits);
}

const void *ws_store_raycast_records_dev(const ws_store *st, size_t *n) { return raycast_records_dev(st ? &st->ray : nullptr, n); }

const int32_t *ws_store_raycast_gradient_dev(const ws_store *st, size_t *n) { return raycast_gradient_dev(st ? &st->ray : nullptr, n); }

int ws_store_raycast_download(ws_store *st, void *records_host, int32_t *gradient_host, size_t capacity_rays, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_raycast_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return raycast_download(st->ray, st->ctx->stream, "ws_store_raycast_download", "ws_store_raycast", records_host, gradient_host, capacity_rays, n_out);
}

int ws_debug_store_raycast_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  if (!st) return invalid("ws_debug_store_raycast_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->ray.timer, enable, ms_out, RAY_PAIRS, 3);
}

// ---- the point sample of the store: the rules and the host flow of ws_map_sample over the chunks, store_sample.hip
static int store_sample(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *points, bool points_on_host, size_t n, int32_t band, int32_t res,
                        uint32_t flags, uint64_t counts[4])
{
  std::unique_lock<std::mutex> lock;
  StoreRayCall c;
  c.res = res;
  WS_TRY(sample_check("ws_store_sample", !st || ((lo == nullptr) != (hi == nullptr)) || band <= 0, points, n, res, flags, [&] {
    WS_TRY(store_query_box(st, "ws_store_sample", lo, hi, true, lock, c.lo, c.hi));
    return res <= 0 ? invalid("ws_store_sample: map_resolution <= 0") : (int)WS_OK;
  }));
  ws_store::Sample &q = st->sample;
  std::vector<StoreRaySlot> listed;
  store_list(st, lo, hi, listed); // (without a box: every written chunk)
  if (listed.size() >= (1u << 19)) return range_error("ws_store_sample", ": the call lists 2^19 present chunks or more");
  c.n_chunks = (uint32_t)listed.size();
  // the live box: the bounding box of the listed chunks (keys are floor(int32 / 64): 64 k + 63 fits), cut to the box
  for (int k = 0; k < 3; ++k) c.blo[k] = INT32_MAX, c.bhi[k] = INT32_MIN;
  for (const StoreRaySlot &e : listed)
  {
    const int32_t key[3] = {e.cx, e.cy, e.cz};
    for (int k = 0; k < 3; ++k) c.blo[k] = std::min(c.blo[k], key[k] * STORE_CS), c.bhi[k] = std::max(c.bhi[k], key[k] * STORE_CS + STORE_CS - 1);
  }
  for (int k = 0; k < 3; ++k) c.blo[k] = std::max(c.blo[k], c.lo[k]), c.bhi[k] = std::min(c.bhi[k], c.hi[k]);
  // (no listed chunk: the call still launches and answers UNKNOWN for every point)
  return sample_run(
      q, st->ctx->stream, points, points_on_host, n, flags, counts, store_lookup_places(listed.size()) > q.table_host.cap,
      [&] { return store_lookup_fill(q.table_host, q.table_dev, listed); },
      [&](const int32_t *pts_dev) { return store_enqueued(st, launch_store_sample(st, q, c, pts_dev, n, band, flags)); });
}

int ws_store_sample(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *points_host, size_t n, int32_t band_mm, int32_t map_resolution,
                    uint32_t flags, uint64_t counts[4])
{
  return store_sample(st, lo, hi, points_host, true, n, band_mm, map_resolution, flags, counts);
}

int ws_store_sample_dev(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *points_dev, size_t n, int32_t band_mm, int32_t map_resolution,
                        uint32_t flags, uint64_t counts[4])
{
  return store_sample(st, lo, hi, points_dev, false, n, band_mm, map_resolution, flags, counts);
}

const void *ws_store_sample_records_dev(const ws_store *st, size_t *n) { return sample_records_dev(st ? &st->sample : nullptr, n); }

const int32_t *ws_store_sample_gradient_dev(const ws_store *st, size_t *n) { return sample_gradient_dev(st ? &st->sample : nullptr, n); }

const int32_t *ws_store_sample_selected_dev(const ws_store *st, size_t *n) { return sample_selected_dev(st ? &st->sample : nullptr, n); }

int ws_store_sample_download(ws_store *st, void *records_host, int32_t *gradient_host, int32_t *selected_host, size_t capacity_points, size_t capacity_selected,
                             size_t *n_out, size_t *n_selected)
{
  if (!st || !n_out) return invalid("ws_store_sample_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return sample_download(st->sample, st->ctx->stream, "ws_store_sample_download", "ws_store_sample", records_host, gradient_host, selected_host, capacity_points,
                         capacity_selected, n_out, n_selected);
}

int ws_debug_store_sample_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  if (!st) return invalid("ws_debug_store_sample_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->sample.timer, enable, ms_out, SAMPLE_PAIRS, 3);
}

// ---- the distance field of the store: the rules and the host flow of ws_map_distance over the chunks, store_distance.hip
int ws_store_distance(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t max_dist_vox, uint32_t flags, size_t *n_sites)
{
  std::unique_lock<std::mutex> lock;
  StoreDistCall c;
  uint32_t ext[3];
  size_t n = 0;
  WS_TRY(distance_check(
      "ws_store_distance", !st, lo, hi, max_dist_vox, flags,
      [&](uint64_t e[3]) {
        WS_TRY(store_query_box(st, "ws_store_distance", lo, hi, false, lock, c.lo, c.hi));
        WS_TRY(st->dist.timer.arm());
        if (c.lo[0] > c.hi[0]) return (int)WS_OK; // no box and no chunk: zero records
        for (int k = 0; k < 3; ++k) e[k] = (uint64_t)((int64_t)c.hi[k] - (int64_t)c.lo[k]) + 1u;
        return (int)WS_OK;
      },
      ext, &n));
  ws_store::Dist &q = st->dist;
  hipStream_t s = st->ctx->stream;
  // the present chunks the box overlaps, and the z range they cover inside it
  std::vector<StoreRaySlot> listed;
  if (n) store_list(st, c.lo, c.hi, listed);
  if (listed.size() >= (1u << 19)) return range_error("ws_store_distance", ": the box overlaps 2^19 present chunks or more");
  c.n_chunks = (uint32_t)listed.size();
  c.nx = ext[0], c.ny = ext[1];
  c.zlo = 1, c.zhi = 0;
  if (c.n_chunks)
  {
    c.zlo = INT32_MAX, c.zhi = INT32_MIN;
    for (const StoreRaySlot &e : listed) c.zlo = std::min(c.zlo, e.cz * STORE_CS), c.zhi = std::max(c.zhi, e.cz * STORE_CS + STORE_CS - 1);
    c.zlo = std::max(c.zlo, c.lo[2]), c.zhi = std::min(c.zhi, c.hi[2]);
  }
  return store_enqueued(st, distance_run(q, s, c.lo, ext, max_dist_vox, flags, n, n_sites, [&] {
    if (store_lookup_places(listed.size()) > q.table_host.cap) WS_HIP(hipStreamSynchronize(s));
    WS_TRY(store_lookup_fill(q.table_host, q.table_dev, listed));
    return launch_store_dist_classify(st, q, c, max_dist_vox, flags);
  }));
}

const uint32_t *ws_store_distance_dev(const ws_store *st, size_t *n) { return distance_dev(st ? &st->dist : nullptr, n); }

int ws_store_distance_download(ws_store *st, uint32_t *host, size_t capacity, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_distance_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return distance_download(st->dist, st->ctx->stream, host, capacity, n_out);
}

int ws_debug_store_distance_timing(ws_store *st, int32_t enable, float ms_out[4])
{
  if (!st) return invalid("ws_debug_store_distance_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->dist.timer, enable, ms_out, DIST_PAIRS, 4);
}

// ---- the ground of the store: the rules and the host flow of ws_map_ground over the chunks, store_ground.hip
int ws_store_ground(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t clear_vox, uint32_t flags, uint64_t counts[4])
{
  std::unique_lock<std::mutex> lock;
  StoreDistCall c;
  uint32_t ext[3];
  size_t n = 0;
  WS_TRY(ground_check(
      "ws_store_ground", !st, lo, hi, clear_vox, flags,
      [&](uint64_t e[3]) {
        WS_TRY(store_query_box(st, "ws_store_ground", lo, hi, false, lock, c.lo, c.hi));
        WS_TRY(st->ground.timer.arm());
        if (c.lo[0] > c.hi[0]) return (int)WS_OK; // no box and no chunk: zero records
        for (int k = 0; k < 3; ++k) e[k] = (uint64_t)((int64_t)c.hi[k] - (int64_t)c.lo[k]) + 1u;
        return (int)WS_OK;
      },
      ext, &n));
  ws_store::Ground &q = st->ground;
  hipStream_t s = st->ctx->stream;
  // the present chunks the box overlaps, and the z range they cover inside it
  std::vector<StoreRaySlot> listed;
  if (n) store_list(st, c.lo, c.hi, listed);
  if (listed.size() >= (1u << 19)) return range_error("ws_store_ground", ": the box overlaps 2^19 present chunks or more");
  c.n_chunks = (uint32_t)listed.size();
  c.nx = ext[0], c.ny = ext[1];
  c.zlo = 1, c.zhi = 0;
  if (c.n_chunks)
  {
    c.zlo = INT32_MAX, c.zhi = INT32_MIN;
    for (const StoreRaySlot &e : listed) c.zlo = std::min(c.zlo, e.cz * STORE_CS), c.zhi = std::max(c.zhi, e.cz * STORE_CS + STORE_CS - 1);
    c.zlo = std::max(c.zlo, c.lo[2]), c.zhi = std::min(c.zhi, c.hi[2]);
  }
  return store_enqueued(st, ground_run(q, s, c.lo, ext, n, counts, [&] {
    if (store_lookup_places(listed.size()) > q.table_host.cap) WS_HIP(hipStreamSynchronize(s));
    WS_TRY(store_lookup_fill(q.table_host, q.table_dev, listed));
    return launch_store_ground_levels(st, q, c, clear_vox, flags);
  }));
}

const void *ws_store_ground_dev(const ws_store *st, size_t *n) { return ground_dev(st ? &st->ground : nullptr, n); }

int ws_store_ground_download(ws_store *st, void *host, size_t capacity, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_ground_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return ground_download(st->ground, st->ctx->stream, host, capacity, n_out);
}

int ws_store_ground_box(ws_store *st, int32_t lo[3], uint32_t ext[3])
{
  if (!st) return invalid("ws_store_ground_box: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return ground_box(st->ground, "ws_store_ground_box", lo, ext);
}

int ws_debug_store_ground_timing(ws_store *st, int32_t enable, float ms_out[2])
{
  if (!st) return invalid("ws_debug_store_ground_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->ground.timer, enable, ms_out, GROUND_PAIRS, 2);
}

// the bridge to the planner: a column distance call whose pass 0 reads the last ground result of the store
int ws_store_ground_distance(ws_store *st, int32_t max_step_q8, int32_t max_dist_vox, uint32_t flags, size_t *n_sites)
{
  std::unique_lock<std::mutex> lock;
  int32_t l[3] = {0, 0, 0};
  uint32_t ext[3];
  size_t n = 0;
  WS_TRY(ground_distance_check(
      "ws_store_ground_distance", !st, max_step_q8, max_dist_vox, flags,
      [&](uint64_t e[3]) {
        lock = std::unique_lock<std::mutex>(st->mu);
        if (!st->ground.have) return invalid("ws_store_ground_distance: no ground result yet (the call runs on the records of the last ws_store_ground)");
        WS_TRY(st->dist.timer.arm());
        for (int k = 0; k < 3; ++k) e[k] = st->ground.n ? (uint64_t)st->ground.ext[k] : 0u, l[k] = st->ground.lo[k];
        return (int)WS_OK;
      },
      ext, &n));
  ws_store::Dist &q = st->dist;
  hipStream_t s = st->ctx->stream;
  const uint32_t dflags = flags | WS_DISTANCE_COLUMNS;
  return store_enqueued(st, distance_run(q, s, l, ext, max_dist_vox, dflags, n, n_sites,
                                         [&] { return launch_ground_sites(s, st->ground, q, (uint32_t)max_step_q8, max_dist_vox, dflags); }));
}

int ws_debug_store_raycast_table(const int32_t *keys_slots, size_t n, int32_t *table, size_t capacity_places, size_t *n_places)
{
  if ((n && table && !keys_slots) || !n_places || n >= (1u << 19)) return invalid("ws_debug_store_raycast_table: bad argument");
  *n_places = store_ray_table_slots(n);
  if (!table) return WS_OK;
  if (capacity_places < *n_places) return invalid("ws_debug_store_raycast_table: the table does not fit");
  std::vector<StoreRaySlot> in(n), out(*n_places);
  if (n) std::memcpy(in.data(), keys_slots, n * sizeof(StoreRaySlot));
  store_ray_table_fill(in.data(), n, out.data());
  std::memcpy(table, out.data(), out.size() * sizeof(StoreRaySlot));
  return WS_OK;
}

uint32_t ws_debug_store_raycast_find(const int32_t *table, size_t n_places, const int32_t key[3])
{
  if (!table || !key || n_places < 2 || (n_places & (n_places - 1))) return STORE_ABSENT;
  std::vector<StoreRaySlot> t(n_places);
  std::memcpy(t.data(), table, n_places * sizeof(StoreRaySlot));
  return store_ray_find(t.data(), (uint32_t)n_places - 1u, key[0], key[1], key[2]);
}

// ---- the frontier of the store: the rules and the host flow of ws_map_frontier over the chunks, store_frontier.hip
namespace
{
// The tables of a frontier call over the n listed chunks (0 < n < 2^19), into st->frontier.table_host: the word-space tables, and the
// list positions of every chunk's six face neighbours, -x +x -y +y -z +z
int store_frontier_tables(ws_store *st, const std::vector<StoreRaySlot> &listed)
{
  const size_t n = listed.size();
  WS_TRY(store_tables_reserve(st, st->frontier.table_host, st->frontier.table_dev, store_frontier_table_bytes(n), store_frontier_table_bytes(n + n / 8)));
  uint32_t *grp = st->frontier.table_host.as<uint32_t>();
  uint32_t *nb = grp + 8 * n;
  store_word_tables(listed, grp);
  const auto before = [](const StoreRaySlot &e, const StoreKey &k) { return StoreKey{e.cx, e.cy, e.cz} < k; };
  for (size_t i = 0; i < n; ++i)
    for (int d = 0; d < 6; ++d)
    {
      // (keys are floor(int32 / 64): a step of one cannot overflow)
      StoreKey k = {listed[i].cx, listed[i].cy, listed[i].cz};
      k[d >> 1] += (d & 1) ? 1 : -1;
      const auto it = std::lower_bound(listed.begin(), listed.end(), k, before);
      const bool found = it != listed.end() && it->cx == k[0] && it->cy == k[1] && it->cz == k[2];
      nb[6 * i + d] = found ? (uint32_t)(it - listed.begin()) : 0xffffffffu;
    }
  return WS_OK;
}
} // namespace

int ws_store_frontier(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t min_value, uint32_t flags, size_t *n_out, size_t *n_clusters)
{
  WS_TRY(frontier_check("ws_store_frontier", !st, lo, hi, min_value, flags));
  std::unique_lock<std::mutex> lock;
  StoreFrontierCall c;
  WS_TRY(store_query_box(st, "ws_store_frontier", lo, hi, false, lock, c.lo, c.hi));
  ws_store::Frontier &q = st->frontier;
  std::vector<StoreRaySlot> listed;
  if (c.lo[0] <= c.hi[0]) store_list(st, c.lo, c.hi, listed); // (else: no box and no chunk)
  if (listed.size() >= (1u << 19)) return range_error("ws_store_frontier", ": the box overlaps 2^19 present chunks or more (4096 words each must stay below 2^31)");
  WS_TRY(q.timer.arm());
  if (listed.empty()) // an empty store, or the box meets no present chunk: nothing in it is free
    return frontier_publish(q, 0, 0, (flags & WS_FRONTIER_CLUSTERS) != 0, n_out, n_clusters);
  c.n_chunks = (uint32_t)listed.size();
  c.min_value = min_value, c.flags = flags;
  const size_t n_words = (size_t)c.n_chunks * 4096u;
  WS_TRY(store_frontier_tables(st, listed));
  return frontier_run(
      q, st->ctx->stream, "ws_store_frontier", store_surface_blocks(c.n_chunks), flags, n_out, n_clusters, n_words > q.mask.cap,
      [&] { return q.mask.grow(n_words, sizeof(uint64_t)); }, [&] { return store_enqueued(st, launch_store_frontier_count(st, q, c)); },
      [&](size_t cap) { return store_enqueued(st, launch_store_frontier_emit(st, q, c, cap)); });
}

const void *ws_store_frontier_records_dev(const ws_store *st, size_t *n) { return surface_records_dev(st ? &st->frontier : nullptr, n); }

const uint32_t *ws_store_frontier_labels_dev(const ws_store *st, size_t *n) { return frontier_labels_dev(st ? &st->frontier : nullptr, n); }

const void *ws_store_frontier_clusters_dev(const ws_store *st, size_t *n) { return frontier_clusters_dev(st ? &st->frontier : nullptr, n); }

int ws_store_frontier_download(ws_store *st, void *records_host, uint32_t *labels_host, void *clusters_host, size_t cap_records, size_t cap_clusters, size_t *n_out,
                               size_t *n_clusters)
{
  if (!st || !n_out) return invalid("ws_store_frontier_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return frontier_download(st->frontier, st->ctx->stream, "ws_store_frontier_download", "ws_store_frontier", records_host, labels_host, clusters_host, cap_records,
                           cap_clusters, n_out, n_clusters);
}

int ws_debug_store_frontier_timing(ws_store *st, int32_t enable, float ms_out[4])
{
  if (!st) return invalid("ws_debug_store_frontier_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->frontier.timer, enable, ms_out, FRONTIER_PAIRS, 4);
}

// ---- the reach of the store: ws_map_reach over the last ws_store_distance result (map_reach.hip reads its records alone)
int ws_store_reach(ws_store *st, const int32_t *seeds_host, size_t n_seeds, int32_t clear_d2, uint32_t flags, uint32_t max_rounds, size_t *n_seeded, size_t *n_reached,
                   uint32_t *rounds)
{
  if (!st) return invalid("ws_store_reach: bad argument");
  std::unique_lock<std::mutex> lock;
  return reach_run(st->reach, st->dist, st->ctx->stream, "ws_store_reach", seeds_host, n_seeds, clear_d2, flags, max_rounds, n_seeded, n_reached, rounds, [&] {
    servers_leave(st->ctx);
    lock = std::unique_lock<std::mutex>(st->mu);
    return (int)WS_OK;
  });
}

const uint32_t *ws_store_reach_dev(const ws_store *st, size_t *n) { return reach_dev(st ? &st->reach : nullptr, n); }

int ws_store_reach_download(ws_store *st, uint32_t *host, size_t capacity, size_t *n_out)
{
  if (!st || !n_out) return invalid("ws_store_reach_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_download(st->reach, st->ctx->stream, host, capacity, n_out);
}

int ws_store_reach_box(ws_store *st, int32_t lo[3], uint32_t ext[3], int32_t *columns)
{
  if (!st) return invalid("ws_store_reach_box: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_box(st->reach, lo, ext, columns);
}

int ws_store_reach_lookup(ws_store *st, const int32_t *points_host, size_t n, int32_t stride, uint32_t *cost_host)
{
  if (!st) return invalid("ws_store_reach_lookup: bad argument");
  servers_leave(st->ctx);
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_lookup(st->reach, st->ctx->stream, "ws_store_reach_lookup", points_host, true, n, stride, cost_host);
}

int ws_store_reach_lookup_dev(ws_store *st, const int32_t *points_dev, size_t n, int32_t stride, uint32_t *cost_dev)
{
  if (!st) return invalid("ws_store_reach_lookup_dev: bad argument");
  servers_leave(st->ctx);
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_lookup(st->reach, st->ctx->stream, "ws_store_reach_lookup_dev", points_dev, false, n, stride, cost_dev);
}

int ws_store_reach_paths(ws_store *st, const int32_t *goals_host, size_t g, uint32_t cap_steps, void *headers_host, void *records_host)
{
  if (!st) return invalid("ws_store_reach_paths: bad argument");
  servers_leave(st->ctx);
  std::lock_guard<std::mutex> lock(st->mu);
  return reach_paths(st->reach, st->ctx->stream, "ws_store_reach_paths", goals_host, g, cap_steps, headers_host, records_host);
}

int ws_debug_store_reach_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  if (!st) return invalid("ws_debug_store_reach_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->reach.timer, enable, ms_out, REACH_PAIRS, 3);
}

// ---- the view gain of the store: the rules and the host flow of ws_map_view_gain over the chunks, store_gain.hip
int ws_store_view_gain(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *origins_host, size_t n_views, const int32_t *dirs_host, size_t n,
                       int32_t max_range_mm, int32_t map_resolution, int32_t min_value, uint32_t flags, uint64_t *best_unknown_k2)
{
  std::unique_lock<std::mutex> lock;
  GainCall c;
  WS_TRY(gain_check("ws_store_view_gain", !st, lo, hi, origins_host, n_views, dirs_host, n, max_range_mm, min_value, map_resolution, flags, best_unknown_k2, [&] {
    if (map_resolution <= 0) return invalid("ws_store_view_gain: map_resolution <= 0");
    for (int k = 0; k < 3 && lo; ++k)
      if (hi[k] < lo[k]) return invalid("ws_store_view_gain: hi < lo");
    return (int)WS_OK;
  }));
  servers_leave(st->ctx);
  WS_TRY(store_query_box(st, "ws_store_view_gain", lo, hi, false, lock, c.lo, c.hi)); // (without a box: the bounding box of the chunks; none: empty)
  if (n_views == 0 || n == 0) return WS_OK; // nothing written, the last result stays
  ws_store::Gain &q = st->gain;
  std::vector<StoreRaySlot> listed;
  if (c.lo[0] <= c.hi[0]) store_list(st, c.lo, c.hi, listed);
  if (listed.size() >= (1u << 19)) return range_error("ws_store_view_gain", ": the box overlaps 2^19 present chunks or more");
  c.m = n_views, c.n = n;
  c.res = map_resolution, c.max_range = max_range_mm, c.min_value = min_value, c.flags = flags;
  return gain_run(
      q, st->ctx->stream, c, origins_host, dirs_host, best_unknown_k2, store_lookup_places(listed.size()) > q.table_host.cap,
      [&] { return store_lookup_fill(q.table_host, q.table_dev, listed); }, [&] { return store_enqueued(st, launch_store_gain(st, q, c, (uint32_t)listed.size())); });
}

const void *ws_store_view_gain_records_dev(const ws_store *st, size_t *n) { return gain_records_dev(st ? &st->gain : nullptr, n); }

const void *ws_store_view_gain_rays_dev(const ws_store *st, size_t *n) { return gain_rays_dev(st ? &st->gain : nullptr, n); }

int ws_store_view_gain_download(ws_store *st, void *records_host, void *rays_host, size_t cap_views, size_t cap_rays, size_t *n_views, size_t *n_rays)
{
  if (!st || !n_views) return invalid("ws_store_view_gain_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  return gain_download(st->gain, st->ctx->stream, "ws_store_view_gain_download", "ws_store_view_gain", records_host, rays_host, cap_views, cap_rays, n_views, n_rays);
}

int ws_debug_store_view_gain_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  if (!st) return invalid("ws_debug_store_view_gain_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->gain.timer, enable, ms_out, GAIN_PAIRS, 3);
}

// ---- one store fused into another under a rigid pose: the plan, the count pass, the host step and the write pass of ws_store_fuse
// (the rules are stated in warpsense_hip.h and live in ws_fuse.h; the kernels in store_fuse.hip)
namespace
{
constexpr int FUSE_PAIRS[3][2] = {{0, 1}, {1, 2}, {2, 3}};

inline int64_t floor_div64(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); } // b > 0

// The candidate chunks of DST: every src chunk, grown by two voxels, mapped forward with the transpose of rot in double precision;
// the chunks its bounding box (2 mm more per side) overlaps, clipped to the reach around pivot_dst and to int32 voxels.  A superset of
// what can receive anything: the rounding of q is below 1 mm.
void fuse_candidates(const ws_store *src, const ws_fuse_pose &pull, int32_t res, std::set<StoreKey> &cand)
{
  const int64_t h = res / 2;
  int64_t vlo[3], vhi[3]; // the dst voxels inside the reach and inside int32
  for (int k = 0; k < 3; ++k)
  {
    vlo[k] = std::max<int64_t>(-floor_div64(-((int64_t)pull.pivot_dst_mm[k] - (FUSE_REACH - 1) - h), res), INT32_MIN); // ceil
    vhi[k] = std::min<int64_t>(floor_div64((int64_t)pull.pivot_dst_mm[k] + (FUSE_REACH - 1) - h, res), INT32_MAX);
  }
  double R[9];
  for (int i = 0; i < 9; ++i) R[i] = (double)pull.rot_q30[i] / 1073741824.0;
  for (const auto &kv : src->dir)
  {
    if (!kv.second.written) continue;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int c = 0; c < 8; ++c)
    {
      double q[3];
      for (int k = 0; k < 3; ++k)
        q[k] = ((double)kv.first[k] * STORE_CS + (((c >> k) & 1) ? STORE_CS + 2 : -2)) * (double)res - (double)pull.pivot_src_mm[k];
      for (int k = 0; k < 3; ++k) // p = rot^T q + pivot_dst
      {
        const double p = R[k] * q[0] + R[3 + k] * q[1] + R[6 + k] * q[2] + (double)pull.pivot_dst_mm[k];
        lo[k] = std::min(lo[k], p), hi[k] = std::max(hi[k], p);
      }
    }
    int64_t c0[3], c1[3];
    bool any = true;
    for (int k = 0; k < 3; ++k)
    {
      // the voxels whose centre v res + h lies in [lo - 2, hi + 2]; far outside the reach the doubles are cut before the conversion
      const double a = std::max(lo[k] - 2.0, -4e12), b = std::min(hi[k] + 2.0, 4e12);
      const int64_t v0 = std::max(floor_div64((int64_t)std::floor(a) - h, res), vlo[k]), v1 = std::min(floor_div64((int64_t)std::ceil(b) - h, res) + 1, vhi[k]);
      any = any && v0 <= v1;
      c0[k] = floor_div64(v0, STORE_CS), c1[k] = floor_div64(v1, STORE_CS);
    }
    if (!any) continue;
    for (int64_t x = c0[0]; x <= c1[0]; ++x)
      for (int64_t y = c0[1]; y <= c1[1]; ++y)
        for (int64_t z = c0[2]; z <= c1[2]; ++z) cand.insert(StoreKey{(int32_t)x, (int32_t)y, (int32_t)z});
  }
}

// the words of the count pass: room for n candidates, cleared in stream order
int fuse_words(ws_store *dst, size_t n)
{
  ws_store::Fuse &q = dst->fuse;
  const size_t words = 2 * FUSE_STATS_DEV + n;
  if (words > q.words.cap || words > q.words_host.cap)
  {
    WS_HIP(hipStreamSynchronize(dst->ctx->stream));
    WS_TRY(q.words.alloc(words + words / 8, sizeof(uint32_t)));
    WS_TRY(q.words_host.alloc(words + words / 8, sizeof(uint32_t), HostBlock::PINNED));
  }
  WS_HIP(hipMemsetAsync(q.words.p, 0, words * sizeof(uint32_t), dst->ctx->stream));
  return WS_OK;
}

// everything of the call that enqueues; the caller synchronises after a failure
int fuse_run(ws_store *dst, ws_store *src, const ws_fuse_pose &pull, int32_t res, int32_t max_weight, bool count_only, uint64_t stats[6])
{
  hipStream_t s = dst->ctx->stream;
  ws_store::Fuse &q = dst->fuse;
  std::set<StoreKey> cand;
  fuse_candidates(src, pull, res, cand);
  if (cand.size() >= FUSE_MAX_CANDIDATES) return range_error("ws_store_fuse", ": 2^23 candidate chunks of DST or more");
  stats[0] = cand.size();
  if (cand.empty()) return WS_OK;

  // the plan: the lookup of SRC's chunks in a table of SRC's ring, the candidates in one of DST's
  size_t places = 0;
  const size_t n = cand.size();
  ws_store::Table *ts = nullptr, *td = nullptr;
  WS_TRY(store_lookup_plan(src, "ws_store_fuse", ": SRC holds 2^19 chunks or more", &ts, &places));
  WS_TRY(store_table(dst, n * 4, &td));
  FuseCand *ch = td->host.as<FuseCand>();
  size_t i = 0;
  for (const StoreKey &k : cand)
  {
    const auto it = dst->dir.find(k);
    ch[i++] = FuseCand{k[0], k[1], k[2], it == dst->dir.end() ? STORE_ABSENT : it->second.slot};
  }
  WS_TRY(fuse_words(dst, n));
  q.timer.mark(0, s);
  WS_HIP(hipMemcpyAsync(ts->dev.p, ts->host.p, places * sizeof(StoreRaySlot), hipMemcpyHostToDevice, s));
  WS_HIP(hipMemcpyAsync(td->dev.p, td->host.p, n * sizeof(FuseCand), hipMemcpyHostToDevice, s));
  q.timer.mark(1, s);

  FuseArgs a;
  for (int k = 0; k < 9; ++k) a.rot[k] = pull.rot_q30[k];
  for (int k = 0; k < 3; ++k) a.pd[k] = pull.pivot_dst_mm[k], a.ps[k] = pull.pivot_src_mm[k];
  a.res = res, a.half = res / 2, a.max_weight = max_weight, a.fill = dst->fill;
  a.rdiv = make_fastdiv(res);
  a.res3 = (int64_t)res * res * res;
  a.tdiv = make_fuse_div(a.res3);
  a.cand = td->dev.as<FuseCand>();
  a.src_table = ts->dev.as<StoreRaySlot>();
  a.src_mask = (uint32_t)places - 1u;
  a.src_segs = src->seg_tab.as<uint32_t *>(), a.src_shift = src->seg_shift;
  a.dst_segs = dst->seg_tab.as<uint32_t *>(), a.dst_shift = dst->seg_shift;
  a.stats = q.words.as<unsigned long long>();
  a.counts = q.words.as<uint32_t>() + 2 * FUSE_STATS_DEV;
  WS_TRY(launch_store_fuse(s, a, n, false));
  q.timer.mark(2, s);
  WS_HIP(hipEventRecord(td->done, s));
  td->used = true;
  WS_HIP(hipMemcpyAsync(q.words_host.p, q.words.p, (2 * FUSE_STATS_DEV + n) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s)); // the one host read of the call: which chunks receive anything decides what is created

  const unsigned long long *sums = q.words_host.as<unsigned long long>();
  const uint32_t *counts = q.words_host.as<uint32_t>() + 2 * FUSE_STATS_DEV;
  for (int k = 0; k < 4; ++k) stats[2 + k] = sums[k];
  std::vector<FuseCand> work; // the candidates with a non-zero count (ch stays readable: its table is not handed out again before the call ends)
  std::set<StoreKey> fresh;
  for (i = 0; i < n; ++i)
  {
    if (!counts[i]) continue;
    work.push_back(ch[i]);
    if (ch[i].slot == STORE_ABSENT) fresh.insert(StoreKey{ch[i].cx, ch[i].cy, ch[i].cz});
  }
  stats[1] = fresh.size();
  if (count_only || work.empty())
  {
    q.timer.mark(3, s);
    WS_HIP(hipEventRecord(ts->done, s));
    ts->used = true;
    return WS_OK;
  }

  {
    const int rc_room = store_make_room(dst, fresh.size(), "ws_store_fuse");
    if (rc_room != WS_OK) // refused before any write; the table of SRC has been read by the count pass
    {
      (void)hipEventRecord(ts->done, s);
      ts->used = true;
      return rc_room;
    }
  }
  for (const StoreKey &k : fresh) dst->dir[k] = ws_store::Entry{store_take_slot(dst), true};
  int rc = WS_OK;
  ws_store::Table *tw = nullptr;
  for (FuseCand &c : work)
    if (c.slot == STORE_ABSENT && rc == WS_OK)
    {
      c.slot = dst->dir[StoreKey{c.cx, c.cy, c.cz}].slot;
      rc = fill_u32(dst->ctx, store_slot_ptr(dst, c.slot), dst->fill, STORE_CHUNK_WORDS);
    }
  if (rc == WS_OK) rc = store_table(dst, work.size() * 4, &tw);
  if (rc == WS_OK)
  {
    std::memcpy(tw->host.p, work.data(), work.size() * sizeof(FuseCand));
    const hipError_t e = hipMemcpyAsync(tw->dev.p, tw->host.p, work.size() * sizeof(FuseCand), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (write table)", __FILE__, __LINE__);
  }
  if (rc == WS_OK)
  {
    a.cand = tw->dev.as<FuseCand>();
    a.dst_segs = dst->seg_tab.as<uint32_t *>(); // (a new segment replaces the table)
    rc = launch_store_fuse(s, a, work.size(), true);
  }
  if (rc != WS_OK) // nothing of DST's existing chunks has been written: the write pass was not enqueued
  {
    (void)hipStreamSynchronize(s);
    store_evict(dst, fresh);
    return rc;
  }
  q.timer.mark(3, s);
  WS_HIP(hipEventRecord(ts->done, s));
  WS_HIP(hipEventRecord(tw->done, s));
  ts->used = tw->used = true;
  return WS_OK;
}
} // namespace

int ws_store_fuse(ws_store *dst, ws_store *src, const ws_fuse_pose *pull, int32_t map_resolution, int32_t max_weight, uint32_t flags, uint64_t stats[6])
{
  if (!dst || !src || !pull || !stats) return invalid("ws_store_fuse: NULL argument");
  if (flags & ~WS_FUSE_COUNT_ONLY) return invalid("ws_store_fuse: unknown flag bits");
  if (dst == src) return invalid("ws_store_fuse: dst and src are the same store");
  if (dst->ctx != src->ctx) return invalid("ws_store_fuse: the stores belong to different contexts");
  if (max_weight < 1 || max_weight > 32767) return invalid("ws_store_fuse: max_weight must be 1 .. 32767");
  if ((int16_t)(dst->fill >> 16) > 0) return invalid("ws_store_fuse: the fill_entry of dst has a weight > 0");
  for (int k = 0; k < 9; ++k)
    if (pull->rot_q30[k] < -(1 << 30) || pull->rot_q30[k] > (1 << 30)) return invalid("ws_store_fuse: a rot_q30 entry beyond +-2^30");
  if (map_resolution < 1 || map_resolution > 1024) return range_error("ws_store_fuse", ": the resolution must be 1 .. 1024 mm");
  servers_leave(dst->ctx);
  // both locks, in address order
  ws_store *first = std::less<ws_store *>()(dst, src) ? dst : src, *second = first == dst ? src : dst;
  std::lock_guard<std::mutex> lock_a(first->mu), lock_b(second->mu);
  WS_TRY(dst->fuse.timer.arm());
  uint64_t out[6] = {0, 0, 0, 0, 0, 0};
  const int rc = store_enqueued(dst, fuse_run(dst, src, *pull, map_resolution, max_weight, (flags & WS_FUSE_COUNT_ONLY) != 0, out));
  if (rc != WS_OK) return rc;
  WS_HIP(hipStreamSynchronize(dst->ctx->stream));
  for (int k = 0; k < 6; ++k) stats[k] = out[k];
  return WS_OK;
}

int ws_debug_store_fuse_timing(ws_store *dst, int32_t enable, float ms_out[3])
{
  if (!dst) return invalid("ws_debug_store_fuse_timing: store is NULL");
  std::lock_guard<std::mutex> lock(dst->mu);
  return query_timing(dst->ctx->stream, dst->fuse.timer, enable, ms_out, FUSE_PAIRS, 3);
}

// ---- a store at half the resolution of another: the plan and the one pass of ws_store_coarsen (the rule is stated in
// warpsense_hip.h and lives in ws_coarsen.h; the kernel in store_coarsen.hip)
namespace
{
constexpr int COARSEN_PAIRS[2][2] = {{0, 1}, {1, 2}};

inline StoreKey parent_of(const StoreKey &k) { return {k[0] >> 1, k[1] >> 1, k[2] >> 1}; } // (arithmetic shift: floor(k / 2))

// The slots of the eight children of dst chunk `key` in SRC into w[1 .. 8], index cx * 4 + cy * 2 + cz: STORE_ABSENT where SRC has no
// such chunk, has not written it yet, or the child's key 2 key + {0, 1} does not lie in int32.  Returns whether any child exists.
bool coarsen_children(const ws_store *src, const StoreKey &key, uint32_t *w)
{
  bool any = false;
  for (int c = 0; c < 8; ++c)
  {
    const int64_t ck[3] = {2 * (int64_t)key[0] + (c >> 2), 2 * (int64_t)key[1] + ((c >> 1) & 1), 2 * (int64_t)key[2] + (c & 1)};
    w[1 + c] = STORE_ABSENT;
    if (ck[0] < INT32_MIN || ck[0] > INT32_MAX || ck[1] < INT32_MIN || ck[1] > INT32_MAX || ck[2] < INT32_MIN || ck[2] > INT32_MAX) continue;
    const auto it = src->dir.find(StoreKey{(int32_t)ck[0], (int32_t)ck[1], (int32_t)ck[2]});
    if (it == src->dir.end() || !it->second.written) continue;
    w[1 + c] = it->second.slot;
    any = true;
  }
  return any;
}

// everything of the call behind its refusals; both locks are held
int coarsen_run(ws_store *dst, ws_store *src, const std::set<StoreKey> &listed, int32_t min_observed, uint64_t *stats)
{
  hipStream_t s = dst->ctx->stream;
  ws_store::Coarsen &q = dst->coarsen;
  // the plan is a directory decision: one row per listed chunk that exists afterwards, the chunks to create counted before any launch
  std::vector<uint32_t> rows;
  std::vector<StoreKey> row_key;
  std::set<StoreKey> fresh;
  for (const StoreKey &k : listed)
  {
    uint32_t w[COARSEN_ROW] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bool any = coarsen_children(src, k, w);
    const auto it = dst->dir.find(k);
    if (it == dst->dir.end() && !any) continue; // no child and no chunk: not created
    if (it == dst->dir.end()) fresh.insert(k);
    else w[0] = it->second.slot;
    rows.insert(rows.end(), w, w + COARSEN_ROW);
    row_key.push_back(k);
  }
  const size_t n = row_key.size();
  if (n >= COARSEN_MAX_CHUNKS) return range_error("ws_store_coarsen", ": 2^23 chunks of DST or more");
  if (stats) stats[0] = n, stats[1] = fresh.size(), stats[2] = stats[3] = 0;
  if (n == 0) return WS_OK;
  WS_TRY(store_make_room(dst, fresh.size(), "ws_store_coarsen"));
  if (stats && (!q.words.cap || !q.words_host.cap))
  {
    WS_TRY(q.words.alloc(2, sizeof(unsigned long long)));
    WS_TRY(q.words_host.alloc(2, sizeof(unsigned long long), HostBlock::PINNED));
  }
  for (const StoreKey &k : fresh) dst->dir[k] = ws_store::Entry{store_take_slot(dst), true}; // (the pass writes every word of them)
  for (size_t i = 0; i < n; ++i)
    if (fresh.count(row_key[i])) rows[i * COARSEN_ROW] = dst->dir[row_key[i]].slot;

  const auto enqueue = [&]() -> int {
    ws_store::Table *t = nullptr;
    WS_TRY(store_table(dst, rows.size(), &t));
    std::memcpy(t->host.p, rows.data(), rows.size() * sizeof(uint32_t));
    if (stats) WS_HIP(hipMemsetAsync(q.words.p, 0, 2 * sizeof(unsigned long long), s));
    q.timer.mark(0, s);
    WS_HIP(hipMemcpyAsync(t->dev.p, t->host.p, rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    q.timer.mark(1, s);
    CoarsenArgs a;
    a.rows = t->dev.as<uint32_t>();
    a.src_segs = src->seg_tab.as<uint32_t *>(), a.src_shift = src->seg_shift;
    a.dst_segs = dst->seg_tab.as<uint32_t *>(), a.dst_shift = dst->seg_shift; // (after store_make_room: a new segment replaces the table)
    a.fill = dst->fill, a.min_observed = min_observed;
    a.stats = stats ? q.words.as<unsigned long long>() : nullptr;
    WS_TRY(launch_store_coarsen(s, a, n));
    q.timer.mark(2, s);
    WS_HIP(hipEventRecord(t->done, s));
    t->used = true;
    if (stats) WS_HIP(hipMemcpyAsync(q.words_host.p, q.words.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    return WS_OK;
  };
  const int rc = enqueue();
  if (rc != WS_OK) // the created chunks leave the directory again; launches already enqueued still run
  {
    (void)hipStreamSynchronize(s);
    store_evict(dst, fresh);
    return rc;
  }
  if (!stats) return WS_OK;
  WS_HIP(hipStreamSynchronize(s));
  stats[2] = q.words_host.as<unsigned long long>()[0], stats[3] = q.words_host.as<unsigned long long>()[1];
  return WS_OK;
}
} // namespace

int ws_store_parents_of(const int32_t *keys, size_t n, int32_t *parents, size_t capacity, size_t *n_out)
{
  if ((!keys && n) || (!parents && capacity)) return invalid("ws_store_parents_of: bad argument");
  std::set<StoreKey> up;
  for (size_t i = 0; i < n; ++i) up.insert(parent_of(StoreKey{keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]}));
  size_t i = 0;
  for (const StoreKey &k : up)
  {
    if (i >= capacity) break;
    for (int a = 0; a < 3; ++a) parents[3 * i + a] = k[a];
    ++i;
  }
  if (n_out) *n_out = up.size();
  return WS_OK;
}

int ws_store_coarsen(ws_store *dst, ws_store *src, const int32_t *dst_keys, size_t n_keys, int32_t min_observed, uint32_t flags, uint64_t stats[4])
{
  if (!dst || !src) return invalid("ws_store_coarsen: NULL argument");
  if (flags != WS_COARSEN_DEFAULT) return invalid("ws_store_coarsen: unknown flag bits");
  if (dst == src) return invalid("ws_store_coarsen: dst and src are the same store");
  if (dst->ctx != src->ctx) return invalid("ws_store_coarsen: the stores belong to different contexts");
  if (min_observed < 1 || min_observed > 8) return invalid("ws_store_coarsen: min_observed must be 1 .. 8");
  if (n_keys && !dst_keys) return invalid("ws_store_coarsen: n_keys > 0 with NULL keys");
  if ((int16_t)(dst->fill >> 16) > 0) return invalid("ws_store_coarsen: the fill_entry of dst has a weight > 0");
  servers_leave(dst->ctx);
  // both locks, in address order
  ws_store *first = std::less<ws_store *>()(dst, src) ? dst : src, *second = first == dst ? src : dst;
  std::lock_guard<std::mutex> lock_a(first->mu), lock_b(second->mu);
  WS_TRY(dst->coarsen.timer.arm());
  std::set<StoreKey> listed;
  if (dst_keys)
    for (size_t i = 0; i < n_keys; ++i) listed.insert(StoreKey{dst_keys[3 * i], dst_keys[3 * i + 1], dst_keys[3 * i + 2]});
  else
    for (const auto &kv : src->dir)
      if (kv.second.written) listed.insert(parent_of(kv.first));
  uint64_t out[4] = {0, 0, 0, 0};
  WS_TRY(coarsen_run(dst, src, listed, min_observed, stats ? out : nullptr));
  for (int k = 0; k < 4 && stats; ++k) stats[k] = out[k];
  return WS_OK;
}

int ws_debug_store_coarsen_timing(ws_store *dst, int32_t enable, float ms_out[2])
{
  if (!dst) return invalid("ws_debug_store_coarsen_timing: store is NULL");
  std::lock_guard<std::mutex> lock(dst->mu);
  return query_timing(dst->ctx->stream, dst->coarsen.timer, enable, ms_out, COARSEN_PAIRS, 2);
}

// ---- where two stores differ under a rigid pose: the host flow of ws_store_changes (the rules are stated in warpsense_hip.h and live
// in ws_changes.h; the kernels in store_changes.hip).  The extraction is the flow of the store's frontier, the lookup of REF the plan
// of the fuse.
int ws_store_changes(ws_store *cur, ws_store *ref, const ws_fuse_pose *pull, int32_t map_resolution, const int32_t lo[3], const int32_t hi[3], int32_t band,
                     int32_t free_value, int32_t min_weight, uint32_t flags, size_t *n_out, size_t *n_clusters, uint64_t stats[6])
{
  const uint32_t kinds = WS_CHANGES_APPEARED | WS_CHANGES_VANISHED;
  if (!cur || !ref || !pull || !stats) return invalid("ws_store_changes: NULL argument");
  if (flags & ~(kinds | WS_CHANGES_CLUSTERS)) return invalid("ws_store_changes: unknown flag bits");
  if (!(flags & kinds)) return invalid("ws_store_changes: neither WS_CHANGES_APPEARED nor WS_CHANGES_VANISHED");
  if (cur == ref) return invalid("ws_store_changes: cur and ref are the same store");
  if (cur->ctx != ref->ctx) return invalid("ws_store_changes: the stores belong to different contexts");
  if ((lo == nullptr) != (hi == nullptr)) return invalid("ws_store_changes: exactly one of lo and hi is NULL");
  for (int k = 0; k < 9; ++k)
    if (pull->rot_q30[k] < -(1 << 30) || pull->rot_q30[k] > (1 << 30)) return invalid("ws_store_changes: a rot_q30 entry beyond +-2^30");
  if (map_resolution < 1 || map_resolution > 1024) return range_error("ws_store_changes", ": the resolution must be 1 .. 1024 mm");
  if (band < 1) return range_error("ws_store_changes", ": band must be >= 1");
  if (free_value < band || free_value > 32767) return range_error("ws_store_changes", ": free_value must be band .. 32767");
  if (min_weight < 1 || min_weight > 32767) return range_error("ws_store_changes", ": min_weight must be 1 .. 32767");
  servers_leave(cur->ctx);
  // both locks, in address order (store_query_box takes CUR's behind its own refusal)
  std::unique_lock<std::mutex> lock_cur, lock_ref;
  if (std::less<ws_store *>()(ref, cur)) lock_ref = std::unique_lock<std::mutex>(ref->mu);
  StoreChangesCall c;
  WS_TRY(store_query_box(cur, "ws_store_changes", lo, hi, false, lock_cur, c.lo, c.hi));
  if (!lock_ref.owns_lock()) lock_ref = std::unique_lock<std::mutex>(ref->mu);
  ws_store::Changes &q = cur->changes;
  hipStream_t s = cur->ctx->stream;
  const bool clusters = (flags & WS_CHANGES_CLUSTERS) != 0;
  std::vector<StoreRaySlot> listed;
  if (c.lo[0] <= c.hi[0]) store_list(cur, c.lo, c.hi, listed); // (else: no box and no chunk)
  if (listed.size() >= (1u << 19)) return range_error("ws_store_changes", ": the box overlaps 2^19 present chunks of CUR or more (4096 words each must stay below 2^31)");
  if (listed.empty()) // an empty store, or the box meets no present chunk: nothing is examined, and no plan is made (REF's limit holds all the same)
  {
    size_t n_ref = 0;
    for (const auto &kv : ref->dir) n_ref += kv.second.written ? 1 : 0;
    if (n_ref >= (1u << 19)) return range_error("ws_store_changes", ": REF holds 2^19 chunks or more");
    WS_TRY(q.timer.arm());
    for (int k = 0; k < 6; ++k) stats[k] = 0;
    return frontier_publish(q, 0, 0, clusters, n_out, n_clusters);
  }
  ws_store::Table *ts = nullptr;
  WS_TRY(store_lookup_plan(ref, "ws_store_changes", ": REF holds 2^19 chunks or more", &ts, &c.ref_places));
  WS_TRY(q.timer.arm());
  c.n_chunks = (uint32_t)listed.size();
  c.pull = *pull;
  c.res = map_resolution, c.band = band, c.free_value = free_value, c.min_weight = min_weight;
  c.kinds = flags & kinds;
  c.ref_table_dev = ts->dev.p;
  const size_t n = listed.size(), n_words = n * 4096u;
  WS_TRY(q.stats.alloc(CH_STATS_DEV));
  WS_TRY(store_tables_reserve(cur, q.table_host, q.table_dev, store_word_table_bytes(n), store_word_table_bytes(n + n / 8)));
  store_word_tables(listed, q.table_host.as<uint32_t>());
  const int rc = frontier_run(
      q, s, "ws_store_changes", store_surface_blocks(c.n_chunks), clusters ? WS_FRONTIER_CLUSTERS : WS_FRONTIER_DEFAULT, n_out, n_clusters, n_words > q.mask.cap,
      [&] { return q.mask.grow(n_words, sizeof(uint64_t)); },
      [&] {
        q.timer.mark(0, s);
        const hipError_t e = hipMemcpyAsync(ts->dev.p, ts->host.p, c.ref_places * sizeof(StoreRaySlot), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return store_enqueued(cur, hip_fail(e, "hipMemcpyAsync (lookup of REF)", __FILE__, __LINE__));
        return store_enqueued(cur, launch_store_changes_count(cur, ref, q, c));
      },
      [&](size_t cap) { return store_enqueued(cur, launch_store_changes_emit(cur, ref, q, c, cap)); });
  // (every pass that reads REF's table has been waited for by now, or never ran)
  (void)hipEventRecord(ts->done, s);
  ts->used = true;
  if (rc != WS_OK) return rc;
  stats[0] = c.n_chunks;
  for (uint32_t k = 0; k < CH_STATS_DEV; ++k) stats[1 + k] = q.stats.host[k];
  return WS_OK;
}

const void *ws_store_changes_records_dev(const ws_store *cur, size_t *n) { return surface_records_dev(cur ? &cur->changes : nullptr, n); }

const uint32_t *ws_store_changes_labels_dev(const ws_store *cur, size_t *n) { return frontier_labels_dev(cur ? &cur->changes : nullptr, n); }

const void *ws_store_changes_clusters_dev(const ws_store *cur, size_t *n) { return frontier_clusters_dev(cur ? &cur->changes : nullptr, n); }

int ws_store_changes_download(ws_store *cur, void *records_host, uint32_t *labels_host, void *clusters_host, size_t cap_records, size_t cap_clusters, size_t *n_out,
                              size_t *n_clusters)
{
  if (!cur || !n_out) return invalid("ws_store_changes_download: NULL argument");
  std::lock_guard<std::mutex> lock(cur->mu);
  return frontier_download(cur->changes, cur->ctx->stream, "ws_store_changes_download", "ws_store_changes", records_host, labels_host, clusters_host, cap_records,
                           cap_clusters, n_out, n_clusters);
}

int ws_debug_store_changes_timing(ws_store *cur, int32_t enable, float ms_out[4])
{
  if (!cur) return invalid("ws_debug_store_changes_timing: store is NULL");
  std::lock_guard<std::mutex> lock(cur->mu);
  return query_timing(cur->ctx->stream, cur->changes.timer, enable, ms_out, FRONTIER_PAIRS, 4);
}
