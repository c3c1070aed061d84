// api_store.hip — the chunk store itself, the global map in device memory (kernels in map_store.hip): the directory, the segments and
// the ring of slot tables; ws_store_create to ws_store_drop_chunk; the box transfers between a map's window and the chunks
// (ws_store_save_box, ws_store_load_box) and the map shift that never leaves the device (ws_shift_device); ws_store_chunks_of_box and
// ws_debug_store_timing.  The calls that read one store are in api_store_query.hip, those over two stores in api_store_pair.hip.
#include <new>
#include <set>

#include "ws_api.h"

using namespace ws;

namespace
{
uint64_t store_capacity(const ws_store *st) { return (uint64_t)st->segs.size() << st->seg_shift; }

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

// room for n words in one slot table (pinned + device) and its event
int store_table_reserve(ws_store::Table &t, size_t n)
{
  if (!t.done) WS_HIP(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  if (n <= t.host.cap) return WS_OK;
  WS_TRY(t.host.alloc(n, sizeof(uint32_t), HostBlock::PINNED));
  return t.dev.alloc(n, sizeof(uint32_t));
}

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

int store_args(const ws_store *st, const ws_map *m, int which, const char *name)
{
  if (!st || !m || (which != WS_MAP_AVG && which != WS_MAP_NEW)) return invalid((std::string(name) + ": bad argument").c_str());
  if (st->ctx != m->ctx) return invalid((std::string(name) + ": the store belongs to another context").c_str());
  return WS_OK;
}
} // namespace

// (declared in ws_api.h: api_store_pair.hip and api_pack.hip hand out slots and take tables by the same rules)
namespace ws
{
uint32_t *store_slot_ptr(const ws_store *st, uint32_t slot)
{
  return st->seg_ptr[slot >> st->seg_shift] + (size_t)(slot & ((1u << st->seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
}

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

void store_evict(ws_store *st, const std::set<StoreKey> &fresh)
{
  for (const StoreKey &k : fresh)
  {
    const auto it = st->dir.find(k);
    if (it == st->dir.end()) continue;
    st->free_slots.push_back(it->second.slot);
    st->dir.erase(it);
  }
}

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
