// api_store_pair.hip — the calls over two chunk stores (api_store.hip): the two that write one store from another, ws_store_fuse
// (store_fuse.hip) and ws_store_coarsen with ws_store_parents_of (store_coarsen.hip), and the one that compares one store with another,
// ws_store_changes (store_changes.hip), with their _dev, _download and _timing entry points.  Each holds both stores' locks.  The box,
// the list and the chunk tables of CUR in ws_store_changes are those of a call that reads one store (api_store_query.hip, ws_api.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <set>

#include "ws_api.h"
#include "ws_changes.h"
#include "ws_coarsen.h"
#include "ws_fuse.h"

using namespace ws;

namespace
{
// both stores' locks, taken in address order
struct BothLocks
{
  std::unique_lock<std::mutex> first, second;
  BothLocks(ws_store *a, ws_store *b)
  {
    if (std::less<ws_store *>()(b, a)) std::swap(a, b);
    first = std::unique_lock<std::mutex>(a->mu);
    second = std::unique_lock<std::mutex>(b->mu);
  }
};

// the refusals of a pose and a resolution, in the name of the entry point
int pose_check(const char *name, const ws_fuse_pose *pull, int32_t res)
{
  for (int k = 0; k < 9; ++k)
    if (pull->rot_q30[k] < -(1 << 30) || pull->rot_q30[k] > (1 << 30)) return invalid(std::string(name) + ": a rot_q30 entry beyond +-2^30");
  if (res < 1 || res > 1024) return range_error(name, ": the resolution must be 1 .. 1024 mm");
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
  if (listed.size() >= STORE_LIST_LIMIT) return range_error(name, too_many);
  *places = store_ray_table_slots(listed.size());
  WS_TRY(store_table(src, *places * 4, ts));
  store_ray_table_fill(listed.data(), listed.size(), (*ts)->host.as<StoreRaySlot>());
  return WS_OK;
}

// ---- one store fused into another under a rigid pose: the plan, the count pass, the host step and the write pass of ws_store_fuse
// (the rules are stated in warpsense_hip.h and live in ws_fuse.h; the kernels in store_fuse.hip)
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

// ---- a store at half the resolution of another: the plan and the one pass of ws_store_coarsen (the rule is stated in
// warpsense_hip.h and lives in ws_coarsen.h; the kernel in store_coarsen.hip)
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

int ws_store_fuse(ws_store *dst, ws_store *src, const ws_fuse_pose *pull, int32_t map_resolution, int32_t max_weight, uint32_t flags, uint64_t stats[6])
{
  if (!dst || !src || !pull || !stats) return invalid("ws_store_fuse: NULL argument");
  if (flags & ~WS_FUSE_COUNT_ONLY) return invalid("ws_store_fuse: unknown flag bits");
  if (dst == src) return invalid("ws_store_fuse: dst and src are the same store");
  if (dst->ctx != src->ctx) return invalid("ws_store_fuse: the stores belong to different contexts");
  if (max_weight < 1 || max_weight > 32767) return invalid("ws_store_fuse: max_weight must be 1 .. 32767");
  if ((int16_t)(dst->fill >> 16) > 0) return invalid("ws_store_fuse: the fill_entry of dst has a weight > 0");
  WS_TRY(pose_check("ws_store_fuse", pull, map_resolution));
  servers_leave(dst->ctx);
  const BothLocks locks(dst, src);
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
  return store_timing(dst, "ws_debug_store_fuse_timing", &ws_store::fuse, enable, ms_out, FUSE_PAIRS);
}

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
  const BothLocks locks(dst, src);
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
  return store_timing(dst, "ws_debug_store_coarsen_timing", &ws_store::coarsen, enable, ms_out, COARSEN_PAIRS);
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
  WS_TRY(pose_check("ws_store_changes", pull, map_resolution));
  if (band < 1) return range_error("ws_store_changes", ": band must be >= 1");
  if (free_value < band || free_value > 32767) return range_error("ws_store_changes", ": free_value must be band .. 32767");
  if (min_weight < 1 || min_weight > 32767) return range_error("ws_store_changes", ": min_weight must be 1 .. 32767");
  servers_leave(cur->ctx);
  WS_TRY(store_box_refuse("ws_store_changes", lo, hi));
  const BothLocks locks(cur, ref);
  StoreChangesCall c;
  store_box_of(cur, lo, hi, false, c.lo, c.hi);
  ws_store::Changes &q = cur->changes;
  hipStream_t s = cur->ctx->stream;
  const bool clusters = (flags & WS_CHANGES_CLUSTERS) != 0;
  std::vector<StoreRaySlot> listed;
  if (c.lo[0] <= c.hi[0]) store_list(cur, c.lo, c.hi, listed); // (else: no box and no chunk)
  if (listed.size() >= STORE_LIST_LIMIT) return range_error("ws_store_changes", ": the box overlaps 2^19 present chunks of CUR or more (4096 words each must stay below 2^31)");
  if (listed.empty()) // an empty store, or the box meets no present chunk: nothing is examined, and no plan is made (REF's limit holds all the same)
  {
    size_t n_ref = 0;
    for (const auto &kv : ref->dir) n_ref += kv.second.written ? 1 : 0;
    if (n_ref >= STORE_LIST_LIMIT) return range_error("ws_store_changes", ": REF holds 2^19 chunks or more");
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
  const size_t n_words = listed.size() * 4096u;
  WS_TRY(q.stats.alloc(CH_STATS_DEV));
  WS_TRY(store_chunk_tables(cur, q.table_host, q.table_dev, listed, store_word_table_bytes, nullptr, 0));
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
  return store_timing(cur, "ws_debug_store_changes_timing", &ws_store::changes, enable, ms_out, FRONTIER_PAIRS);
}
