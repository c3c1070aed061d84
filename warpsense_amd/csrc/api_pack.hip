// api_pack.hip — packed snapshots of the chunk store (ws_store_pack, ws_store_unpack, ws_pack_*; the format is stated in
// warpsense_hip.h and lives in ws_pack.h, the kernels in store_pack.hip): the host-only restatement of the rule, the validation of a
// header list, and the host flow of the two device calls.  Which chunks exist is the directory's word on both sides: a pack lists
// the chunks before anything is launched, an unpack hands out the slots before anything is launched.
#include <algorithm>
#include <cstring>
#include <set>
#include <vector>

#include "ws_api.h"
#include "ws_pack.h"

using namespace ws;

namespace
{
constexpr int PACK_PAIRS[3][2] = {{0, 1}, {1, 2}, {3, 4}}, UNPACK_PAIRS[3][2] = {{0, 1}, {5, 5}, {5, 5}}; // (event 5 is never marked: zeros)

StoreKey header_key(const uint32_t *h) { return {(int32_t)h[PACK_HDR_KEY], (int32_t)h[PACK_HDR_KEY + 1], (int32_t)h[PACK_HDR_KEY + 2]}; }

int pack_refuse(size_t chunk, const char *what) { return invalid("ws_pack_check: chunk " + std::to_string(chunk) + ": " + what); }

// everything of an unpack behind the argument checks; payload_host or payload_dev
int store_unpack(ws_store *st, const char *name, const uint32_t *headers, const uint32_t *payload_host, const uint32_t *payload_dev, size_t n, uint64_t payload_words,
                 uint32_t fill, uint32_t flags)
{
  if (!st || (n && !headers) || (payload_words && !payload_host && !payload_dev)) return invalid(std::string(name) + ": NULL argument");
  if (flags) return invalid(std::string(name) + ": unknown flag bits");
  WS_TRY(ws_pack_check(headers, n, payload_words));
  if (n >= 0x7fffffffull) return invalid(std::string(name) + ": more than 2^31 - 1 chunks");
  servers_leave(st->ctx);
  std::lock_guard<std::mutex> lock(st->mu);
  ws_store::Pack &q = st->pack;
  hipStream_t s = st->ctx->stream;
  if (n == 0) return WS_OK;
  std::set<StoreKey> fresh;
  for (size_t i = 0; i < n; ++i)
  {
    const auto it = st->dir.find(header_key(headers + i * PACK_HDR));
    if (it == st->dir.end()) fresh.insert(header_key(headers + i * PACK_HDR));
  }
  // every refusal before the first launch: the chunk limit and the segments, the staging of a host payload, the table
  WS_TRY(store_make_room(st, fresh.size(), name));
  if (payload_host && payload_words > q.stage.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.stage.grow((size_t)payload_words, sizeof(uint32_t)));
  }
  ws_store::Table *t = nullptr;
  WS_TRY(store_table(st, n * (PACK_HDR + 1), &t));
  WS_TRY(q.timer.arm());
  q.unpacked_last = true;
  for (const StoreKey &k : fresh) st->dir[k] = ws_store::Entry{store_take_slot(st), true}; // (the pass writes every word of them)
  uint32_t *w = t->host.as<uint32_t>();
  std::memcpy(w, headers, n * PACK_HDR * sizeof(uint32_t));
  for (size_t i = 0; i < n; ++i)
  {
    ws_store::Entry &e = st->dir[header_key(headers + i * PACK_HDR)];
    e.written = true;
    w[n * PACK_HDR + i] = e.slot;
  }
  const auto enqueue = [&]() -> int {
    WS_HIP(hipMemcpyAsync(t->dev.p, t->host.p, n * (PACK_HDR + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (payload_host && payload_words)
      WS_HIP(hipMemcpyAsync(q.stage.p, payload_host, (size_t)payload_words * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    WS_TRY(launch_store_unpack(st, q, t->dev.as<uint32_t>(), n, payload_host ? q.stage.as<uint32_t>() : payload_dev, fill));
    WS_HIP(hipEventRecord(t->done, s));
    t->used = true;
    return WS_OK;
  };
  const int rc = enqueue();
  if (rc != WS_OK) // the created chunks leave the directory again; launches already enqueued still run
  {
    (void)hipStreamSynchronize(s);
    store_evict(st, fresh);
    return rc;
  }
  if (payload_host) WS_HIP(hipStreamSynchronize(s)); // the caller's payload may be reused
  return WS_OK;
}
} // namespace

// ---- host only: no GPU, no context
int ws_pack_check(const uint32_t *headers, size_t n_chunks, uint64_t payload_words)
{
  if (n_chunks && !headers) return invalid("ws_pack_check: NULL headers");
  uint64_t running = 0;
  for (size_t i = 0; i < n_chunks; ++i)
  {
    const uint32_t *h = headers + i * PACK_HDR;
    if (i && !(header_key(h - PACK_HDR) < header_key(h))) return pack_refuse(i, "the keys do not ascend strictly");
    if (h[PACK_HDR_ZERO] != 0u) return pack_refuse(i, "header word 7 is not zero");
    uint32_t count[4] = {0, 0, 0, 0};
    for (uint32_t b = 0; b < PACK_BRICKS; ++b) ++count[pack_code(h, b)];
    if (count[3]) return pack_refuse(i, "a class code is 3");
    if (count[PACK_UNIFORM] != h[PACK_HDR_UNIFORM] || count[PACK_DENSE] != h[PACK_HDR_DENSE]) return pack_refuse(i, "the brick counts differ from the class map");
    if (pack_chunk_first(h) != running) return pack_refuse(i, "the first payload word is not the sum of the chunks before");
    running += pack_chunk_words(h); // (at most 2^18 per chunk: 2^64 is out of reach)
  }
  if (running != payload_words) return invalid("ws_pack_check: the chunks' payload words do not add up to payload_words");
  return WS_OK;
}

int ws_pack_expand_chunk(const uint32_t *header, const uint32_t *payload, uint32_t fill, uint32_t *out)
{
  if (!header || !out) return invalid("ws_pack_expand_chunk: NULL argument");
  if (!payload && pack_chunk_words(header)) return invalid("ws_pack_expand_chunk: NULL payload of a chunk that has payload words");
  for (uint32_t b = 0, at = 0; b < PACK_BRICKS; ++b)
  {
    const uint32_t c = pack_code(header, b);
    if (c == 3u) return invalid("ws_pack_expand_chunk: a class code is 3");
    for (uint32_t w = 0; w < PACK_BRICK_WORDS; ++w) out[pack_chunk_index(b, w)] = c == PACK_DEFAULT ? fill : c == PACK_UNIFORM ? payload[at] : payload[at + w];
    at += pack_class_words(c);
  }
  return WS_OK;
}

int ws_pack_chunk(const uint32_t *chunk, const int32_t key[3], uint32_t fill, uint32_t *header_out, uint32_t *payload_out, uint64_t cap_words, uint64_t *words)
{
  if (!chunk || !key || !header_out || !words) return invalid("ws_pack_chunk: NULL argument");
  uint32_t h[PACK_HDR] = {};
  for (int k = 0; k < 3; ++k) h[PACK_HDR_KEY + k] = (uint32_t)key[k];
  for (uint32_t b = 0; b < PACK_BRICKS; ++b)
  {
    const uint32_t w0 = chunk[pack_chunk_index(b, 0)];
    bool d_fill = false, d_w0 = false;
    for (uint32_t w = 0; w < PACK_BRICK_WORDS; ++w)
    {
      const uint32_t v = chunk[pack_chunk_index(b, w)];
      d_fill |= v != fill, d_w0 |= v != w0;
    }
    const uint32_t c = pack_class(d_fill, d_w0);
    pack_set_code(h, b, c);
    h[PACK_HDR_UNIFORM] += c == PACK_UNIFORM, h[PACK_HDR_DENSE] += c == PACK_DENSE;
  }
  *words = pack_chunk_words(h);
  std::memcpy(header_out, h, sizeof(h));
  if (*words > cap_words || (*words && !payload_out))
  {
    set_error("ws_pack_chunk: the chunk's payload words do not fit cap_words");
    return WS_ERR_CAPACITY;
  }
  for (uint32_t b = 0, at = 0; b < PACK_BRICKS; ++b)
  {
    const uint32_t c = pack_code(h, b);
    for (uint32_t w = 0; w < pack_class_words(c); ++w) payload_out[at + w] = chunk[pack_chunk_index(b, w)];
    at += pack_class_words(c);
  }
  return WS_OK;
}

// ---- the device calls
int ws_store_pack(ws_store *st, const int32_t *keys, size_t n_keys, uint32_t flags, size_t *n_chunks, uint64_t *payload_words, uint64_t stats[4])
{
  if (!st) return invalid("ws_store_pack: store is NULL");
  if (flags & ~WS_PACK_EMIT_DIRECT) return invalid("ws_store_pack: unknown flag bits");
  if (n_keys && !keys) return invalid("ws_store_pack: n_keys > 0 with NULL keys");
  servers_leave(st->ctx);
  std::lock_guard<std::mutex> lock(st->mu);
  // the chunks of the call, ascending: a directory decision, before anything is launched
  std::vector<StoreRaySlot> listed;
  if (keys)
  {
    std::set<StoreKey> named;
    for (size_t i = 0; i < n_keys; ++i)
      if (!named.insert(StoreKey{keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]}).second) return invalid("ws_store_pack: a key is named twice");
    for (const StoreKey &k : named)
    {
      const auto it = st->dir.find(k);
      if (it == st->dir.end() || !it->second.written) return invalid("ws_store_pack: the store does not hold a named chunk");
      listed.push_back(StoreRaySlot{k[0], k[1], k[2], it->second.slot});
    }
  }
  else
    for (const auto &kv : st->dir)
      if (kv.second.written) listed.push_back(StoreRaySlot{kv.first[0], kv.first[1], kv.first[2], kv.second.slot});
  const size_t n = listed.size();
  ws_store::Pack &q = st->pack;
  hipStream_t s = st->ctx->stream;
  WS_TRY(q.timer.arm());
  q.unpacked_last = false;
  q.n = 0, q.n_words = 0; // (whatever happens from here on, the old result is gone: its buffers may be replaced)
  if (n_chunks) *n_chunks = 0;
  if (payload_words) *payload_words = 0;
  for (int k = 0; k < 4 && stats; ++k) stats[k] = 0;
  if (n == 0) return WS_OK;
  WS_TRY(q.words.alloc(3));
  if (n * PACK_HDR > q.headers.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.headers.grow(n * PACK_HDR, sizeof(uint32_t)));
  }
  ws_store::Table *t = nullptr;
  WS_TRY(store_table(st, n * 4, &t));
  std::memcpy(t->host.p, listed.data(), n * sizeof(StoreRaySlot));
  const auto finish = [&](int rc) { // the table is free again when the call returns, whatever happened
    (void)hipEventRecord(t->done, s);
    t->used = true;
    if (rc != WS_OK) (void)hipStreamSynchronize(s);
    return rc;
  };
  const auto count = [&]() -> int {
    WS_HIP(hipMemcpyAsync(t->dev.p, t->host.p, n * sizeof(StoreRaySlot), hipMemcpyHostToDevice, s));
    WS_TRY(launch_store_pack_count(st, q, t->dev.p, n));
    WS_TRY(q.words.fetch(s, 3));
    WS_HIP(hipStreamSynchronize(s)); // the one host read the call needs: the payload is sized from the scanned total
    return WS_OK;
  };
  int rc = count();
  if (rc != WS_OK) return finish(rc);
  const uint64_t total = q.words.host[0], n_uniform = q.words.host[1], n_dense = q.words.host[2];
  rc = q.payload.grow((size_t)total, sizeof(uint32_t));
  if (rc == WS_OK && total)
  {
    rc = launch_store_pack_emit(st, q, t->dev.p, n, (flags & WS_PACK_EMIT_DIRECT) != 0, q.payload.cap);
    if (rc == WS_OK)
    {
      const hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize (emit pass)", __FILE__, __LINE__);
    }
  }
  if (finish(rc) != WS_OK) return rc;
  q.n = n, q.n_words = total;
  if (n_chunks) *n_chunks = n;
  if (payload_words) *payload_words = total;
  if (stats)
  {
    stats[0] = (uint64_t)n * PACK_BRICKS - n_uniform - n_dense, stats[1] = n_uniform, stats[2] = n_dense;
    stats[3] = ((uint64_t)n * PACK_HDR + total) * sizeof(uint32_t);
  }
  return WS_OK;
}

const uint32_t *ws_store_pack_headers_dev(const ws_store *st, size_t *n_chunks)
{
  if (n_chunks) *n_chunks = st ? st->pack.n : 0;
  return st && st->pack.n ? st->pack.headers.as<uint32_t>() : nullptr;
}

const uint32_t *ws_store_pack_payload_dev(const ws_store *st, uint64_t *payload_words)
{
  if (payload_words) *payload_words = st ? st->pack.n_words : 0;
  return st && st->pack.n_words ? st->pack.payload.as<uint32_t>() : nullptr;
}

int ws_store_pack_download(ws_store *st, uint32_t *headers_host, uint32_t *payload_host, size_t cap_chunks, uint64_t cap_words, size_t *n_chunks,
                           uint64_t *payload_words)
{
  if (!st || !n_chunks || !payload_words) return invalid("ws_store_pack_download: NULL argument");
  std::lock_guard<std::mutex> lock(st->mu);
  const ws_store::Pack &q = st->pack;
  *n_chunks = q.n, *payload_words = q.n_words;
  if ((headers_host && cap_chunks < q.n) || (payload_host && cap_words < q.n_words))
  {
    set_error("ws_store_pack_download: the capacities are too small for the last ws_store_pack");
    return WS_ERR_CAPACITY;
  }
  hipStream_t s = st->ctx->stream;
  if (headers_host && q.n) WS_HIP(hipMemcpyAsync(headers_host, q.headers.p, q.n * PACK_HDR * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (payload_host && q.n_words) WS_HIP(hipMemcpyAsync(payload_host, q.payload.p, (size_t)q.n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  WS_HIP(hipStreamSynchronize(s));
  return WS_OK;
}

int ws_store_unpack(ws_store *st, const uint32_t *headers_host, const uint32_t *payload_host, size_t n_chunks, uint64_t payload_words, uint32_t fill, uint32_t flags)
{
  return store_unpack(st, "ws_store_unpack", headers_host, payload_host, nullptr, n_chunks, payload_words, fill, flags);
}

int ws_store_unpack_dev(ws_store *st, const uint32_t *headers_host, const uint32_t *payload_dev, size_t n_chunks, uint64_t payload_words, uint32_t fill, uint32_t flags)
{
  return store_unpack(st, "ws_store_unpack_dev", headers_host, nullptr, payload_dev, n_chunks, payload_words, fill, flags);
}

int ws_debug_store_pack_timing(ws_store *st, int32_t enable, float ms_out[3])
{
  if (!st) return invalid("ws_debug_store_pack_timing: store is NULL");
  std::lock_guard<std::mutex> lock(st->mu);
  return query_timing(st->ctx->stream, st->pack.timer, enable, ms_out, st->pack.unpacked_last ? UNPACK_PAIRS : PACK_PAIRS, 3);
}
