// ws_internal.h — shared host/device definitions of libwarpsense_hip (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "warpsense_hip.h"

namespace ws
{
constexpr int MATRIX_RESOLUTION = 32768; // include/warpsense/consts.h:12-13
constexpr int WEIGHT_RESOLUTION = 64;    // include/warpsense/consts.h:9-10
constexpr int DZ_PER_DISTANCE = 100;     // (int)(tan(45/128 deg)/2 * 32768), update_tsdf.cu:49-50 (checked on the host at load)
constexpr size_t MAX_SCAN_POINTS = 1000000; // update_tsdf.h:33
constexpr int WS_FAN_TABLE = 264;           // ws_map::fan_steps: 256 fan steps + the tile grid's division constants

// ---- tiles: 4 x 4 x 64 voxels of the ring buffer's STORAGE index space (sx >> 2, sy >> 2, sz >> 6) ----
// (tall: a wave's accesses are four 256-byte z-runs, and the vertical fan of a LiDAR azimuth falls into few tiles;
// measured against 8x8x16: tile resolve 265 -> 189 us, sparse integrate 239 -> 130 us)
// A tile is the unit of the scatter's exact resolve (one workgroup folds all candidates of a tile in LDS) and of
// the sparse integrate.  Storage space, not world space: a tile's z-runs are contiguous in memory and never
// straddle the ring seam.
#ifndef WS_TILE_XB
#define WS_TILE_XB 2
#define WS_TILE_YB 2
#define WS_TILE_ZB 6
#endif
constexpr int TILE_XB = WS_TILE_XB, TILE_YB = WS_TILE_YB, TILE_ZB = WS_TILE_ZB;
static_assert(TILE_XB + TILE_YB + TILE_ZB == 10 && TILE_ZB >= 2, "a tile is 1024 voxels: 256 threads x 4 consecutive z");
constexpr int TILE_VOXELS = 1 << (TILE_XB + TILE_YB + TILE_ZB); // 1024
constexpr uint64_t KEY_INF = ~0ull;
// the voxel bytes are two planes in one allocation: [0] keyed / touched / free-space hit (VOX_*), [1] "an off-ray free-space
// candidate (tau, -weight) landed here" (blind, idempotent byte stores of the free pass)
// Where a voxel's byte lives: tile-major, and inside a tile in BRICKS of 4 x 4 x 8 voxels (128 bytes, z fastest inside a brick,
// the eight bricks of a tile one after the other): byte = tile * 1024 + vbrick(voxel in tile).  Rays of a LiDAR ring sweep
// horizontally: with one byte per voxel in the maps' own z-fastest order every voxel column is a cache line of its own and a
// wave's 64 candidates are 64 lines (2.3 CU-cycles each from the L2, 9 from beyond: tools/ta_bench.hip -- round 5's free pass,
// 28 % fewer instructions than round 4's, took the same 118 us because of them); in bricks horizontal neighbours share lines,
// a ray stays in a brick for four column changes, and a tile's bytes are ONE contiguous kilobyte for the resolve.
__host__ __device__ inline size_t vstate_plane_bytes(int64_t n_tiles) { return ((size_t)n_tiles * 1024u + 16 + 255) & ~(size_t)255; }
__host__ __device__ inline uint32_t vbrick(uint32_t local /* lx(2) ly(2) lz(6), local_of() */)
{
  return ((local & 0x38u) << 4) | ((local >> 3) & 0x78u) | (local & 7u);
}
constexpr uint32_t WS_TAIL_STATS = 65536; // per-workgroup slots of the tail march: records, flush groups (1 000 000 points / 64 rays x up to 2 workgroups), then 2 per resolve workgroup
constexpr uint32_t WS_BLOCK_STATS = 2 * WS_TAIL_STATS + 2 * 4096 + WS_TAIL_STATS; // (+ start ticks per tail workgroup of a -DWS_TAIL_TIMING build)

// ring-buffer parameters passed BY VALUE to kernels (the reference chases three device pointers per
// access, device_map.h:93-101)
struct MapParams
{
  int32_t size[3];
  int32_t pos[3];
  int32_t offset[3];
};

// ---- candidate records ---------------------------------------------------------------------
// One scatter target of a ray tail (a write_tsdf_min call, update_tsdf.cu:107-125) is ONE 64-bit word:
//   t = point | ray step | fan (38 bits) | value(16) | voxel in tile(10)
// `fan` = fan step - mid + MID (mid: the on-ray fan step, update_tsdf.cu:104; MID = 2^(F-1) - 1): ascending like the fan step
// itself, and the weight is negated iff fan != MID (update_tsdf.cu:118-121) -- no separate sign-of-weight bit.  The top 38 bits
// are unique per candidate, so ascending records == canonical serial order (the low bits never decide).
// The 38 bits are shared out PER SCAN (round 5; 20 | 13 | 5 for every scan before -- a ray of more than 8192 steps or 31 fan
// steps was dropped with WS_ERR_RANGE, which the reference has no counterpart of): a scan of n points needs P = ceil(log2 n) bits
// for the point, the rest goes to the step (up to 16 bits: 65 536 steps) and the fan (5 to 8 bits: 31 to 255 fan steps).  The
// reference's own 131 072-point scans admit 32 768 steps and 63 fan steps (40 m rays at 5 mm); a million points 8192 / 31 as
// before.  rec_format() is the one place that decides; the kernels get S and F as scalars.
constexpr int REC_VOX_BITS = 10, REC_VALUE_SHIFT = 10, REC_T_SHIFT = 26;
constexpr int T_BITS = 38;
constexpr uint64_t T_MASK = (1ull << T_BITS) - 1;
struct RecFormat
{
  int32_t S, F; // bits of the ray step and of the fan field
};
__host__ __device__ inline RecFormat rec_format(uint64_t n_points)
{
  int P = 1;
  while ((1ull << P) < n_points) ++P; // point < n <= 2^P
  const int R = T_BITS - P;            // >= 18 for n <= 2^20 (MAX_SCAN_POINTS)
  RecFormat f;
  f.F = 5 + (R - 18) / 3;
  f.S = R - f.F;
  if (f.S > 16) // (the marches carry a step in 16 bits next to the lane)
  {
    f.S = 16;
    f.F = R - 16 > 8 ? 8 : R - 16;
  }
  return f;
}
__host__ __device__ inline int32_t rec_max_steps(const RecFormat &f) { return 1 << f.S; }
__host__ __device__ inline int32_t rec_max_fan(const RecFormat &f) { return (1 << f.F) - 1; } // iter_steps the fan field holds
__host__ __device__ inline uint32_t rec_fan_mid(int32_t F) { return (1u << (F - 1)) - 1u; }
__host__ __device__ inline uint64_t make_rec(uint32_t point, int32_t step, int32_t fan_minus_mid, int32_t value, uint32_t local, int32_t S, int32_t F)
{
  // built as two 32-bit halves (the shifts are scan constants in scalar registers; 64-bit shifts by a variable are three
  // instructions each on gfx950): u = step | fan is below 2^24, t = point | u is 38 bits, the record's high word is t >> 6
  const uint32_t u = ((uint32_t)step << F) | ((uint32_t)fan_minus_mid + rec_fan_mid(F));
  const uint32_t hi = (point << (S + F - 6)) | (u >> 6);                                                                  // S + F >= 18
  const uint32_t lo = (u << REC_T_SHIFT) | (((uint32_t)value & 0xffffu) << REC_VALUE_SHIFT) | local;                      // (the top bits of u leave the word)
  return ((uint64_t)hi << 32) | lo;
}
__host__ __device__ inline int32_t rec_value(uint64_t rec) { return (int32_t)(int16_t)(uint16_t)(rec >> REC_VALUE_SHIFT); }
__host__ __device__ inline uint32_t rec_local(uint64_t rec) { return (uint32_t)rec & ((1u << REC_VOX_BITS) - 1u); }
__host__ __device__ inline bool rec_negative(uint64_t rec, uint32_t fan_mask, uint32_t fan_mid) { return (((uint32_t)(rec >> REC_T_SHIFT)) & fan_mask) != fan_mid; }

// Records live in SUB-CHUNKS of 32 (256 bytes) that belong to one tile each.  A wave of the tail march owns a run of
// sub-chunk ids (its share of the block its workgroup took from the pool, refilled 32 at a time); the first record a wave
// makes for a tile opens a sub-chunk of that run, and every later one goes straight to its place there: position = the
// record's rank among the wave's records of the tile, counted in LDS.  HBM sees a record once, where it stays.  When the wave
// is through (or its LDS bookkeeping is full) it publishes its sub-chunks: ONE atomic per tile on tile_nsub[tile] reserves
// places in the tile's entry table, tile_ent[tile][j] = id << 5 | (records - 1).  Entries beyond TILE_DIRECT go through a
// hash (tile, j) -> entry + 1.  Nobody ever waits for anybody: the resolve -- a later kernel -- reads what is there.
constexpr int SUB_BITS = 5, SUB_RECS = 1 << SUB_BITS, TILE_DIRECT = 128;
constexpr uint32_t SUB_WAVE_FIRST = 128; // sub-chunks a wave of the tail march starts with
constexpr uint32_t SUB_REFILL = 32;      // and what it asks the pool for when it runs low
#ifndef WS_TAIL_WAVES
#define WS_TAIL_WAVES 4 // waves per workgroup of the tail march (tsdf_tail.hip)
#endif
constexpr uint32_t SUB_WG_BLOCK = WS_TAIL_WAVES * SUB_WAVE_FIRST; // ... the fixed block of ids of a work item (its waves' shares side by side)
constexpr uint32_t SUB_ID_LIMIT = (1u << 27) - 2u;  // an entry is id << 5 | fill - 1, + 1 in the hash
// per-tile bytes, two planes in one allocation (tile_flag_plane_bytes apart): [0] "the free pass / an off-ray mark touched the
// tile" (plain idempotent byte stores), [1] "the tile is on the scan's list" (it has records).  The resolve visits the listed
// tiles through the list and finds the others by scanning these planes.
__host__ __device__ inline size_t tile_flag_plane_bytes(int64_t n_tiles) { return ((size_t)n_tiles + 16 + 255) & ~(size_t)255; }
constexpr uint32_t SUB_LOST = 0xffffffffu; // the pool was exhausted (scan aborted): nothing is written, nothing published
constexpr int AZ_BINS = 8192; // sort bins of the rays: polar cells around the sensor (ray_setup_block, tsdf_setup.hip); bin AZ_BINS = ray without steps

struct TileEntry // 16 bytes: one touched tile of the scan in flight
{
  uint32_t tile;
  int32_t tx, ty, tz; // tile coordinates (so that 256 threads per tile do not divide the tile id again)
};

struct TsdfCounters // device-resident
{
  // ---- the first line: what the marches hit with atomics while they run
  uint32_t chunk_cursor;  // sub-chunks handed out from the bottom of the pool by the tail march (reset by the set-up pass of the next scan)
  uint32_t n_listed;      // tiles with records (what the marches put on the tile list; final when the resolve starts; survives until the next scatter)
  uint32_t pad2[2];
  unsigned long long ub_total; // bits 0..47: sum of the per-ray record upper bounds of the scan; bits 48..63: set-up blocks that have added theirs
  uint32_t big_inserted;  // keys ever put into the (tile, chunk) hash since it was last emptied (the host empties it when it fills up)
  uint32_t free_cursor;   // sub-chunks handed out from the TOP of the pool by the free pass (one record each: a free-space candidate on a keyed voxel)
  uint32_t n_appended;    // tiles WITHOUT records the non-fused resolve has put behind the listed ones (tile_list[n_listed ...]) for the separate integrate pass;
                          // a counter of its own: every workgroup of the resolve reads n_listed on entry, so nothing may move that word while the resolve runs
  uint32_t pad0;
  // statistics of the last update (ws_tsdf_stats)
  uint32_t last_records;
  uint32_t last_contested;
  uint32_t last_listed;
  uint32_t last_runs;
  uint32_t last_free_keyed;
  uint32_t last_chunks;
  unsigned long long last_need; // record bound of the last scan
  uint32_t last_unlisted; // tiles without records (marks of the byte planes only) the resolve found by its scan
  uint32_t pad1;
  // ---- a line of their own (round 6): the words that EVERY workgroup of the free pass and of the resolve reads when it starts.
  // Next to the cursors above they shared a cache line with the launch's own atomics -- a look at `abort` at the start of the tail
  // march's workgroups took that kernel from 135 to 210 us.
  // No launch clears a word that the same launch can set (the set-up pass used to clear both while its other
  // workgroups OR-ed into them, and an OR that landed first was lost -- a ray beyond the key range then vanished without a repeat).
  alignas(128) uint32_t abort; // != 0: the scan in flight leaves no trace and is repeated: it ran out of sub-chunks (set by the marches, cleared by the set-up pass)
  uint32_t error;              // error bits since the map's buffers were last prepared (also OR-ed into the sticky host-visible error word, which is what is read)
  uint32_t range_seq;          // scan_seq of the last scan whose set-up pass found a ray beyond its key range (never cleared: only equality with
                               // the scan in flight counts, and every writer of one launch writes the same value); folded into abort by its readers
};
static_assert(offsetof(TsdfCounters, abort) % 128 == 0 && offsetof(TsdfCounters, abort) >= 128, "TsdfCounters: abort / error in a line of their own");

// device-resident Gauss-Newton state (tsdf_registration.cpp:28-96)
struct GnCore
{
  float T[16];      // total_transform, column-major
  int32_t center[3];
  float alpha;
  float prev[4];
  float it_weight_gradient;
  float epsilon;
  int32_t max_iterations;
  int32_t iterations;
  int32_t finished;
  int32_t error; // 1: the grid barrier of reg_loop_kernel timed out
};
struct GnState
{
  GnCore core;
  int64_t sums[44]; // last h(36) g(6) e c
};

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define WS_HIP(call)                                                     \
  do                                                                     \
  {                                                                      \
    hipError_t e__ = (call);                                             \
    if (e__ != hipSuccess) return ws::hip_fail(e__, #call, __FILE__, __LINE__); \
  } while (0)

#define WS_TRY(call)                        \
  do                                        \
  {                                         \
    const int rc__ = (call);                \
    if (rc__ != WS_OK) return rc__;         \
  } while (0)

// ---- the owners of every device and pinned allocation of the library.  For each of them: after a failed allocation the object is
// empty (null pointers, zero capacity), release() may be called any number of times, and a successful grow(need) leaves cap >= need.
// a device buffer whose contents are not kept when it grows
struct DevBuf
{
  enum Slack
  {
    EXACT,  // what was asked for: fixed-size members, and staging that follows boxes of gigabytes
    EIGHTH, // an eighth more: a result that gains a few records per call does not reallocate on every call
  };
  void *p = nullptr;
  size_t cap = 0; // elements
  template <typename T> T *as() { return static_cast<T *>(p); }
  template <typename T> const T *as() const { return static_cast<const T *>(p); }
  // exactly `n` elements in place of whatever it held.  The caller has synchronised the stream.
  int alloc(size_t n, size_t elem_bytes = 1)
  {
    release();
    const hipError_t e = hipMalloc(&p, n * elem_bytes);
    if (e != hipSuccess)
    {
      p = nullptr;
      return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
    }
    cap = n;
    return WS_OK;
  }
  // room for at least `need` elements.  The caller has synchronised the stream.
  int grow(size_t need, size_t elem_bytes, Slack slack = EIGHTH) { return need <= cap ? WS_OK : alloc(slack == EIGHTH ? need + need / 8 : need, elem_bytes); }
  void release()
  {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// pinned host memory; a MAPPED block is also addressed by the device, through `dev`.  Its contents are not kept when it grows
struct HostBlock
{
  enum Kind
  {
    PINNED = hipHostMallocDefault,
    MAPPED = hipHostMallocMapped,
  };
  void *p = nullptr;   // as the host addresses it
  void *dev = nullptr; // device view (MAPPED only)
  size_t cap = 0;      // elements
  template <typename T> T *as() { return static_cast<T *>(p); }
  template <typename T> const T *as() const { return static_cast<const T *>(p); }
  template <typename T> T *dev_as() { return static_cast<T *>(dev); }
  template <typename T> const T *dev_as() const { return static_cast<const T *>(dev); }
  // exactly `n` elements in place of whatever it held, zero-filled if `zero`.  Nothing on the device uses the old block any more.
  int alloc(size_t n, size_t elem_bytes, Kind kind, bool zero = false)
  {
    release();
    hipError_t e = hipHostMalloc(&p, n * elem_bytes, (unsigned)kind);
    if (e != hipSuccess) p = nullptr;
    if (e == hipSuccess && kind == MAPPED) e = hipHostGetDevicePointer(&dev, p, 0);
    if (e != hipSuccess)
    {
      release();
      return hip_fail(e, kind == MAPPED ? "hipHostMalloc (mapped)" : "hipHostMalloc", __FILE__, __LINE__);
    }
    if (zero) std::memset(p, 0, n * elem_bytes);
    cap = n;
    return WS_OK;
  }
  int grow(size_t need, size_t elem_bytes, Kind kind, bool zero = false) { return need <= cap ? WS_OK : alloc(need, elem_bytes, kind, zero); }
  void release()
  {
    if (p) (void)hipHostFree(p);
    p = dev = nullptr;
    cap = 0;
  }
};

// 64-bit words a query's kernels leave on the device, and the pinned words the host reads them from after a stream synchronise
struct DevCounter
{
  unsigned long long *dev = nullptr, *host = nullptr;
  int alloc(size_t words, bool on_device = true)
  {
    hipError_t e = hipSuccess;
    if (on_device && !dev && (e = hipMalloc((void **)&dev, words * sizeof(unsigned long long))) != hipSuccess) dev = nullptr;
    if (e == hipSuccess && !host && (e = hipHostMalloc((void **)&host, words * sizeof(unsigned long long), hipHostMallocDefault)) != hipSuccess) host = nullptr;
    if (e == hipSuccess) return WS_OK;
    release();
    return hip_fail(e, "hipMalloc / hipHostMalloc (query counter)", __FILE__, __LINE__);
  }
  // enqueue the copy into the pinned words, from `dev` unless the device words live elsewhere
  int fetch(hipStream_t s, size_t words = 1, const unsigned long long *from = nullptr)
  {
    WS_HIP(hipMemcpyAsync(host, from ? from : dev, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    return WS_OK;
  }
  void release()
  {
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = nullptr;
  }
};

// events around the launches of a query (ws_debug_*_timing)
struct QueryTimer
{
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // (the frontier marks six, the others up to five)
  bool on = false;
  uint32_t marked = 0; // bit i: ev[i] has been recorded since the last arm() / set()
  // the start of a query call: nothing recorded yet, and the events exist if they are wanted
  int arm()
  {
    marked = 0;
    if (on)
      for (hipEvent_t &e : ev)
        if (!e) WS_HIP(hipEventCreate(&e));
    return WS_OK;
  }
  void mark(int i, hipStream_t s)
  {
    if (!on) return;
    (void)hipEventRecord(ev[i], s);
    marked |= 1u << i;
  }
  // ms_out[k]: from event pairs[k][0] to event pairs[k][1] of the last call, 0 unless that call recorded both
  int read(float *ms_out, const int (*pairs)[2], int n, hipStream_t s)
  {
    if (!ms_out) return WS_OK;
    for (int k = 0; k < n; ++k) ms_out[k] = 0.f;
    if (!marked) return WS_OK;
    WS_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < n; ++k)
      if ((marked >> pairs[k][0]) & (marked >> pairs[k][1]) & 1u) WS_HIP(hipEventElapsedTime(&ms_out[k], ev[pairs[k][0]], ev[pairs[k][1]]));
    return WS_OK;
  }
  // enable < 0: leave as it is; 0: off; 1: on, with a fresh set of events (those of an earlier enabled period are not read again)
  void set(int32_t enable)
  {
    if (enable < 0) return;
    if (!enable || !on) release();
    on = enable != 0;
    marked = 0;
  }
  void release()
  {
    for (hipEvent_t &e : ev)
    {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
};

// ---- what a mesh call and a ray-cast call leave behind, whatever they ran over: the window of a map (ws_map::Mesh, ws_map::Raycast)
// or the chunks of the store (ws_store::Mesh, ws_store::Ray).  Everything is allocated on first use and grown on demand; the one flow
// of each query (mesh_run, raycast_run in ws_api.h) and the launchers of the four .hip files take these, not their owners.
struct MeshResult
{
  QueryTimer timer;                    // 0 count passes 1 scans 2, 3 emit passes 4
  DevBuf scratch;                      // bytes: bit planes, per-word bases and counts, workgroup totals and their scans (mesh_scratch_bytes)
  DevCounter total;                    // pinned half only: vertices, quads (the device words are in `scratch`)
  DevBuf vert, face;                   // 16-byte vertices; 3 indices per face
  size_t nv = 0, nf = 0;               // vertices and faces of the last call
  void release() { timer.release(), total.release(); for (DevBuf *b : {&scratch, &vert, &face}) b->release(); }
};
struct RayResult
{
  QueryTimer timer;                    // 0 upload 1 march 2 gradient 3
  DevBuf dirs, rec, grad;              // int32 [rays][3] staging of host directions; 16-byte records; int32 [rays][3]
  DevCounter hits;                     // records with range_mm >= 0
  size_t n = 0;                        // rays of the last call
  bool has_grad = false;               // the last call also wrote `grad`
  void release() { timer.release(), hits.release(); for (DevBuf *b : {&dirs, &rec, &grad}) b->release(); }
};
// ... a surface call (ws_map::Surface, ws_store::Surface; the one flow is surface_run in ws_api.h): the per-workgroup totals of the
// count pass and their scan, and the two outputs.  What a source counts per column or per word is its own
struct SurfResult
{
  QueryTimer timer;                    // events around the launches: 0 count 1 scan 2, 3 emit 4
  DevBuf blk_tot, blk_off;             // uint32 / uint64 [workgroups of the emit pass] qualifying voxels, and their exclusive scan
  DevCounter total;                    // the scan's last element
  DevBuf rec, marker;                  // 16-byte records; 7 floats per record
  size_t n = 0;                        // records of the last call
  bool has_marker = false;             // the last call also wrote `marker`
  void release() { timer.release(), total.release(); for (DevBuf *b : {&blk_tot, &blk_off, &rec, &marker}) b->release(); }
};
// ... and a distance call (ws_map::Distance, ws_store::Dist; the one flow is distance_run in ws_api.h)
struct DistResult
{
  QueryTimer timer;                    // 0 pass 0, 1 x 2 y 3 z 4
  DevBuf rec;                          // uint32: one record per voxel (per column under WS_DISTANCE_COLUMNS)
  DevBuf plane;                        // 2 x uint16 per record: ping-pong planes of the running minimum
  DevCounter sites;                    // site voxels / site columns of the last call
  size_t n = 0;                        // records of the last call
  // what ws_map_reach / ws_store_reach need of the last call beside its records: `have` once a call has succeeded (n may be 0),
  // its box (first voxel and extent; ext[2] is not read under WS_DISTANCE_COLUMNS) and its flags; ws_map_clearance / ws_store_clearance
  // need its clamp besides (max_dist_vox: no d2 of the records exceeds R R)
  bool have = false;
  int32_t lo[3] = {0, 0, 0};
  uint32_t ext[3] = {0, 0, 0};
  uint32_t flags = 0;
  int32_t R = 0;
  void release() { timer.release(), sites.release(), have = false, n = 0; for (DevBuf *b : {&rec, &plane}) b->release(); }
};
// ... and a ground call (ws_map::Ground, ws_store::Ground; the one flow is ground_run in ws_api.h, the rules are in ws_ground.h)
constexpr int32_t GROUND_MAX_CLEAR = 64;         // clear_vox: a step of the column walk carries ONE 64-bit word of the step above (ws_ground.h)
constexpr uint32_t GROUND_PER_LAUNCH = 1u << 24; // columns of one launch of a ground pass
struct GroundResult
{
  QueryTimer timer;                    // 0 pass 1 (levels) 1 pass 2 (steps) 2
  DevBuf lvl, rec;                     // 8 bytes per column: the records of pass 1 (step 0), and the records of the result
  DevCounter counts;                   // columns per class [4]
  size_t n = 0;                        // records of the last call
  // what ws_map_ground_distance / ws_store_ground_distance need of the last call beside its records: `have` once a call has
  // succeeded (n may be 0), and its box (first voxel and extent; ext[2] saturates at 2^32 - 1)
  bool have = false;
  int32_t lo[3] = {0, 0, 0};
  uint32_t ext[3] = {0, 0, 0};
  void release() { timer.release(), counts.release(), have = false, n = 0; for (DevBuf *b : {&lvl, &rec}) b->release(); }
};
// ... and a sample call (ws_map::Sample, ws_store::Sample; the one flow is sample_run in ws_api.h)
struct SampleResult
{
  QueryTimer timer;                    // 0 upload 1 sample pass 2 scan and emit pass 3
  DevBuf pts, rec, grad, sel;          // int32 [points][3] staging of host points; 16-byte records; int32 [points][3]; int32 [selected][3]
  DevBuf blk_tot, blk_off;             // uint32 / uint64 [workgroups] selected points, and their exclusive scan
  DevCounter counts;                   // points per class [4], then the scan's total
  size_t n = 0, n_sel = 0;             // points and selected points of the last call
  bool has_grad = false, has_sel = false; // the last call also wrote `grad` / `sel`
  void release() { timer.release(), counts.release(); for (DevBuf *b : {&pts, &rec, &grad, &sel, &blk_tot, &blk_off}) b->release(); }
};
// ... and a frontier call (ws_map::Frontier, ws_store::Frontier): its extraction IS a surface call (surface_run in ws_api.h; no marker),
// and with WS_FRONTIER_CLUSTERS the clustering of the sorted records follows (frontier_clusters, map_frontier.hip)
struct FrontierResult : SurfResult // timer: 0 count 1 scan 2, 3 emit 4 clustering 5
{
  DevBuf parent, labels;               // uint32 [records]: union-find parents, then the heads' numbers; roots, then the labels
  DevBuf head_tot, head_off;           // uint32 / uint64 [records / 256] cluster heads per workgroup, and their exclusive scan
  DevCounter heads;                    // the scan's last element: the number of clusters
  DevBuf clusters;                     // 64-byte rows
  size_t n_clusters = 0;               // rows of the last call
  bool has_clusters = false;           // the last call also wrote `labels` and `clusters`
  void release() { SurfResult::release(), heads.release(); for (DevBuf *b : {&parent, &labels, &head_tot, &head_off, &clusters}) b->release(); }
};
// ... and a reach call (ws_map::Reach, ws_store::reach; the one flow is reach_run in ws_api.h, the kernels are in map_reach.hip).  The
// result carries its own box: lookups and paths need the costs alone, so a later distance call leaves it valid.
struct ReachBox // the box of a reach result as its kernels take it (ws_reach.h)
{
  int32_t lo[3];    // first world voxel
  uint32_t e[3];    // extents of the record index (a, b, c), c fastest: (nx, ny, nz), and (1, nx, ny) under WS_DISTANCE_COLUMNS
  uint32_t columns; // != 0: a = 0, b = x - lo[0], c = y - lo[1], z is ignored
};
struct ReachResult
{
  QueryTimer timer;                    // 0 seeding 1 rounds 2 count 3
  DevBuf cost;                         // uint32: one cost per record of the distance result
  DevBuf mark, list;                   // uint32 [tiles]: the last round a tile was queued for; uint32 [2][tiles]: the tile lists of this round and the next
  DevBuf seeds;                        // int32 [seeds][3] staging of the host seeds
  DevCounter words;                    // [0] kept seeds [1] reached records [2] [3] lengths of the two tile lists
  DevBuf pts, out;                     // staging of a host lookup: int32 [points][stride], uint32 [points]
  DevBuf goals, hdr, steps;            // paths: int32 [goals][3], 16-byte headers, 16-byte records [goals][cap_steps]
  size_t n = 0;                        // costs of the last call
  bool have = false;                   // a call has succeeded since the last failure (n may be 0)
  ReachBox box = {};
  std::vector<uint32_t> active;        // the tiles listed per round of the last call (ws_debug_reach_active)
  void release()
  {
    timer.release(), words.release(), have = false, n = 0;
    for (DevBuf *b : {&cost, &mark, &list, &seeds, &pts, &out, &goals, &hdr, &steps}) b->release();
  }
};
// ... and a view-gain call (ws_map::Gain, ws_store::Gain; the one flow is gain_run in ws_api.h, the rules are in ws_gain.h)
struct GainResult
{
  QueryTimer timer;                    // 0 upload 1 fan preparation and march 2 maximum 3
  DevBuf org, dirs;                    // int32 [views][3], int32 [rays][3]: staging of the host arrays
  DevBuf prep;                         // 32 bytes per ray of the fan: what depends on the direction alone
  DevBuf rec, rays;                    // 32-byte view records; 8-byte ray records [views][rays]
  DevCounter best;                     // the largest unknown_k2 of the last call
  size_t m = 0, n = 0;                 // views and rays of the last call
  bool has_rays = false;               // the last call also wrote `rays`
  void release() { timer.release(), best.release(), m = n = 0; for (DevBuf *b : {&org, &dirs, &prep, &rec, &rays}) b->release(); }
};
// ... and a clearance call (ws_map::Clearance, ws_store::clear; the one flow is clearance_run in ws_api.h, the rules are in
// ws_clearance.h, the kernels in map_clearance.hip: they read the records of a distance result alone)
struct ClearanceResult
{
  QueryTimer timer;                    // 0 upload 1 trajectories 2 best 3
  DevBuf poses, body;                  // int32 [trajectories x poses][12] staging of host poses; int32 [64][4] the body
  DevBuf rec, pose_rec;                // 32-byte trajectory records; 8-byte pose records [trajectories][poses]
  DevCounter best;                     // the index of the best trajectory as int64, -1 for none
  size_t t = 0, p = 0;                 // trajectories and poses per trajectory of the last call
  bool has_poses = false;              // the last call also wrote `pose_rec`
  void release() { timer.release(), best.release(), t = p = 0; for (DevBuf *b : {&poses, &body, &rec, &pose_rec}) b->release(); }
};

} // namespace ws

struct ws_context
{
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // profiling
  uint32_t prof_mask = 0;
  struct Span
  {
    hipEvent_t a, b;
    int cls;
  };
  std::vector<Span> spans;       // recorded, not yet resolved
  std::vector<hipEvent_t> pool;  // free events
  std::mutex lists_mu;           // guards the two lists below (objects are created and destroyed while another thread's call walks them)
  std::vector<struct ws_map *> maps; // maps of this context (sticky device-side errors are reported at ws_sync)
  std::vector<struct ws_reg *> regs; // registrations of this context (a resident server of ws_reg_iterate is asked to leave by whoever enqueues other work)
  double prof_ms[WS_K_COUNT] = {};
  int64_t prof_n[WS_K_COUNT] = {};
};

struct ws_map
{
  ws_context *ctx = nullptr;
  ws::MapParams par[2]; // [WS_MAP_AVG], [WS_MAP_NEW]
  int64_t n_vox = 0;
  ws::DevBuf data[2];       // uint32 [n_vox] (+ 16 bytes: the tile kernels read the four voxels of a column as one access, also at the very end)
  ws::DevBuf vstate;        // uint8: two planes of one byte per voxel, tile-major in bricks (vstate_plane_bytes, vbrick): keyed / touched by free space / free-space hit on a keyed voxel; off-ray free-space hit
  ws::DevBuf rays;          // per-ray set-up records (sizeof(RaySetup) x 1 000 000)
  ws::DevBuf az_hist, az_off, ray_order; // uint32: rays grouped by direction bin
  ws::DevBuf ray_bin;       // [1 000 000] uint2: (direction bin, rank inside the bin) per ray
  ws::DevBuf fan_steps;     // int32 [256] first ray step whose fan has j + 1 targets (depends on res only), see tail_bound
  int32_t fan_steps_host[ws::WS_FAN_TABLE] = {}; // staging of the same (lives as long as the map: async upload); [256..259]: division constants of ntz, nty
  bool prepped = false; // the scatter's scratch (histograms, tile counters, free-space hash) is zero / empty
  int32_t tau = 0, max_weight = 0, res = 0;
  bool new_is_default = false; // new_map known to be (tau,0) everywhere
  int integrate_mode = WS_INTEGRATE_SPARSE;
  ws::DevBuf scan_dev;      // int32: 1 000 000-point upload buffer
  // tile grid (4 x 4 x 64 voxels of storage space)
  int32_t ntx = 0, nty = 0, ntz = 0;
  int64_t n_tiles = 0;
  ws::DevBuf tile_nsub;     // uint32 [n_tiles] sub-chunks (= entries) of the tile in the scan in flight (zero between scans)
  ws::DevBuf tile_ent;      // uint32 [n_tiles][TILE_DIRECT] entries: sub-chunk id << 5 | records - 1 (never cleared: tile_nsub says how many are valid)
  ws::DevBuf tile_dirty;    // uint8: two planes of [n_tiles] bytes (tile_flag_plane_bytes): touched by the free-space pass / an off-ray mark; on the list
  ws::DevBuf tile_list;     // TileEntry [n_tiles] touched tiles of the scan in flight
  // candidate records of the ray tails: the pool of sub-chunks (32 x 8 bytes)
  ws::DevBuf rec;           // uint64
  uint32_t sub_cap = 0;
  ws::DevBuf big_keys;      // uint64: (tile, entry number) -> entry + 1 for entries beyond TILE_DIRECT: keys, then uint32 values
  uint32_t big_slots = 0;
  ws::DevBuf block_stats;   // uint32: per-workgroup statistics (no shared counters in the hot kernels)
  uint32_t tail_blocks = 0;        // workgroups of the last tail march
  uint32_t resolve_blocks = 0;     // workgroups of the last tile resolve
  bool fused_done = false;         // the last scatter already integrated into avg_map
  uint32_t scan_seq = 0;           // scatters launched on this map (ray_setup reports its record bound under this number)
  uint64_t chunk_budget_bytes = 0; // (test entry, unused since round 4's sub-chunks: the pool is always sized by estimate)
  uint32_t est_shift = 0;          // the pool's share for the records is the record bound / 32 >> (est_shift - 1) (0: the whole bound; tests shrink it to force the abort route)
  ws::DevBuf counters;         // TsdfCounters
  ws::HostBlock counters_host; // pinned copy of the same (ws_tsdf_stats)
  ws::HostBlock status;                      // uint32, mapped: [0] sticky error bits, [4..5] record bound of the scan in flight (u64), [6] its sequence number,
                                             // [8] sequence number of the last scan whose marches have finished, [9] != 0: that scan was aborted (bit 0 pool exhausted, bit 1 key range),
                                             // [10] keys in the (tile, entry) hash
  ws::DevBuf box_stage;          // uint32: device staging for ws_map_extract_box / ws_map_insert_box
  uint32_t last_error_bits = 0;  // device error bits already taken from `status`, not yet shown by ws_tsdf_stats
  // The map queries: each keeps the result of its last call and the scratch of its passes apart from the others', all of it allocated
  // on first use and grown on demand.  `mu` serialises the calls that use them (the reference's readers hold a SHARED lock).
  struct Surface : ws::SurfResult // ws_map_surface (map_surface.hip)
  {
    std::mutex mu;
    ws::DevBuf col_cnt;                  // uint32 [columns of the box] qualifying voxels per (x, y) column
    void release() { SurfResult::release(), col_cnt.release(); }
  } surf;
  struct Mesh : ws::MeshResult // ws_map_mesh (map_mesh.hip)
  {
    std::mutex mu;
  } mesh;
  struct Raycast : ws::RayResult // ws_map_raycast (map_raycast.hip)
  {
    std::mutex mu;
  } ray;
  struct Distance : ws::DistResult // ws_map_distance (map_distance.hip)
  {
    std::mutex mu;
  } dist;
  struct Ground : ws::GroundResult // ws_map_ground (map_ground.hip); ws_map_ground_distance holds mu, then dist.mu
  {
    std::mutex mu;
  } ground;
  struct Sample : ws::SampleResult // ws_map_sample (map_sample.hip)
  {
    std::mutex mu;
  } sample;
  struct Frontier : ws::FrontierResult // ws_map_frontier (map_frontier.hip)
  {
    std::mutex mu;
    ws::DevBuf col_cnt;                  // uint32 [columns of the box] frontier voxels per (x, y) column
    void release() { FrontierResult::release(), col_cnt.release(); }
  } frontier;
  struct Reach : ws::ReachResult // ws_map_reach (map_reach.hip); a reach call holds dist.mu, then mu
  {
    std::mutex mu;
  } reach;
  struct Gain : ws::GainResult // ws_map_view_gain (map_gain.hip)
  {
    std::mutex mu;
  } gain;
  struct Clearance : ws::ClearanceResult // ws_map_clearance (map_clearance.hip); a clearance call holds dist.mu, then mu
  {
    std::mutex mu;
  } clear;
  // The scan whose verdict (did its records fit the pool?) has not been looked at yet: ws_tsdf_update* return after the
  // launches, like the reference's update_tsdf (update_tsdf.cu:165); the next call that takes this map settles it first
  // (settle_tsdf: the verdict is in host-mapped memory ~0.35 ms after the launches) and repeats the scan if it was aborted.
  // The reference's caller runs "one writer or many readers" (tsdf_mapping.cpp:62-75,114-124, tsdf_registration.cpp:54), and
  // every reader entry point settles: `active` is the lock-free fast path, `settle_mu` makes the slow path (wait for the
  // verdict; for an aborted scan: new pool, the scan again) exclusive -- a second reader waits there until the map is whole.
  struct PendingScan
  {
    std::atomic<bool> active{false};
    uint32_t seq = 0;
    size_t n = 0;  // the points are in ws_map::scan_dev (the set-up pass of the scan keeps a copy there: a repeat does not depend on the caller's buffer)
    int32_t pos[3] = {0, 0, 0}, up[3] = {0, 0, 0};
    bool fused = false;
    bool s0 = false;              // the scan went into a non-default new_map (decided when it was first launched)
    bool integrate_after = false; // ws_tsdf_update*: an integrate pass follows the scatter
    int attempts = 0;
  } pending;
  std::mutex settle_mu;
  hipStream_t shift_stream = nullptr; // second stream for asynchronous slab transfers (map shift off the scan path)
  hipEvent_t shift_event = nullptr;
  ws::DevBuf shift_stage_dev;         // uint32: packed leaving slabs
  ws::HostBlock shift_stage_host;     // pinned; the two grow together (shift_reserve)
  ws_shift *shift_open = nullptr;       // the ticket in flight
  // every allocation of the map (streams, events and the ticket are the caller's: map_free)
  void release()
  {
    for (ws::DevBuf *b : {&data[0], &data[1], &vstate, &rays, &az_hist, &az_off, &ray_order, &ray_bin, &fan_steps, &scan_dev, &tile_nsub, &tile_ent, &tile_dirty,
                          &tile_list, &rec, &big_keys, &block_stats, &counters, &box_stage, &shift_stage_dev})
      b->release();
    for (ws::HostBlock *b : {&counters_host, &status, &shift_stage_host}) b->release();
    surf.release(), mesh.release(), ray.release(), dist.release(), ground.release(), sample.release(), frontier.release(), reach.release(), gain.release(), clear.release();
  }
};

struct ws_shift
{
  ws_map *map = nullptr;
  ws_shift_plan_t plan; // the steps and their boxes (ws_shift_plan)
  size_t offset[3];     // of leaving slab i in the staging buffers (voxels)
  size_t total = 0;
};

struct ws_reg
{
  ws_context *ctx = nullptr;
  ws::DevBuf points; // int32 [cap][3]
  size_t n = 0;
  ws::DevBuf partials; // int64 [2][REG_BLOCKS][32]: reg_iter_kernel alternates, reg_pass_kernel uses [0]
  ws::DevBuf state;                  // GnState [2], double buffered by reg_iter_kernel's launch parity
  ws::HostBlock state_host;          // GnState, pinned staging
  ws::HostBlock result_host;         // GnState, mapped: the resident loop writes its final state here
  ws::HostBlock host_flag;           // int32, mapped: the device sets it when the loop has finished
  int latest = 0;                    // state buffer holding the newest state
  ws::DevBuf sums_dev;               // int64 [44]
  ws::DevBuf grid_bar;               // uint32: two sets of {abort flag, counted group accumulators} of reg_loop_kernel (alternate launches)
  ws::DevBuf pass_arrived;            // uint32: arrival counter of reg_pass_kernel (zero between launches, which are ordered on the stream)
  ws::HostBlock iter_host;            // int64, mapped: the 44 sums of ws_reg_iterate, then the call's sequence number
  uint32_t iter_seq = 0;
  // the resident server behind ws_reg_iterate (reg_server_kernel, reg_server.hip): requests travel through host-mapped memory
  ws::HostBlock srv_mail;             // ServerMail, mapped
  ws::DevBuf srv_ctl;                 // uint32: device words of the server (bell, pose, arrival counters), zero at creation
  std::atomic<uint32_t> srv_launch{0};   // id of the last server launched (0: none yet); it lives until ServerMail::exited says so
  std::atomic<bool> srv_stopping{false}; // somebody has asked that server to leave: the next request waits for it and starts a new one
  uint32_t srv_ids = 0;               // launch ids handed out
  uint32_t srv_seq = 0;               // request numbers handed out (1 .. 2^31 - 1)
  uint32_t srv_served = 0;            // the last request that was answered
  int srv_enabled = 1;                // 0: one launch per ws_reg_iterate (reg_pass_kernel), WS_REG_SERVER=0
  uint32_t srv_idle_us = 50;          // the server leaves after this long without a request
  uint32_t srv_launches = 0;          // statistics (ws_debug_reg_server)
  struct
  {
    const ws_map *map = nullptr;
    const void *points = nullptr, *map_data = nullptr;
    size_t n = 0;
    int32_t res = 0;
    uint32_t flags = 0;
    ws::MapParams par;
  } srv_sig;                          // what the living server was launched for
  uint32_t loop_launches = 0;
  bool loop_sets_clear = false;
  int loop_mode = 0;                 // WS_REG_LOOP_*
  int loop_supported = 0;            // the device holds the whole grid of reg_loop_kernel at once
  int debug_stall_next = 0;          // ws_debug_reg_stall
  int resident_fallbacks = 0;        // registrations redone with one launch per iteration after a barrier timeout
  // multi-GPU resident loop (ws_reg_peer_*): the ranks' totals meet in mailboxes in each other's HBM
  ws::DevBuf mailbox;                // own mailbox, [2][64] uint64: fine-grained device memory, which peer_own_mailbox allocates itself
  void *peer_mailbox[8] = {};        // every rank's mailbox as this process addresses it ([peer_rank] == mailbox)
  bool peer_opened[8] = {};          // opened with hipIpcOpenMemHandle (to be closed)
  ws::DevBuf peer_block_dev;         // PeerBlock
  int peer_rank = 0, peer_world = 0; // 0: not connected
  int peer_blocks = 0;               // grid of the peer loop on this rank
  bool peer_dirty = false;           // an exchange failed or was given up: the mailboxes hold partial additions until ws_reg_peer_reset / reconnect
  // ws_register_cloud_batch (reg_batch_kernel): per hypothesis a start record, then a result record; grows on demand
  ws::HostBlock batch;               // mapped; cap: hypotheses the block holds
  int batch_variant = 0;             // 1: reg_batch_kernel with the per-lane voxel cache (WS_REG_BATCH_VARIANT in the environment: tuning)
  // every allocation but the peers' mailboxes, which ws_reg_peer_disconnect closes
  void release()
  {
    for (ws::DevBuf *b : {&points, &partials, &state, &sums_dev, &grid_bar, &pass_arrived, &srv_ctl, &mailbox, &peer_block_dev}) b->release();
    for (ws::HostBlock *b : {&state_host, &result_host, &host_flag, &iter_host, &srv_mail, &batch}) b->release();
  }
};

// The chunk store (ws_store_*, map_store.hip): the global map in device memory.  64^3-voxel chunks, index x*4096 + y*64 + z like
// HDF5GlobalMap's (hdf5_global_map.cpp:53-57), in a pool that grows by segments; a chunk never moves.  The DIRECTORY (key -> slot)
// is the host's: slots are handed out before anything is launched, so which chunks exist never depends on what a kernel finds.
namespace ws
{
constexpr int32_t STORE_CS = 64, STORE_CHUNK_WORDS = STORE_CS * STORE_CS * STORE_CS;
constexpr uint32_t STORE_NEW = 0x80000000u;    // slot table of a save: the chunk was created by this call (the kernel writes all of it)
constexpr uint32_t STORE_ABSENT = 0xffffffffu; // slot table of a load: the store has no such chunk (the kernel writes fill_entry)
constexpr int STORE_TABLES = 8;                // per-call slot tables in flight: a shift enqueues up to six launches
constexpr size_t STORE_TABLE_WORDS = 8192;     // chunks a table holds from the start (a whole 1025^3 window overlaps 17^3 = 4913)
} // namespace ws

struct ws_store
{
  ws_context *ctx = nullptr;
  uint32_t fill = 0;
  uint64_t max_chunks = 0;  // 0: no limit
  uint32_t seg_shift = 0;   // a segment holds 1 << seg_shift chunks
  std::mutex mu;            // every call on the store
  struct Entry
  {
    uint32_t slot;
    bool written; // false only inside the call that created the chunk, until its first save launch (which writes it whole) is enqueued
  };
  std::map<std::array<int32_t, 3>, Entry> dir;    // chunk key -> slot, ascending (cx, cy, cz)
  std::vector<uint32_t> free_slots;               // of dropped chunks, reused first
  uint32_t next_slot = 0;                         // slots ever handed out from the segments
  std::vector<ws::DevBuf> segs;                   // uint32 [STORE_CHUNK_WORDS << seg_shift] each
  std::vector<uint32_t *> seg_ptr;                // their base pointers ...
  ws::DevBuf seg_tab;                             // ... and the copy the kernels read (rewritten when a segment is added, which waits for the stream)
  // slot tables of the calls in flight: filled in pinned memory, copied in stream order, reused once the event behind the launch
  // that read them has passed
  struct Table
  {
    ws::HostBlock host;
    ws::DevBuf dev;
    hipEvent_t done = nullptr;
    bool used = false;
  } tab[ws::STORE_TABLES];
  int tab_next = 0;
  ws::QueryTimer timer[3]; // per axis of a shift: 0 save 1 load 2 (ws_store_save_box / _load_box use the first)
  // ws_store_surface (store_surface.hip), ws_store_mesh (store_mesh.hip), ws_store_raycast (store_raycast.hip) and ws_store_distance
  // (store_distance.hip): the results of the last calls, apart from each other, and the chunk table of the call in flight; the store's
  // mutex serialises the calls
  struct Surface : ws::SurfResult
  {
    ws::DevBuf mask;                     // uint64 [4096 per listed chunk] the qualifying voxels of a word, bit = z
    ws::HostBlock table_host;            // bytes, pinned: the call's chunk tables (store_word_table_bytes); free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernels read
    void release() { SurfResult::release(), mask.release(), table_host.release(), table_dev.release(); }
  } surf;
  struct Mesh : ws::MeshResult
  {
    ws::HostBlock table_host;            // bytes, pinned: the call's chunk tables (store_mesh_table_bytes); free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernels read
    void release() { MeshResult::release(), table_host.release(), table_dev.release(); }
  } mesh;
  struct Ray : ws::RayResult
  {
    ws::HostBlock table_host;            // StoreRaySlot, pinned: the call's chunk lookup; free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernels read
    void release() { RayResult::release(), table_host.release(), table_dev.release(); }
  } ray;
  struct Dist : ws::DistResult
  {
    ws::HostBlock table_host;            // StoreRaySlot, pinned: the call's chunk lookup; free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernel reads
    void release() { DistResult::release(), table_host.release(), table_dev.release(); }
  } dist;
  struct Ground : ws::GroundResult // ws_store_ground (store_ground.hip)
  {
    ws::HostBlock table_host;            // StoreRaySlot, pinned: the call's chunk lookup; free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernel reads
    void release() { GroundResult::release(), table_host.release(), table_dev.release(); }
  } ground;
  struct Sample : ws::SampleResult // ws_store_sample (store_sample.hip)
  {
    ws::HostBlock table_host;            // StoreRaySlot, pinned: the call's chunk lookup; free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernels read
    void release() { SampleResult::release(), table_host.release(), table_dev.release(); }
  } sample;
  struct Frontier : ws::FrontierResult // ws_store_frontier (store_frontier.hip)
  {
    ws::DevBuf mask;                     // uint64 [4096 per listed chunk] the frontier voxels of a word, bit = z
    ws::HostBlock table_host;            // bytes, pinned: the call's chunk tables (store_frontier_table_bytes); free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernels read
    void release() { FrontierResult::release(), mask.release(), table_host.release(), table_dev.release(); }
  } frontier;
  struct Changes : ws::FrontierResult // ws_store_changes with this store as CUR (store_changes.hip); timer: 0 uploads and count 1 scan 2, 3 emit 4 clustering 5
  {
    ws::DevBuf mask;                     // uint64 [4096 per listed chunk] the records of a word, bit = z
    ws::HostBlock table_host;            // bytes, pinned: the call's word-space tables (store_word_table_bytes); free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernels read
    ws::DevCounter stats;                // the sums of the count pass (CH_STATS_DEV, ws_changes.h)
    void release() { FrontierResult::release(), mask.release(), table_host.release(), table_dev.release(), stats.release(); }
  } changes;
  ws::ReachResult reach; // ws_store_reach (map_reach.hip: it reads the records of `dist` alone)
  struct Gain : ws::GainResult // ws_store_view_gain (store_gain.hip)
  {
    ws::HostBlock table_host;            // StoreRaySlot, pinned: the call's chunk lookup; free again when the call returns, which synchronises
    ws::DevBuf table_dev;                // ... and the copy the kernels read
    void release() { GainResult::release(), table_host.release(), table_dev.release(); }
  } gain;
  ws::ClearanceResult clear; // ws_store_clearance (map_clearance.hip: it reads the records of `dist` alone)
  struct Fuse // ws_store_fuse with this store as DST (store_fuse.hip)
  {
    ws::DevBuf words;      // uint64 [4] the sums of the count pass, then uint32 [candidates] the per-chunk counts
    ws::HostBlock words_host; // ... and the pinned block the host reads them from
    ws::QueryTimer timer;
    void release() { words.release(), words_host.release(), timer.release(); }
  } fuse;
  struct Coarsen // ws_store_coarsen with this store as DST (store_coarsen.hip)
  {
    ws::DevBuf words;         // uint64 [2] the sums of the pass: voxels that received a value, voxels short of min_observed
    ws::HostBlock words_host; // ... and the pinned block the host reads them from
    ws::QueryTimer timer;     // 0 upload of the plan 1 the pass 2
    void release() { words.release(), words_host.release(), timer.release(); }
  } coarsen;
  struct Pack // ws_store_pack of this store, and ws_store_unpack into it (store_pack.hip)
  {
    ws::QueryTimer timer;     // a pack: 0 classify 1 scan 2, 3 emit 4; an unpack: 0 launch 1
    ws::DevBuf headers;       // uint32 [WS_PACK_HEADER_WORDS per packed chunk]
    ws::DevBuf payload;       // uint32: the payload stream
    ws::DevCounter words;     // the scan's sums: payload words, uniform bricks, dense bricks
    ws::DevBuf stage;         // uint32: the payload of a ws_store_unpack from host memory
    size_t n = 0;             // chunks of the last pack
    uint64_t n_words = 0;     // payload words of the last pack
    bool unpacked_last = false; // the timer holds an unpack's events
    void release() { timer.release(), words.release(), n = 0, n_words = 0; for (ws::DevBuf *b : {&headers, &payload, &stage}) b->release(); }
  } pack;
  void release()
  {
    pack.release();
    coarsen.release();
    fuse.release();
    gain.release();
    clear.release();
    reach.release();
    frontier.release();
    changes.release();
    surf.release();
    mesh.release();
    ray.release();
    dist.release();
    ground.release();
    sample.release();
    for (ws::DevBuf &b : segs) b.release();
    segs.clear(), seg_ptr.clear();
    seg_tab.release();
    for (Table &t : tab)
    {
      t.host.release(), t.dev.release();
      if (t.done) (void)hipEventDestroy(t.done);
      t.done = nullptr;
      t.used = false;
    }
    for (ws::QueryTimer &t : timer) t.release();
  }
};

// scan pre-processing buffers (App::preprocess on the device, scan_preprocess.hip)
struct ws_scan
{
  ws_context *ctx = nullptr;
  size_t cap = 0;         // points
  size_t table_slots = 0; // power of two >= 2 * cap
  ws::DevBuf in_stage;              // float: staging of a host cloud, grown on demand
  ws::DevBuf tmp, out;              // int32 [cap][3]
  ws::DevBuf slot_of;               // uint32 [cap]
  ws::DevBuf keys, first;           // uint64 / uint32 [table_slots]
  ws::DevBuf wg_count, wg_off;      // uint32 [workgroups]
  ws::DevBuf counters;              // uint32
  ws::HostBlock host_count;         // uint32, mapped
  ws::DevBuf sweep_table;           // int32 [WS_SWEEP_MAX_BINS][16]: the pose table of a sweep, allocated by the first sweep call
  ws::HostBlock sweep_stage;        // ... and the pinned block it is uploaded from
  size_t n_out = 0;
  void release()
  {
    for (ws::DevBuf *b : {&in_stage, &tmp, &out, &slot_of, &keys, &first, &wg_count, &wg_off, &counters, &sweep_table}) b->release();
    host_count.release();
    sweep_stage.release();
  }
};

namespace ws
{
// profiling spans around a kernel class
void prof_begin(ws_context *ctx, int cls);
void prof_end(ws_context *ctx, int cls);

// launchers implemented in the .hip files
void fill_fan_steps(int32_t *fan_steps, int32_t res, int32_t ntz, int32_t nty);
int launch_tsdf_scatter(ws_map *m, const int32_t *xyz_dev, size_t n, const int32_t scanner_pos[3], const int32_t up[3], bool fused);
int settle_tsdf(ws_map *m); // the verdict of the scan in flight (repeats an aborted scan); every entry point that takes a map calls it first
size_t ray_setup_bytes();
int launch_scatter_prep(ws_map *m);
int resize_records(ws_map *m, uint64_t sub_chunks); // api_map.hip: (re)allocate the pool (waits for the stream)
uint64_t subs_for_scan(const ws_map *m, uint64_t need_records, uint64_t n_points); // sub-chunks the pool should hold for a scan of that record bound
int launch_tsdf_integrate(ws_map *m);
int launch_tsdf_stats(ws_map *m); // fills the last_* statistics of TsdfCounters from the per-workgroup slots
int launch_box_copy(ws_map *m, const ws::MapParams &par, int which, const int32_t lo[3], const int32_t ext[3], uint32_t *box_dev, bool pack, hipStream_t stream);
// map_surface.hip: count + scan (the total arrives in ws_map::surf.total.host after a stream synchronise), then the emit pass, which
// writes no record at or beyond `cap`
size_t surface_blocks_for(int64_t n_cols);
int launch_surface_count(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t band);
int launch_surface_emit(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t band, bool marker, size_t cap);
// map_mesh.hip: bits + cells + quads + scans (the totals arrive in q.total.host after a stream synchronise), then the emit passes
size_t mesh_scratch_bytes(uint64_t n_words);
int launch_mesh_count(ws_map *m, MeshResult &q, int which, const int32_t lo[3], const int32_t ext[3], uint32_t flags);
int launch_mesh_emit(ws_map *m, MeshResult &q, int which, const int32_t lo[3], const int32_t ext[3], uint32_t flags);
// map_raycast.hip: the march and, with WS_RAYCAST_GRADIENT, the gradient pass (the hit count arrives in q.hits.host after a stream synchronise)
int launch_raycast(ws_map *m, RayResult &q, int which, const int32_t origin[3], const int32_t *dirs_dev, size_t n, int32_t max_range, uint32_t flags);
// map_sample.hip: the sample pass and, with a selection, the scan and the emit pass (the class counts arrive in q.counts.host after a
// stream synchronise)
int launch_sample(ws_map *m, SampleResult &q, int which, const int32_t *pts_dev, size_t n, int32_t band, uint32_t flags);
// map_distance.hip: pass 0 over the ring (it clears q.sites.dev and marks events 0, 1), and the line passes over the records of a box
// of extent `ext` that a pass 0 has prepared (events 1 .. 4; `plane`: two planes of one uint16 per record, the first one written by
// pass 0; under WS_DISTANCE_COLUMNS ext[2] is not read).  A line of the fastest axis holds at most DIST_MAX_LINE voxels.
constexpr uint32_t DIST_MAX_LINE = 65535u * 256u;
int launch_dist_classify(ws_map *m, DistResult &q, int which, const int32_t lo[3], const int32_t ext[3], int32_t R, uint32_t flags);
int dist_passes(hipStream_t s, QueryTimer &t, uint32_t *rec, uint16_t *plane, const uint32_t ext[3], int32_t R, uint32_t flags);
// map_ground.hip: pass 1 over the ring (it clears q.counts.dev and marks events 0, 1); pass 2 over the records of pass 1, of a window
// or of the store alike (events 1, 2); and pass 0 of ws_*_ground_distance over the records of a ground result: the classes and g0 of
// a column distance field (it clears d.sites.dev and marks events 0, 1 of d)
int launch_ground_levels(ws_map *m, GroundResult &q, int which, const int32_t lo[3], const int32_t ext[3], int32_t H, uint32_t flags);
int ground_steps(hipStream_t s, GroundResult &q, uint32_t nx, uint32_t ny);
int launch_ground_sites(hipStream_t s, const GroundResult &q, DistResult &d, uint32_t max_step, int32_t R, uint32_t flags);
int fill_u32(ws_context *ctx, uint32_t *dst, uint32_t value, int64_t n);
int launch_box_fill(ws_map *m, const ws::MapParams &par, int which, const int32_t lo[3], const int32_t ext[3], uint32_t value, hipStream_t stream);
int check_all_equal_host(const uint32_t *data, int64_t n, uint32_t value);
// map_store.hip: the inclusive world box [lo, hi] of map `which` (window parameters `par`) -> the chunks of the store (save) or back
// (load).  c0 / nc: first key and count per axis of the chunks the box overlaps; table_dev: one slot word per such chunk, x major;
// any_new: the table of a save holds a chunk flagged STORE_NEW
int launch_store_copy(ws_store *st, ws_map *m, const ws::MapParams &par, int which, const int32_t lo[3], const int32_t hi[3], const int32_t c0[3],
                      const int32_t nc[3], const uint32_t *table_dev, bool save, bool any_new, hipStream_t stream);

// store_mesh.hip: the passes of map_mesh.hip over the chunks the call lists.  The host has written the tables of `n_chunks` listed
// chunks (store_mesh_table_bytes: {B, N, P, n}, then {cx, cy, cz, slot}, then 27 neighbour positions per chunk) into
// q.table_host; the totals arrive in q.total.host after a stream synchronise
struct StoreMeshCall
{
  uint32_t n_chunks; // < 2^19: 4096 words each
  int32_t res;
  uint32_t flags;
  int32_t lo[3], hi[3]; // the box, inclusive world voxels
};
inline size_t store_word_table_bytes(size_t n_chunks) { return n_chunks * (16 + 16); } // {B, N, P, n} and {cx, cy, cz, slot}: ws_store_words.h
size_t store_mesh_table_bytes(size_t n_chunks); // those two tables, then the neighbour positions
int launch_store_mesh_count(ws_store *st, ws_store::Mesh &q, const StoreMeshCall &c);
int launch_store_mesh_emit(ws_store *st, ws_store::Mesh &q, const StoreMeshCall &c);

// store_surface.hip: the passes of map_surface.hip over the chunks the call lists.  The host has written the two word-space tables of
// `n_chunks` listed chunks ({B, N, P, n}, then {cx, cy, cz, slot}: the head of the mesh's tables) into q.table_host; the total arrives
// in q.total.host after a stream synchronise, and the emit pass writes no record at or beyond `cap`
struct StoreSurfCall
{
  uint32_t n_chunks;    // 0 < n_chunks < 2^19: 4096 words each
  int32_t band, tau, res;
  int32_t lo[3], hi[3]; // the box, inclusive world voxels
};
size_t store_surface_blocks(uint32_t n_chunks); // workgroups of the emit pass: entries of blk_tot and blk_off
int launch_store_surface_count(ws_store *st, ws_store::Surface &q, const StoreSurfCall &c);
int launch_store_surface_emit(ws_store *st, ws_store::Surface &q, const StoreSurfCall &c, bool marker, size_t cap);

// map_frontier.hip: the passes of map_surface.hip with the 7-point rule of ws_frontier.h (count + scan, the total arrives in
// q.total.host after a stream synchronise; then the emit pass, which writes no record at or beyond `cap`), and the clustering of the
// n sorted records in q.rec of a window or of the store: labels and cluster table (it synchronises once in between, for the number of
// clusters, and marks events 4 and 5)
int launch_frontier_count(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t min_value, uint32_t flags);
int launch_frontier_emit(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t min_value, uint32_t flags, size_t cap);
int frontier_clusters(FrontierResult &q, hipStream_t s, size_t n);
// store_frontier.hip: the same over the chunks the call lists.  The host has written the two word-space tables of `n_chunks` listed
// chunks and the list positions of every chunk's six face neighbours (store_frontier_table_bytes) into q.table_host
struct StoreFrontierCall
{
  uint32_t n_chunks;    // 0 < n_chunks < 2^19: 4096 words each
  int32_t min_value;
  uint32_t flags;
  int32_t lo[3], hi[3]; // the box, inclusive world voxels
};
inline size_t store_frontier_table_bytes(size_t n_chunks) { return store_word_table_bytes(n_chunks) + n_chunks * 6 * sizeof(uint32_t); }
int launch_store_frontier_count(ws_store *st, ws_store::Frontier &q, const StoreFrontierCall &c);
int launch_store_frontier_emit(ws_store *st, ws_store::Frontier &q, const StoreFrontierCall &c, size_t cap);
// store_changes.hip: the passes of ws_store_changes over the chunks of CUR the call lists, in the flow of the store's frontier.  The
// host has written the two word-space tables of the `n_chunks` listed chunks into q.table_host and enqueued the upload of REF's
// chunk lookup (`ref_places` places at ref_table_dev); the sums arrive in q.stats.host after a stream synchronise
struct StoreChangesCall
{
  uint32_t n_chunks;    // 0 < n_chunks < 2^19: 4096 words each
  ws_fuse_pose pull;
  int32_t res, band, free_value, min_weight;
  uint32_t kinds;       // WS_CHANGES_APPEARED | WS_CHANGES_VANISHED: the kinds that become records
  int32_t lo[3], hi[3]; // the box, inclusive world voxels of CUR
  const void *ref_table_dev;
  size_t ref_places;
};
int launch_store_changes_count(ws_store *cur, const ws_store *ref, ws_store::Changes &q, const StoreChangesCall &c);
int launch_store_changes_emit(ws_store *cur, const ws_store *ref, ws_store::Changes &q, const StoreChangesCall &c, size_t cap);

// store_pack.hip: the passes of ws_store_pack over the `n` chunks of `table_dev` ({cx, cy, cz, slot} each, ascending keys) into
// q.headers (classify: class maps, counts and keys; scan: the first-word indices, and q.words.dev = payload words, uniform bricks,
// dense bricks) and, once the host has sized q.payload from the total, into q.payload (emit, which writes no word at or beyond
// `cap`); and the pass of ws_store_unpack: `n` chunks whose headers and slots ({WS_PACK_HEADER_WORDS words} x n, then n slots)
// are at table_dev
int launch_store_pack_count(ws_store *st, ws_store::Pack &q, const void *table_dev, size_t n);
int launch_store_pack_emit(ws_store *st, ws_store::Pack &q, const void *table_dev, size_t n, bool direct, uint64_t cap);
int launch_store_unpack(ws_store *st, ws_store::Pack &q, const uint32_t *table_dev, size_t n, const uint32_t *payload_dev, uint32_t fill);

// map_reach.hip: the geodesic field over the records of a distance result, of a window or of the store alike.  reach_tiles: the tiles
// of a box.  launch_reach_seed clears costs, marks and words, takes the n_seeds seeds in q.seeds (it marks events 0, 1) and queues
// their tiles for round 1; launch_reach_round runs round `r` over the `active` tiles of its list; launch_reach_count counts the
// finite costs (events 2, 3).  The words arrive in q.words.host after fetch and a stream synchronise.
constexpr uint32_t REACH_INF = 0xffffffffu;
constexpr int REACH_SWEEPS = 32;             // S: sweeps of a tile in LDS per round
constexpr int REACH_VA = 8, REACH_VB = 8, REACH_VC = 8;  // the tile of a volume, in (a, b, c) of ReachBox: 512 records
constexpr int REACH_CA = 1, REACH_CB = 16, REACH_CC = 32; // the tile of a column map: 512 records, 32 along the fastest axis
constexpr uint32_t REACH_ROUNDS_PER_TILE = 64; // max_rounds = 0 stands for REACH_ROUNDS_PER_TILE x tiles + 64
uint64_t reach_tiles(const ReachBox &b);
int launch_reach_seed(ReachResult &q, hipStream_t s, const uint32_t *dist, size_t n_seeds, uint32_t clear_d2, uint32_t flags);
int launch_reach_round(ReachResult &q, hipStream_t s, const uint32_t *dist, uint32_t r, uint32_t active, uint32_t clear_d2, uint32_t flags);
int launch_reach_count(ReachResult &q, hipStream_t s);
int launch_reach_lookup(const ReachResult &q, hipStream_t s, const int32_t *pts_dev, size_t n, int32_t stride, uint32_t *out_dev);
int launch_reach_paths(ReachResult &q, hipStream_t s, size_t g, uint32_t cap_steps);

// store_raycast.hip: the march of ws_raycast.h over the chunks the call lists.  The kernels find a chunk through an open-addressing
// table key -> slot of a power-of-two size >= 2 x listed chunks (linear probing from store_ray_hash; an empty place has slot
// STORE_ABSENT), which the host has written into q.table_host; the hit count arrives in q.hits.host after a stream synchronise
struct alignas(16) StoreRaySlot
{
  int32_t cx, cy, cz;
  uint32_t slot;
};
__host__ __device__ inline uint32_t store_ray_hash(int32_t cx, int32_t cy, int32_t cz)
{
  uint32_t h = (uint32_t)cx * 0x9e3779b1u ^ (uint32_t)cy * 0x85ebca77u ^ (uint32_t)cz * 0xc2b2ae3du;
  return h ^ (h >> 15);
}
inline size_t store_ray_table_slots(size_t n_chunks)
{
  size_t s = 2;
  while (s < 2 * n_chunks) s <<= 1;
  return s;
}
// the table of `n` chunks ({cx, cy, cz, slot} each, distinct keys) into table[store_ray_table_slots(n)]
inline void store_ray_table_fill(const StoreRaySlot *chunks, size_t n, StoreRaySlot *table)
{
  const size_t slots = store_ray_table_slots(n);
  for (size_t i = 0; i < slots; ++i) table[i] = StoreRaySlot{0, 0, 0, STORE_ABSENT};
  for (size_t i = 0; i < n; ++i)
  {
    size_t at = store_ray_hash(chunks[i].cx, chunks[i].cy, chunks[i].cz) & (slots - 1);
    while (table[at].slot != STORE_ABSENT) at = (at + 1) & (slots - 1);
    table[at] = chunks[i];
  }
}
// the slot of a chunk, STORE_ABSENT if the table does not list it (at least half of the places are empty: the probe ends)
__host__ __device__ inline uint32_t store_ray_find(const StoreRaySlot *table, uint32_t mask, int32_t cx, int32_t cy, int32_t cz)
{
  for (uint32_t at = store_ray_hash(cx, cy, cz) & mask;; at = (at + 1u) & mask)
  {
    const StoreRaySlot e = table[at];
    if (e.slot == STORE_ABSENT || (e.cx == cx && e.cy == cy && e.cz == cz)) return e.slot;
  }
}
struct StoreRayCall
{
  uint32_t n_chunks;    // listed chunks (< 2^19); 0: every record is a no-hit
  int32_t res;
  int32_t lo[3], hi[3]; // the box, inclusive world voxels
  int32_t blo[3], bhi[3]; // the bounding box of the listed chunks, cut to the box
};
int launch_store_raycast(ws_store *st, ws_store::Ray &q, const StoreRayCall &c, const int32_t origin[3], const int32_t *dirs_dev, size_t n, int32_t max_range, uint32_t flags);
// store_sample.hip: the passes of map_sample.hip over the chunks the call lists, found through the lookup of store_raycast.hip in
// q.table_host (`c`: the box and the live box of a ray cast)
int launch_store_sample(ws_store *st, ws_store::Sample &q, const StoreRayCall &c, const int32_t *pts_dev, size_t n, int32_t band, uint32_t flags);

// map_gain.hip, store_gain.hip: the view gain of a checked call (gain_check, ws_api.h) whose origins and directions are in q.org and
// q.dirs: clear, fan preparation, march, maximum (events 1 .. 3; the maximum arrives in q.best.host after a stream synchronise).  For
// the store the host has written the lookup of store_raycast.hip for `n_chunks` listed chunks into q.table_host
struct GainCall
{
  size_t m, n;          // views (1 .. 65535), rays of the fan (1 .. 2^19)
  int32_t lo[3], hi[3]; // the box, inclusive world voxels (lo > hi: empty)
  int32_t res, max_range, min_value;
  uint32_t flags;
};
int launch_map_gain(ws_map *m, GainResult &q, int which, const GainCall &c);
int launch_store_gain(ws_store *st, ws_store::Gain &q, const GainCall &c, uint32_t n_chunks);

// map_clearance.hip: the trajectories of a checked call (clearance_run, ws_api.h) over the records of a distance result, of a window or
// of the store alike: the trajectory pass (events 1, 2) and the pass that finds the best (event 3; it arrives in q.best.host after a
// stream synchronise).  The body is in q.body, the poses at poses_dev
struct ClearCall
{
  size_t t, p;          // trajectories (1 .. 2^20), poses of each (1 .. 65535)
  uint32_t k;           // spheres of the body (1 .. 64)
  int32_t res, soft;
  uint32_t flags;
};
int launch_clearance(ClearanceResult &q, const DistResult &d, hipStream_t s, const ClearCall &c, const int32_t *poses_dev);

// store_distance.hip: pass 0 of the distance field over the chunks the call lists (it clears q.sites.dev and marks events 0, 1).  The
// host has written the lookup of store_raycast.hip (store_ray_table_fill) for `n_chunks` listed chunks into q.table_host
struct StoreDistCall
{
  uint32_t n_chunks;    // listed chunks (< 2^19); 0: every voxel is unknown
  int32_t lo[3], hi[3]; // the box, inclusive world voxels
  int32_t zlo, zhi;     // the z range of the listed chunks, cut to the box (zlo > zhi without a listed chunk)
  uint32_t nx, ny;      // columns of the box (nx ny < 2^32)
};
int launch_store_dist_classify(ws_store *st, ws_store::Dist &q, const StoreDistCall &c, int32_t R, uint32_t flags);

// store_ground.hip: pass 1 of the ground layer over the chunks the call lists (it clears q.counts.dev and marks events 0, 1); the
// call and the lookup are those of the distance field
int launch_store_ground_levels(ws_store *st, ws_store::Ground &q, const StoreDistCall &c, int32_t H, uint32_t flags);

// the bin rule of a sweep (ws_sweep_t, checked by api_scan.hip) and its pose table on the device
struct PreSweep
{
  const int32_t *table; // [k][16] to_int_mat(poses[b]), column-major, one 64-byte row per bin
  uint32_t k;
  uint32_t columns; // by index: bins follow the column of a point ...
  uint32_t rows;    // ... n / columns
  int32_t ring_major;
  int32_t time_field; // >= 0: by the float at this index of the point's record
  float t_begin, t_end;
};
int launch_scan_preprocess(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const int32_t M[16], int32_t res, const PreSweep *sweep = nullptr);
size_t pre_table_slots(size_t max_points);

// ---- registration: the kernels and their launchers, one file per route (the routes: head of reg_loop.hip)
// reg_loop.hip: the resident loop, alone or with peers
int launch_reg_loop(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, const ws::GnCore &init, bool peers = false, size_t first = 0, size_t count = 0);
int reg_loop_supported(int device);
size_t reg_barrier_bytes();
size_t reg_peer_block_bytes();
void reg_peer_block_fill(void *host_image, void *const mailbox[8], int rank, int world);
size_t reg_mailbox_bytes();
int reg_groups();
int reg_default_blocks();
// reg_launches.hip: one launch per iteration, one launch per call, the solve alone
int launch_reg_iteration(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, int32_t k);
// reg_pass_kernel over points [first, first + count): from the newest state (first the update from `sums` if `apply`) into `sums`;
// or, given a pose T, without a state into host-mapped `sums`, then `seq`
int launch_reg_pass(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t first, size_t count, int64_t *sums, int apply,
                    const float *T = nullptr, uint32_t seq = 0);
int launch_reg_solve(ws_reg *r, const int64_t *sums_dev);
int launch_solve6_test(ws_context *ctx, const double *A_dev, const double *b_dev, size_t n, double *x_dev, int32_t *status_dev);
size_t reg_partials_bytes();
// reg_server.hip: the resident server and the host's half of its mailbox
int launch_reg_server(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, uint32_t launch_id, uint32_t served, uint32_t idle_us);
size_t reg_server_mail_bytes();
size_t reg_server_ctl_bytes();
void reg_server_mail_write(void *mail, const float T[16], uint32_t seq);
void reg_server_mail_stop(void *mail, uint32_t launch_id);
int reg_server_mail_answer(const void *mail, uint32_t seq, int64_t sums[44]);
int reg_server_mail_selftest();
uint32_t reg_server_mail_exited(const void *mail);
// reg_batch.hip: reg_batch_kernel, k workgroups, one Gauss-Newton loop each, from the start records in ws_reg::batch into its result records
int launch_reg_batch(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t k, int32_t max_iterations, float it_weight_gradient, float epsilon);
size_t reg_batch_record_bytes(); // start + result record of one hypothesis
void reg_batch_write(void *records, size_t k, const float T[16]);
void reg_batch_read(const void *records, size_t n, size_t k, float T[16], int32_t *iterations, int32_t *e, int32_t *c);
int reg_batch_default_variant();
} // namespace ws
