// map_frontier.hip — the frontier of a device map (gfx950; ws_map_frontier, include/warpsense_hip.h): the observed-free voxels of a box
// that touch a never-observed voxel of the box, as the ORDERED stream compaction of map_surface.hip with the 7-point rule of
// ws_frontier.h in place of its 1-point predicate, and the clustering of the sorted records, which the frontier of the chunk store
// (store_frontier.hip) runs as well.
//
//   frontier_kernel<COUNT>     frontier voxels per (x, y) column of the box, and per workgroup (FR_COLS consecutive columns)
//   frontier_scan_kernel       exclusive scan of the workgroup totals (one workgroup; the last element is the total)
//   frontier_kernel<EMIT>      the rule again; a record goes to (workgroup base + columns before + rank inside the column)
//
// A wave takes a column 64 world z at a time, lane = z: the ring's seam along z falls between two lanes, the loads of a wave are two
// contiguous runs at most.  Only where a lane's voxel is FREE does the wave read the neighbours: the same z of the four neighbour
// columns through the ring's offset, and z - 1, z + 1 across the wrap.  A neighbour outside the box is not read.
//
//   fc_init_kernel             every record its own parent
//   fc_link_kernel             a record finds its up to 13 EARLIER 26-neighbours by binary search in the sorted records (four columns
//                              and its predecessor) and unites with each: the larger root is hooked under the smaller by a
//                              compare-and-swap, so the root of a component ends as its smallest record index whatever the order
//   fc_flatten_kernel          root of every record; root == self marks a cluster head; heads per workgroup
//   fc_scan_kernel             exclusive scan of those (the last element is the number of clusters, which the host reads)
//   fc_number_kernel           a head's number is its rank among the heads; it writes its row of the table, empty
//   fc_label_kernel            label = number of the root; count, lo, hi and sum by integer atomics, a wave whose lanes all carry one
//                              label reduces first (records are sorted: most waves do)
//
// Plain launches on the context's stream; no workgroup waits for another.  The only loops without a fixed trip count are the binary
// searches and the find / hook retries, which strictly descend.  The parent words are read and written by workgroups on different
// XCDs inside fc_link_kernel, whose L2s are not coherent with each other: they are accessed with agent-scope atomic loads and
// compare-and-swaps only, never with plain loads.
#include "ws_frontier.h"
#include "ws_mesh.h" // block_scan_256

namespace ws
{
constexpr int FR_COLS = 16; // columns per workgroup: four per wave, one after the other
constexpr int FR_WAVES = 4;
constexpr int FR_COUNT = 0, FR_EMIT = 1;

struct FrArgs
{
  BoxArgs box;
  int32_t min_value;
  uint32_t any_weight;
  uint32_t *col_cnt;                  // [n_cols]
  uint32_t *blk_tot;                  // [workgroups]
  const unsigned long long *blk_off;  // [workgroups] exclusive scan of blk_tot
  su32x4 *rec;                        // x, y, z, mask
  unsigned long long cap;             // records the output buffer holds
};

__device__ __forceinline__ uint32_t fr_lanes_below(unsigned long long mask)
{
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// storage index of a ring coordinate one step down / up
__device__ __forceinline__ int32_t ring_step(int32_t i, int32_t size, bool up) { return up ? (i + 1 == size ? 0 : i + 1) : (i == 0 ? size - 1 : i - 1); }

template <int MODE>
__global__ __launch_bounds__(256) void frontier_kernel(FrArgs a)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t col0 = blockIdx.x * (uint32_t)FR_COLS;
  const bool any_weight = a.any_weight != 0;
  uint32_t before = 0; // EMIT: records of the workgroup's columns before column `lane`
  unsigned long long base = 0;
  if (MODE != FR_COUNT)
  {
    const uint32_t c = (lane < FR_COLS && col0 + lane < a.box.n_cols) ? a.col_cnt[col0 + lane] : 0u;
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < FR_COLS; d <<= 1)
    {
      const uint32_t t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    before = inc - c;
    base = a.blk_off[blockIdx.x];
  }
  const int32_t sx = a.box.mp.size[0], sy = a.box.mp.size[1], sz = a.box.mp.size[2];
  uint32_t wave_total = 0;
  for (int k = 0; k < FR_COLS / FR_WAVES; ++k)
  {
    const int ci = wave * (FR_COLS / FR_WAVES) + k;
    const uint32_t col = col0 + (uint32_t)ci;
    if (col >= a.box.n_cols) break; // (the same for the whole wave)
    int32_t x, y, xi, yi, zs0;
    box_column_xy(a.box, col, x, y, xi, yi, zs0);
    const int32_t xr = x - a.box.lo[0], yr = y - a.box.lo[1];
    // storage index of storage z 0 of the column and of its four neighbour columns (size[0] * size[1] < 2^31, ws_map_create)
    const int64_t cbase = (int64_t)(xi * sy + yi) * (int64_t)sz;
    const int64_t nbase[4] = {(int64_t)(ring_step(xi, sx, false) * sy + yi) * (int64_t)sz, (int64_t)(ring_step(xi, sx, true) * sy + yi) * (int64_t)sz,
                              (int64_t)(xi * sy + ring_step(yi, sy, false)) * (int64_t)sz, (int64_t)(xi * sy + ring_step(yi, sy, true)) * (int64_t)sz};
    const bool nin[4] = {xr > 0, xr + 1 < a.box.ex, yr > 0, yr + 1 < a.box.ey}; // the neighbour column lies in the box
    unsigned long long out = base + __shfl(before, ci, 64);
    uint32_t cnt = 0;
    for (int32_t z0 = 0; z0 < a.box.ez; z0 += 64)
    {
      const int32_t zr = z0 + lane;
      const bool in = zr < a.box.ez;
      int32_t zs = zs0 + zr; // zs0 < size_z and zr < ez <= size_z
      if (zs >= sz) zs -= sz;
      uint32_t raw = 0u; // (weight 0: not free)
      if (in) raw = __builtin_nontemporal_load(a.box.data + cbase + zs);
      const bool fre = in && fr_free(raw, any_weight, a.min_value);
      uint32_t mask = 0u;
      if (fre)
      {
#pragma unroll
        for (int d = 0; d < 4; ++d)
          if (nin[d] && fr_unknown(a.box.data[nbase[d] + zs], any_weight)) mask |= 1u << d;
        if (zr > 0 && fr_unknown(a.box.data[cbase + ring_step(zs, sz, false)], any_weight)) mask |= fr_bit(2, false);
        if (zr + 1 < a.box.ez && fr_unknown(a.box.data[cbase + ring_step(zs, sz, true)], any_weight)) mask |= fr_bit(2, true);
      }
      const unsigned long long b = __ballot(mask != 0u);
      if (MODE == FR_COUNT)
        cnt += (uint32_t)__popcll(b);
      else
      {
        const unsigned long long o = out + fr_lanes_below(b);
        // (the count pass sized the buffer; a map that changed in between must not write beyond it)
        if (mask != 0u && o < a.cap) fr_put_record(a.rec, o, x, y, a.box.lo[2] + zr, mask);
        out += (unsigned long long)__popcll(b);
      }
    }
    if (MODE == FR_COUNT)
    {
      if (lane == 0) a.col_cnt[col] = cnt;
      wave_total += cnt;
    }
  }
  if (MODE == FR_COUNT)
  {
    __shared__ uint32_t wtot[FR_WAVES];
    if (lane == 0) wtot[wave] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) a.blk_tot[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  }
}

// exclusive scan of the workgroup totals
__global__ __launch_bounds__(1024) void frontier_scan_kernel(const uint32_t *tot, unsigned long long *off, uint32_t n, unsigned long long *total)
{
  scan_block_totals(tot, off, n, total);
}

static uint32_t fr_blocks(uint32_t n_cols) { return (n_cols + FR_COLS - 1) / FR_COLS; }

static FrArgs fr_args(const ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t min_value, uint32_t flags, size_t cap)
{
  FrArgs a;
  a.box = box_args(m, which, lo, ext);
  a.min_value = min_value;
  a.any_weight = (flags & WS_FRONTIER_ANY_WEIGHT) ? 1u : 0u;
  a.col_cnt = static_cast<uint32_t *>(m->frontier.col_cnt.p);
  a.blk_tot = static_cast<uint32_t *>(m->frontier.blk_tot.p);
  a.blk_off = static_cast<unsigned long long *>(m->frontier.blk_off.p);
  a.rec = static_cast<su32x4 *>(m->frontier.rec.p);
  a.cap = cap;
  return a;
}

// passes 1 and 2; the total arrives in m->frontier.total.host (pinned) once the stream has been synchronised.  The workgroups are
// those of the surface cloud (surface_blocks_for): FR_COLS == SURF_COLS
int launch_frontier_count(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t min_value, uint32_t flags)
{
  const FrArgs a = fr_args(m, which, lo, ext, min_value, flags, 0);
  const uint32_t blocks = fr_blocks(a.box.n_cols);
  hipStream_t s = m->ctx->stream;
  QueryTimer &t = m->frontier.timer;
  t.mark(0, s);
  hipLaunchKernelGGL((frontier_kernel<FR_COUNT>), dim3(blocks), dim3(256), 0, s, a);
  t.mark(1, s);
  hipLaunchKernelGGL(frontier_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)a.blk_tot, static_cast<unsigned long long *>(m->frontier.blk_off.p), blocks,
                     m->frontier.total.dev);
  t.mark(2, s);
  WS_HIP(hipGetLastError());
  return m->frontier.total.fetch(s);
}

// pass 3: no record at or beyond `cap` is written
int launch_frontier_emit(ws_map *m, int which, const int32_t lo[3], const int32_t ext[3], int32_t min_value, uint32_t flags, size_t cap)
{
  const FrArgs a = fr_args(m, which, lo, ext, min_value, flags, cap);
  hipStream_t s = m->ctx->stream;
  m->frontier.timer.mark(3, s);
  hipLaunchKernelGGL((frontier_kernel<FR_EMIT>), dim3(fr_blocks(a.box.n_cols)), dim3(256), 0, s, a);
  m->frontier.timer.mark(4, s);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

// ---- the clustering of n sorted records (n < 2^31)
constexpr uint32_t FC_WG = 256;

struct FcArgs
{
  const mi32x4 *rec;                  // [n] x, y, z, mask: ascending (x, y, z)
  uint32_t n;
  uint32_t *parent;                   // [n] union-find parents; from fc_number_kernel on: the number of a head
  uint32_t *labels;                   // [n] roots; from fc_label_kernel on: the labels
  uint32_t *head_tot;                 // [workgroups]
  const unsigned long long *head_off; // [workgroups] exclusive scan of head_tot
  unsigned long long *table;          // [k_cap] rows of eight 64-bit words
  unsigned long long k_cap;           // rows the table holds
};

__device__ __forceinline__ uint32_t fc_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of record i: parents only ever point to smaller indices, the walk descends.  On its way it hands a record its grandparent
// (path halving): the word of a record that is no root only ever moves to another ancestor, further down, and no hook looks at it
__device__ __forceinline__ uint32_t fc_find(uint32_t *parent, uint32_t i)
{
  for (;;)
  {
    uint32_t p = fc_load(parent + i);
    if (p == i) return i;
    const uint32_t g = fc_load(parent + p);
    if (g == p) return p;
    (void)__hip_atomic_compare_exchange_strong(parent + i, &p, g, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    i = g;
  }
}

// one component out of the components of a and b: the larger root goes under the smaller.  A compare-and-swap that fails means that
// root has just been hooked under a smaller one by somebody else: both finds start again from where they are, further down
__device__ __forceinline__ void fc_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
  for (;;)
  {
    a = fc_find(parent, a);
    b = fc_find(parent, b);
    if (a == b) return;
    const uint32_t hi = max(a, b), lo = min(a, b);
    uint32_t expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
}

// (x, y, z) of record r before (tx, ty, tz), the order of the records; tz in 64 bits: z - 1 of the smallest int32 is a valid target
__device__ __forceinline__ bool fc_before(const mi32x4 r, int32_t tx, int32_t ty, int64_t tz)
{
  if (r.x != tx) return r.x < tx;
  if (r.y != ty) return r.y < ty;
  return (int64_t)r.z < tz;
}

__global__ __launch_bounds__(256) void fc_init_kernel(FcArgs a)
{
  const uint32_t i = blockIdx.x * FC_WG + threadIdx.x;
  if (i < a.n) a.parent[i] = i;
}

__global__ __launch_bounds__(256) void fc_link_kernel(FcArgs a)
{
  const uint32_t i = blockIdx.x * FC_WG + threadIdx.x;
  if (i >= a.n) return;
  const mi32x4 r = a.rec[i];
  // the predecessor along z is the record before
  if (i > 0)
  {
    const mi32x4 q = a.rec[i - 1];
    if (q.x == r.x && q.y == r.y && (int64_t)q.z == (int64_t)r.z - 1) fc_unite(a.parent, i, i - 1);
  }
  // the four earlier columns: (x - 1, y - 1), (x - 1, y), (x - 1, y + 1), (x, y - 1); their records of z - 1 .. z + 1 lie side by side
#pragma unroll
  for (int c = 0; c < 4; ++c)
  {
    const int dx = c < 3 ? -1 : 0, dy = c < 3 ? c - 1 : -1;
    if ((dx < 0 && r.x == INT32_MIN) || (dy < 0 && r.y == INT32_MIN) || (dy > 0 && r.y == INT32_MAX)) continue; // no such column
    const int32_t tx = r.x + dx, ty = r.y + dy;
    const int64_t tz = (int64_t)r.z - 1;
    uint32_t lo = 0, hi = i; // the first record of [0, i) that is not before (tx, ty, tz): every target lies before record i
    while (lo < hi)
    {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (fc_before(a.rec[mid], tx, ty, tz)) lo = mid + 1; else hi = mid;
    }
    for (uint32_t j = lo; j < i && j < lo + 3u; ++j)
    {
      const mi32x4 q = a.rec[j];
      if (q.x != tx || q.y != ty || (int64_t)q.z > (int64_t)r.z + 1) break;
      fc_unite(a.parent, i, j);
    }
  }
}

// the roots, and the heads per workgroup
__global__ __launch_bounds__(256) void fc_flatten_kernel(FcArgs a)
{
  const uint32_t i = blockIdx.x * FC_WG + threadIdx.x;
  uint32_t head = 0;
  if (i < a.n)
  {
    const uint32_t root = fc_find(a.parent, i);
    a.labels[i] = root;
    head = root == i ? 1u : 0u;
  }
  uint32_t c = (uint32_t)__popcll(__ballot(head != 0u));
  __shared__ uint32_t wtot[4];
  if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) a.head_tot[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

__global__ __launch_bounds__(1024) void fc_scan_kernel(const uint32_t *tot, unsigned long long *off, uint32_t n, unsigned long long *total)
{
  scan_block_totals(tot, off, n, total);
}

// a head's number, into its parent word (the parents are not read any more), and its empty row: first, count 0, lo, hi, sum, zero
__global__ __launch_bounds__(256) void fc_number_kernel(FcArgs a)
{
  __shared__ uint32_t wsum[4];
  const uint32_t i = blockIdx.x * FC_WG + threadIdx.x;
  const bool head = i < a.n && a.labels[i] == i;
  const unsigned long long k = a.head_off[blockIdx.x] + block_scan_256(head ? 1u : 0u, wsum);
  if (!head) return;
  a.parent[i] = (uint32_t)k; // fewer clusters than records
  if (k >= a.k_cap) return;   // (the scan sized the table)
  unsigned long long *row = a.table + k * 8ull;
  row[0] = (unsigned long long)i;                                                      // first, count = 0
  row[1] = (unsigned long long)(uint32_t)INT32_MAX | ((unsigned long long)(uint32_t)INT32_MAX << 32); // lo.x, lo.y
  row[2] = (unsigned long long)(uint32_t)INT32_MAX | ((unsigned long long)(uint32_t)INT32_MIN << 32); // lo.z, hi.x
  row[3] = (unsigned long long)(uint32_t)INT32_MIN | ((unsigned long long)(uint32_t)INT32_MIN << 32); // hi.y, hi.z
  row[4] = row[5] = row[6] = row[7] = 0ull;
}

__device__ __forceinline__ int32_t wave_min(int32_t v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// count, lo, hi and sum of `cnt` members into a row: integer atomics, whose result does not depend on their order
__device__ __forceinline__ void fc_row_add(unsigned long long *row, uint32_t cnt, const int32_t lo[3], const int32_t hi[3], const long long sum[3])
{
  uint32_t *w = reinterpret_cast<uint32_t *>(row);
  atomicAdd(w + 1, cnt);
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    atomicMin(reinterpret_cast<int32_t *>(w + 2 + k), lo[k]);
    atomicMax(reinterpret_cast<int32_t *>(w + 5 + k), hi[k]);
    atomicAdd(row + 4 + k, (unsigned long long)sum[k]);
  }
}

__global__ __launch_bounds__(256) void fc_label_kernel(FcArgs a)
{
  const uint32_t i = blockIdx.x * FC_WG + threadIdx.x;
  const bool in = i < a.n;
  uint32_t label = 0xffffffffu;
  mi32x4 r = {0, 0, 0, 0};
  if (in)
  {
    r = a.rec[i];
    label = a.parent[a.labels[i]]; // the number of the root, written by the launch before
    a.labels[i] = label;
  }
  const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)label);
  if (__ballot(in) == ~0ull && __ballot(label == first) == ~0ull) // a full wave of one cluster: one lane adds for all
  {
    const int32_t lo[3] = {wave_min(r.x), wave_min(r.y), wave_min(r.z)}, hi[3] = {wave_max(r.x), wave_max(r.y), wave_max(r.z)};
    const long long sum[3] = {wave_sum(r.x), wave_sum(r.y), wave_sum(r.z)};
    if ((threadIdx.x & 63) == 0 && label < a.k_cap) fc_row_add(a.table + (unsigned long long)label * 8ull, 64u, lo, hi, sum);
    return;
  }
  if (!in || label >= a.k_cap) return;
  const int32_t p[3] = {r.x, r.y, r.z};
  const long long s[3] = {r.x, r.y, r.z};
  fc_row_add(a.table + (unsigned long long)label * 8ull, 1u, p, p, s);
}

// labels and cluster table of the n records in q.rec (0 < n < 2^31).  Synchronises twice: for the number of clusters, which sizes the
// table, and at the end
int frontier_clusters(FrontierResult &q, hipStream_t s, size_t n)
{
  const uint32_t blocks = (uint32_t)((n + FC_WG - 1) / FC_WG);
  WS_TRY(q.heads.alloc(1));
  if (n > q.parent.cap || n > q.labels.cap || blocks > q.head_tot.cap || blocks > q.head_off.cap)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(q.parent.grow(n, sizeof(uint32_t)));
    WS_TRY(q.labels.grow(n, sizeof(uint32_t)));
    WS_TRY(q.head_tot.grow(blocks, sizeof(uint32_t)));
    WS_TRY(q.head_off.grow(blocks, sizeof(unsigned long long)));
  }
  FcArgs a;
  a.rec = static_cast<const mi32x4 *>(q.rec.p);
  a.n = (uint32_t)n;
  a.parent = q.parent.as<uint32_t>();
  a.labels = q.labels.as<uint32_t>();
  a.head_tot = q.head_tot.as<uint32_t>();
  a.head_off = q.head_off.as<unsigned long long>();
  a.table = nullptr;
  a.k_cap = 0;
  hipLaunchKernelGGL(fc_init_kernel, dim3(blocks), dim3(FC_WG), 0, s, a);
  hipLaunchKernelGGL(fc_link_kernel, dim3(blocks), dim3(FC_WG), 0, s, a);
  hipLaunchKernelGGL(fc_flatten_kernel, dim3(blocks), dim3(FC_WG), 0, s, a);
  hipLaunchKernelGGL(fc_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)a.head_tot, q.head_off.as<unsigned long long>(), blocks, q.heads.dev);
  WS_HIP(hipGetLastError());
  WS_TRY(q.heads.fetch(s));
  WS_HIP(hipStreamSynchronize(s)); // the table is sized from the number of heads
  const size_t k = (size_t)*q.heads.host;
  WS_TRY(q.clusters.grow(k, 64));
  a.table = q.clusters.as<unsigned long long>();
  a.k_cap = q.clusters.cap;
  hipLaunchKernelGGL(fc_number_kernel, dim3(blocks), dim3(FC_WG), 0, s, a);
  hipLaunchKernelGGL(fc_label_kernel, dim3(blocks), dim3(FC_WG), 0, s, a);
  q.timer.mark(5, s);
  WS_HIP(hipGetLastError());
  WS_HIP(hipStreamSynchronize(s));
  q.n_clusters = k;
  q.has_clusters = true;
  return WS_OK;
}

} // namespace ws
