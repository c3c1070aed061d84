// map_reach.hip — ws_map_reach / ws_store_reach: the cost of the cheapest path from a set of seeds to every record of a distance
// result (the rules are stated in warpsense_hip.h, their device part in ws_reach.h).  Block-wise Bellman-Ford: the box is cut into
// tiles of 512 records, a ROUND is one plain launch with one workgroup per active tile, and the host sizes the next round from one
// word.  Why this needs no hand-off inside a launch:
//   - every cost ever stored is the cost of a real step sequence from a kept seed, and costs only fall;
//   - a tile is written by ONE workgroup per round (a tile enters a round's list once: the marks are atomic maxima of round numbers);
//   - a halo value read from global memory may be the round's start or fresher -- either is a valid upper bound;
//   - whoever lowers a cost on the rim of its tile marks the tiles beyond that rim for the NEXT launch, and a tile that ran out of
//     sweeps marks itself: a record that can still be improved always lies in a tile on the next list, so an empty list is the fixed
//     point.  What one workgroup stores has to reach another only across a kernel boundary.
// No grid barrier, no flag polling, no waiting on another workgroup; the sweep loop is bounded by REACH_SWEEPS and the round loop by
// the host's max_rounds.
#include "ws_reach.h"

namespace ws
{
namespace
{
constexpr int REACH_WG = 256;

struct ReachArgs
{
  ReachBox box;
  ReachGrid grid;
  const uint32_t *dist;     // the distance records
  uint32_t *cost;
  uint32_t *mark;           // [tiles] the last round the tile was queued for (0: never)
  uint32_t *list;           // [2][tiles]: round r reads list[r & 1] and appends to the other
  unsigned long long *words; // [0] kept seeds [1] reached records [2 + i] length of list[i]
  uint32_t clear_d2, flags;
};

// the tile is queued for round `r` once, whoever asks first
__device__ inline void reach_queue(const ReachArgs &a, uint32_t tile, uint32_t r)
{
  if (atomicMax(&a.mark[tile], r) < r)
  {
    const unsigned long long at = atomicAdd(&a.words[2 + (r & 1u)], 1ull);
    if (at < (unsigned long long)a.grid.n_tiles) a.list[(size_t)(r & 1u) * a.grid.n_tiles + (size_t)at] = tile; // (always: a tile is appended once per round)
  }
}

// one thread per seed: a seed inside the box on a traversable record gets cost 0 and queues its tile for round 1
__global__ __launch_bounds__(REACH_WG) void reach_seed_kernel(ReachArgs a, const int32_t *seeds, uint32_t n_seeds)
{
  const uint32_t i = blockIdx.x * REACH_WG + threadIdx.x;
  bool kept = false;
  uint32_t p[3];
  if (i < n_seeds && reach_locate(a.box, seeds[3 * (size_t)i], seeds[3 * (size_t)i + 1], seeds[3 * (size_t)i + 2], p))
  {
    const uint32_t idx = reach_index(a.box, p[0], p[1], p[2]);
    if (reach_traversable(a.dist[idx], a.clear_d2, a.flags))
    {
      kept = true;
      a.cost[idx] = 0u;
      const uint32_t ta = p[0] / (uint32_t)(a.box.columns ? REACH_CA : REACH_VA), tb = p[1] / (uint32_t)(a.box.columns ? REACH_CB : REACH_VB),
                     tc = p[2] / (uint32_t)(a.box.columns ? REACH_CC : REACH_VC);
      reach_queue(a, (ta * a.grid.nt[1] + tb) * a.grid.nt[2] + tc, 1u);
    }
  }
  const unsigned long long b = __ballot(kept);
  if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&a.words[0], (unsigned long long)__popcll(b));
}

// the 27 tiles around a record that sits at l of 0 .. T - 1 along an axis: bit 0 the tile before (l == 0), bit 1 its own, bit 2 the one behind
__device__ inline uint32_t reach_axis_bits(uint32_t l, uint32_t T) { return 2u | (l == 0u ? 1u : 0u) | (l == T - 1u ? 4u : 0u); }

// One round of one tile of TA x TB x TC records, c fastest; a thread holds CELLS / REACH_WG of them.
template <int TA, int TB, int TC> __global__ __launch_bounds__(REACH_WG) void reach_round_kernel(ReachArgs a, uint32_t r)
{
  constexpr int HA = TA + 2, HB = TB + 2, HC = TC + 2, HN = HA * HB * HC, CELLS = TA * TB * TC, PER = CELLS / REACH_WG;
  static_assert(CELLS % REACH_WG == 0, "a tile is a multiple of the workgroup");
  __shared__ uint32_t c[HN];
  __shared__ uint32_t marks; // bit (da + 1) 9 + (db + 1) 3 + dc + 1: that tile is to run in the next round (bit 13: this one)
  const uint32_t tid = threadIdx.x;
  const uint32_t tile = a.list[(size_t)(r & 1u) * a.grid.n_tiles + blockIdx.x];
  const uint32_t tc = tile % a.grid.nt[2], tb = (tile / a.grid.nt[2]) % a.grid.nt[1], ta = tile / (a.grid.nt[2] * a.grid.nt[1]);
  const uint32_t o[3] = {ta * TA, tb * TB, tc * TC};
  if (tid == 0u)
  {
    marks = 0u;
    // the length of this round's list has been read by the host: it is the next round's target after the one this launch fills
    if (blockIdx.x == 0u) a.words[2 + (r & 1u)] = 0ull;
  }
  // the tile and its halo of one record; outside the box nothing exists
  for (uint32_t h = tid; h < (uint32_t)HN; h += REACH_WG)
  {
    const uint32_t hc = h % HC, hb = (h / HC) % HB, ha = h / (HC * HB);
    uint32_t q[3];
    uint32_t v = REACH_INF;
    if ((TA > 1 || ha == 1u) && reach_neighbour(a.box, o, (int)ha - 1, (int)hb - 1, (int)hc - 1, q)) v = a.cost[reach_index(a.box, q[0], q[1], q[2])];
    c[h] = v;
  }
  uint32_t at[PER], idx[PER], start[PER], cur[PER], rim[PER];
  bool trav[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k)
  {
    const uint32_t cell = tid + (uint32_t)k * REACH_WG;
    const uint32_t lc = cell % TC, lb = (cell / TC) % TB, la = cell / (TC * TB);
    at[k] = ((la + 1u) * HB + lb + 1u) * HC + lc + 1u;
    const bool inside = o[0] + la < a.box.e[0] && o[1] + lb < a.box.e[1] && o[2] + lc < a.box.e[2];
    idx[k] = inside ? reach_index(a.box, o[0] + la, o[1] + lb, o[2] + lc) : 0u;
    trav[k] = inside && reach_traversable(a.dist[idx[k]], a.clear_d2, a.flags);
    const uint32_t bc = reach_axis_bits(lc, TC), bb = reach_axis_bits(lb, TB), ba = reach_axis_bits(la, TA);
    const uint32_t mbc = ((bb & 1u) ? bc : 0u) | ((bb & 2u) ? bc << 3 : 0u) | ((bb & 4u) ? bc << 6 : 0u);
    rim[k] = (((ba & 1u) ? mbc : 0u) | ((ba & 2u) ? mbc << 9 : 0u) | ((ba & 4u) ? mbc << 18 : 0u)) & ~(1u << 13);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) start[k] = cur[k] = c[at[k]]; // (a record that is not traversable keeps REACH_INF for ever)
  // Jacobi sweeps in LDS: all read, barrier, the improved write, barrier
  int more = 0;
  for (int sweep = 0; sweep < REACH_SWEEPS; ++sweep)
  {
    uint32_t best[PER];
    int changed = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k)
    {
      best[k] = cur[k];
      if (!trav[k]) continue;
#pragma unroll
      for (int da = (TA > 1 ? -1 : 0); da <= (TA > 1 ? 1 : 0); ++da)
#pragma unroll
        for (int db = -1; db <= 1; ++db)
#pragma unroll
          for (int dc = -1; dc <= 1; ++dc)
          {
            if (da == 0 && db == 0 && dc == 0) continue;
            const uint32_t v = c[(int)at[k] + (da * HB + db) * HC + dc];
            if (v < best[k]) best[k] = min(best[k], v + reach_weight(da, db, dc)); // (v is finite here, and a finite cost + 17 fits)
          }
      changed |= best[k] < cur[k];
    }
    more = __syncthreads_or(changed);
    if (!more) break;
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (best[k] < cur[k]) c[at[k]] = cur[k] = best[k];
    __syncthreads();
  }
  // only this tile's records are written; the tiles beyond a lowered rim record run in the next round.  In round 1 a seed counts as
  // lowered: its cost was stored by the seeding pass, not by a workgroup that could have marked for it.
  uint32_t m = 0u;
#pragma unroll
  for (int k = 0; k < PER; ++k)
  {
    if (!trav[k]) continue;
    if (cur[k] < start[k]) a.cost[idx[k]] = cur[k];
    if (cur[k] < start[k] || (r == 1u && cur[k] != REACH_INF)) m |= rim[k];
  }
  if (tid == 0u && more) m |= 1u << 13; // out of sweeps with the last one still improving: this tile again
  if (m) atomicOr(&marks, m);
  __syncthreads();
  if (tid < 27u && ((marks >> tid) & 1u))
  {
    const int64_t na = (int64_t)ta + (int)(tid / 9u) - 1, nb = (int64_t)tb + (int)((tid / 3u) % 3u) - 1, nc = (int64_t)tc + (int)(tid % 3u) - 1;
    if (na >= 0 && nb >= 0 && nc >= 0 && na < (int64_t)a.grid.nt[0] && nb < (int64_t)a.grid.nt[1] && nc < (int64_t)a.grid.nt[2])
      reach_queue(a, ((uint32_t)na * a.grid.nt[1] + (uint32_t)nb) * a.grid.nt[2] + (uint32_t)nc, r + 1u);
  }
}

// the records with a finite cost: one atomic add per wave
__global__ __launch_bounds__(REACH_WG) void reach_count_kernel(const uint32_t *cost, uint32_t n, unsigned long long *out)
{
  const uint64_t waves = (uint64_t)gridDim.x * (REACH_WG / 64);
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long cnt = 0ull;
  for (uint64_t base = ((uint64_t)blockIdx.x * (REACH_WG / 64) + threadIdx.x / 64u) * 64u; base < n; base += waves * 64u)
  {
    const uint64_t i = base + lane;
    cnt += (unsigned long long)__popcll(__ballot(i < n && cost[i] != REACH_INF));
  }
  if (lane == 0u && cnt) atomicAdd(out, cnt);
}

// the costs at n world voxels, `stride` int32 apart
__global__ __launch_bounds__(REACH_WG) void reach_lookup_kernel(ReachBox box, const uint32_t *cost, const int32_t *pts, uint32_t n, uint32_t stride, uint32_t *out)
{
  const uint32_t i = blockIdx.x * REACH_WG + threadIdx.x;
  if (i >= n) return;
  const int32_t *q = pts + (size_t)i * stride;
  uint32_t p[3];
  out[i] = reach_locate(box, q[0], q[1], q[2], p) ? cost[reach_index(box, p[0], p[1], p[2])] : REACH_INF;
}

// One wave per goal walks back to a seed.  Lane l < 27 looks at the neighbour (l / 9 - 1, l / 3 % 3 - 1, l % 3 - 1): ascending lanes are
// ascending (da, db, dc), and the lowest lane whose neighbour explains the cost is the predecessor.
__global__ __launch_bounds__(64) void reach_paths_kernel(ReachBox box, const uint32_t *cost, const int32_t *goals, uint32_t cap, uint4 *hdr, int4 *steps)
{
  const uint32_t goal = blockIdx.x, lane = threadIdx.x;
  const int32_t gz = goals[3 * (size_t)goal + 2];
  uint32_t p[3];
  if (!reach_locate(box, goals[3 * (size_t)goal], goals[3 * (size_t)goal + 1], gz, p))
  {
    if (lane == 0u) hdr[goal] = make_uint4(REACH_INF, 0u, 0u, 2u);
    return;
  }
  uint32_t cv = cost[reach_index(box, p[0], p[1], p[2])];
  if (cv == REACH_INF)
  {
    if (lane == 0u) hdr[goal] = make_uint4(REACH_INF, 0u, 0u, 1u);
    return;
  }
  const uint32_t total = cv, bound = cv / 10u; // every step costs at least 10
  const int da = (int)(lane / 9u) - 1, db = (int)((lane / 3u) % 3u) - 1, dc = (int)(lane % 3u) - 1;
  const bool looks = lane < 27u && lane != 13u;
  const uint32_t w = reach_weight(da, db, dc);
  uint32_t n_steps = 0u, written = 0u, status = 0u;
  for (;;)
  {
    if (written < cap)
    {
      if (lane == 0u)
      {
        const int32_t x = box.lo[0] + (int32_t)(box.columns ? p[1] : p[0]), y = box.lo[1] + (int32_t)(box.columns ? p[2] : p[1]);
        steps[(size_t)goal * cap + written] = make_int4(x, y, box.columns ? gz : box.lo[2] + (int32_t)p[2], (int32_t)cv);
      }
      ++written;
    }
    if (cv == 0u || n_steps >= bound) break;
    uint32_t q[3];
    bool ok = false;
    if (looks && reach_neighbour(box, p, da, db, dc, q))
    {
      const uint32_t cn = cost[reach_index(box, q[0], q[1], q[2])];
      ok = cn != REACH_INF && cn + w == cv;
    }
    const unsigned long long found = __ballot(ok);
    if (!found) break;
    const uint32_t l = (uint32_t)__ffsll((long long)found) - 1u;
    const int la = (int)(l / 9u) - 1, lb = (int)((l / 3u) % 3u) - 1, lc = (int)(l % 3u) - 1;
    p[0] = (uint32_t)((int64_t)p[0] + la), p[1] = (uint32_t)((int64_t)p[1] + lb), p[2] = (uint32_t)((int64_t)p[2] + lc);
    cv -= reach_weight(la, lb, lc);
    ++n_steps;
  }
  if (cv != 0u) status = 3u; // no predecessor: not a fixed point (does not happen on the result of a reach call)
  if (lane == 0u) hdr[goal] = make_uint4(total, n_steps, written, status);
}

ReachArgs reach_args(ReachResult &q, const uint32_t *dist, uint32_t clear_d2, uint32_t flags)
{
  ReachArgs a;
  a.box = q.box;
  a.grid = reach_grid(q.box);
  a.dist = dist;
  a.cost = q.cost.as<uint32_t>();
  a.mark = q.mark.as<uint32_t>();
  a.list = q.list.as<uint32_t>();
  a.words = q.words.dev;
  a.clear_d2 = clear_d2, a.flags = flags;
  return a;
}
} // namespace

uint64_t reach_tiles(const ReachBox &b)
{
  const uint64_t t[3] = {(uint64_t)(b.columns ? REACH_CA : REACH_VA), (uint64_t)(b.columns ? REACH_CB : REACH_VB), (uint64_t)(b.columns ? REACH_CC : REACH_VC)};
  uint64_t n = 1;
  for (int k = 0; k < 3; ++k) n *= ((uint64_t)b.e[k] + t[k] - 1u) / t[k];
  return n;
}

int launch_reach_seed(ReachResult &q, hipStream_t s, const uint32_t *dist, size_t n_seeds, uint32_t clear_d2, uint32_t flags)
{
  const ReachArgs a = reach_args(q, dist, clear_d2, flags);
  const size_t n = (size_t)q.box.e[0] * q.box.e[1] * q.box.e[2];
  q.timer.mark(0, s);
  WS_HIP(hipMemsetAsync(q.cost.p, 0xff, n * sizeof(uint32_t), s));
  WS_HIP(hipMemsetAsync(q.mark.p, 0, (size_t)a.grid.n_tiles * sizeof(uint32_t), s));
  WS_HIP(hipMemsetAsync(q.words.dev, 0, 4 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(reach_seed_kernel, dim3((unsigned)((n_seeds + REACH_WG - 1) / REACH_WG)), dim3(REACH_WG), 0, s, a, q.seeds.as<int32_t>(), (uint32_t)n_seeds);
  q.timer.mark(1, s);
  WS_HIP(hipGetLastError());
  return q.words.fetch(s, 4);
}

int launch_reach_round(ReachResult &q, hipStream_t s, const uint32_t *dist, uint32_t r, uint32_t active, uint32_t clear_d2, uint32_t flags)
{
  const ReachArgs a = reach_args(q, dist, clear_d2, flags);
  if (active == 0u || active > a.grid.n_tiles) // (a tile is listed once per round)
  {
    set_error("reach: a round's list holds more tiles than the box has");
    return WS_ERR_INVALID;
  }
  if (q.box.columns)
    hipLaunchKernelGGL((reach_round_kernel<REACH_CA, REACH_CB, REACH_CC>), dim3(active), dim3(REACH_WG), 0, s, a, r);
  else
    hipLaunchKernelGGL((reach_round_kernel<REACH_VA, REACH_VB, REACH_VC>), dim3(active), dim3(REACH_WG), 0, s, a, r);
  WS_HIP(hipGetLastError());
  return q.words.fetch(s, 4);
}

int launch_reach_count(ReachResult &q, hipStream_t s)
{
  const size_t n = (size_t)q.box.e[0] * q.box.e[1] * q.box.e[2];
  q.timer.mark(2, s);
  const unsigned blocks = (unsigned)std::min<size_t>((n + REACH_WG - 1) / REACH_WG, 4096);
  hipLaunchKernelGGL(reach_count_kernel, dim3(blocks), dim3(REACH_WG), 0, s, (const uint32_t *)q.cost.p, (uint32_t)n, q.words.dev + 1);
  q.timer.mark(3, s);
  WS_HIP(hipGetLastError());
  return q.words.fetch(s, 4);
}

int launch_reach_lookup(const ReachResult &q, hipStream_t s, const int32_t *pts_dev, size_t n, int32_t stride, uint32_t *out_dev)
{
  hipLaunchKernelGGL(reach_lookup_kernel, dim3((unsigned)((n + REACH_WG - 1) / REACH_WG)), dim3(REACH_WG), 0, s, q.box, (const uint32_t *)q.cost.p, pts_dev, (uint32_t)n,
                     (uint32_t)stride, out_dev);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

int launch_reach_paths(ReachResult &q, hipStream_t s, size_t g, uint32_t cap_steps)
{
  if (cap_steps) WS_HIP(hipMemsetAsync(q.steps.p, 0, g * (size_t)cap_steps * 16, s));
  hipLaunchKernelGGL(reach_paths_kernel, dim3((unsigned)g), dim3(64), 0, s, q.box, (const uint32_t *)q.cost.p, (const int32_t *)q.goals.p, cap_steps,
                     static_cast<uint4 *>(q.hdr.p), static_cast<int4 *>(q.steps.p));
  WS_HIP(hipGetLastError());
  return WS_OK;
}
} // namespace ws
