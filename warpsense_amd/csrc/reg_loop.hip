// reg_loop.hip — Point-to-TSDF registration for MI355X (gfx950): the routes, and the resident loop.
//
// Replaces calc_jacobis_krnl + h_g_e_reduction_krnl + the host reduce() of the reference
// (src/warpsense/cuda/registration.cu:14-257,310-368) and moves the Gauss-Newton update of
// cuda::TSDFRegistration::register_cloud (src/warpsense/tsdf_registration.cpp:55-92) onto the device.
//
// One Gauss-Newton iteration, in every workgroup (256 x 512 lanes):
//   phase A  (k > 0) total of the previous iteration's partial sums (exact integer sums -> order independent,
//            bit-identical to the reference's tree); the first wave runs the 6x6 solve (lane-parallel LU in
//            double), xi -> SE(3) and the convergence test exactly like the reference's host code.  Doing this
//            redundantly per workgroup costs nothing extra and saves a broadcast.
//   phase B  fixed-point transform, voxel + 6-neighbour gather, gradient, Jacobian, per-lane accumulation
//            of the 21 unique terms of J J^T, the 6 of J v, |v| and the count in int64 registers
//            (v_mad_i64_i32), a transposing wave64 reduction (32 values in 32 exchanges instead of 32 x 6),
//            LDS across the waves, one 29-word partial per workgroup.
// No Jacobian / value / mask arrays ever reach HBM (the reference writes and re-reads 51 B per point).
//
// The device code lies in four layers, each a header that includes the ones before it: reg_reduce.h (the exact integer sums),
// reg_gn.h (the Gauss-Newton update), reg_points.h (a lane's points and the sums over them), reg_exchange.h (the counted
// exchange, agent-scope hand-over between kernels).  Five routes are built from them, one file per kind of launch:
// reg_loop_kernel (default; this file) runs ALL iterations in one launch: resident workgroups, partial sums exchanged through
// wrapping group accumulators whose words count their additions (the exchange is the barrier), a per-lane voxel cache.
// reg_iter_kernel (reg_launches.hip) is one launch per iteration (state and 256 x 32 partials double buffered by launch parity: what
// one launch writes only the next one reads, so it needs no fences or atomics); it is the fallback when the grid cannot be
// resident, and the A/B reference.
// reg_pass_kernel (reg_launches.hip) is one launch per call of the multi-GPU path and of perform_registration without the resident
// server.  Unlike reg_iter_kernel it hands results over INSIDE a launch and through ONE state buffer: the partials go to the last
// workgroup to arrive (an arrival counter), the state and the sums to the next launch or graph node, all of it written and read
// at agent scope (reg_exchange.h); reg_solve_kernel is its update alone, fed with all-reduced sums.
// reg_server_kernel (reg_server.hip) is perform_registration WITHOUT a launch per call: it stays on the GPU across the calls of
// ws_reg_iterate, takes pose and request number from a line of host-mapped memory and answers with the 44 sums.
// reg_batch_kernel (reg_batch.hip) is K registrations of one cloud in one launch, a workgroup per start pose
// (ws_register_cloud_batch): nothing is exchanged between workgroups.
// This file, reg_launches.hip and reg_server.hip are compiled as ONE unit, reg_routes.hip, which says why.
#include <cstdlib>
#include <cstring>

#include "reg_exchange.h"

namespace ws
{
// ---- the whole Gauss-Newton loop in ONE launch -------------------------------------------------------
// The launch boundary between two iterations above costs ~5.5 us (dispatch of 256 workgroups, end-of-kernel
// cache write-back, the gap to the next launch) for ~10 us of work.  reg_loop_kernel keeps the 256
// workgroups resident (one per CU, checked on the host before the launch) and replaces the boundary by a
// grid-wide exchange of the partial sums that is its own barrier (reg_exchange.h).  The
// per-iteration structure (and every arithmetic step) is the one of reg_iter_kernel; the points of a
// lane stay in registers for the whole loop.
struct LoopArgs
{
  PointArgs pts;
  GnCore init;       // the state the loop starts from (by value: no staging copy, no host synchronisation before the launch)
  GnState *state;    // out: state[0] (device copy for ws_reg_poll)
  GnState *result_host; // out: the same in host-mapped memory (the host only waits for the stream, no copy back)
  uint64_t *accum;   // [2][REG_GROUPS][REG_WORDS] counted group accumulators, zeroed before the launch; the abort flag (zeroed too)
                     // sits REG_ACCUM_OFFSET bytes in front of them (its own pointer would be the 257th byte of arguments)
  PeerBlock *peers;  // multi-GPU loop only
  uint32_t *clear_next; // the set of the NEXT launch (abort flag + accumulators): cleared on the way out
  uint32_t clear_words;
  int32_t debug_stall;  // test hook (ws_debug_reg_stall): workgroup 0 keeps its first contribution to itself.  Sits in the padding
                        // behind clear_words on purpose: 8 more bytes of kernel arguments made this kernel 30 % slower (1.07 -> 1.39 ms)
  int32_t *host_flag;
};
// Measured on MI355X / ROCm 7.0 (tools/reg_fit.py): with 264 bytes of kernel arguments instead of 256 an iteration of this
// kernel takes 7.86 us instead of 6.03 us -- same instructions, and 192 bytes are no faster than 256.  Keep them within 256.
static_assert(sizeof(LoopArgs) <= 256, "reg_loop_kernel: more than 256 bytes of kernel arguments");

constexpr size_t REG_ACCUM_OFFSET = 256; // accumulators behind the abort flag

// PEERS: this rank's shard of the points, a grid of any multiple of REG_GROUPS workgroups (ranks that share one GPU in the
// tests split the chip), and the cross-GPU exchange behind the on-chip one
// MFMA: the cloud (shard) has at most one point per lane -- every real scan: the reference's RegistrationCuda holds 131 072
// points -- and the sums come from the matrix cores (mfma_consume above)
template <bool PEERS, bool MFMA>
__global__ __launch_bounds__(REG_THREADS) void reg_loop_kernel(LoopArgs a)
{
  const uint32_t n_blocks = PEERS ? gridDim.x : (uint32_t)REG_BLOCKS, stride = n_blocks * REG_THREADS, per_group = n_blocks / REG_GROUPS;
  uint32_t *const abort_flag = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(a.accum) - REG_ACCUM_OFFSET);
  __shared__ unsigned long long wg_sum[REG_SLOTS + MF_AUX]; // the workgroup's totals of an iteration (LDS atomics of the eight waves)
  __shared__ alignas(16) uint32_t mf_stage[MFMA ? (REG_THREADS / 64) * MF_STAGE_WORDS : 4];
  const MfLane mfl = make_mf_lane();
  __shared__ int64_t red[REG_SLOTS];
  __shared__ alignas(16) float T_sh[16];
  __shared__ alignas(16) int32_t TI_sh[16];
  __shared__ int stop_sh;

  const Prefetched pref = prefetch_points(a.pts, stride);
  const bool wave_has_points = __ballot(pref.valid[0]) != 0ull; // later passes of the grid only have points where the first has
  const LoopGather lg = make_loop_gather(a.pts);
  GnCore st; // first wave only, identical in all of its lanes
  if (threadIdx.x < 64) st = a.init;
  uint64_t mb_then0 = 0, mb_then1 = 0; // first wave, PEERS: this lane's mailbox words of both parities when last complete
  uint32_t mb_base = 0;                // exchanges before this launch
  if (PEERS && threadIdx.x < 64)
  {
    mb_then0 = a.peers->then[0][threadIdx.x];
    mb_then1 = a.peers->then[1][threadIdx.x];
    mb_base = a.peers->exchanges;
  }
  // The loop state is uniform, so the compiler would keep it in scalar registers -- on top of the ~50 the kernel arguments
  // occupy, i.e. spilled to vector lanes and reloaded (v_readlane) in the middle of the first wave's dependency chain,
  // and everything the vector unit computes from it (all of it is float arithmetic) would cross between the two register
  // files.  Pinned to vector registers here it simply stays where it is used.
  pin_vgpr(st.center[0]); pin_vgpr(st.center[1]); pin_vgpr(st.center[2]);
  pin_vgpr(st.alpha); pin_vgpr(st.it_weight_gradient); pin_vgpr(st.epsilon);
  pin_vgpr(st.prev[0]); pin_vgpr(st.prev[1]); pin_vgpr(st.prev[2]); pin_vgpr(st.prev[3]);
  pin_vgpr(st.max_iterations); pin_vgpr(st.iterations); pin_vgpr(st.finished); pin_vgpr(st.error);
  uint64_t then_cur[REG_GROUPS], then_other[REG_GROUPS]; // first wave: the accumulator words of both parities when last complete
#pragma unroll
  for (int g = 0; g < REG_GROUPS; ++g) then_cur[g] = then_other[g] = 0;
  VoxelCache cache[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
  {
    cache[u].bx = cache[u].by = cache[u].bz = 0;
    cache[u].cur = cache[u].xn = cache[u].xl = cache[u].yn = cache[u].yl = cache[u].zn = cache[u].zl = 0;
    cache[u].filled = false;
  }
#ifdef WS_REG_TIMING
  long long ts[7], tot[6] = {0, 0, 0, 0, 0, 0}, miss_ticks = 0, hit_ticks = 0;
  int miss_its = 0, miss_lanes = 0;
#define WS_LSTAMP(i) ts[i] = wall_clock64()
#else
#define WS_LSTAMP(i)
#endif
  float Tel = 0.f; // first wave, lanes 0 .. 15: the pose element (lane & 3, lane >> 2)
#pragma unroll
  for (int i = 0; i < 16; ++i) Tel = (int)threadIdx.x == i ? a.init.T[i] : Tel; // (a dynamic index into the arguments costs a scratch copy)
  if (threadIdx.x < 16)
  {
    T_sh[threadIdx.x] = Tel;
    store_int_pose(TI_sh, (int)threadIdx.x, Tel);
  }
  if (threadIdx.x < REG_SLOTS + MF_AUX) wg_sum[threadIdx.x] = 0;
  uint32_t k = 0;
  for (;; ++k)
  {
    WS_LSTAMP(0);
    WS_LSTAMP(1);
    WS_LSTAMP(2);
    if (threadIdx.x < 64)
    {
      if (k > 0)
      {
        // totals of iteration k - 1 (parity (k + 1) & 1) straight from the counted accumulators: this IS the grid barrier
        int64_t total = 0;
        bool ok = counted_collect(a.accum + (size_t)((k + 1) & 1) * REG_GROUPS * REG_WORDS, abort_flag, then_cur, then_other, red, per_group, &total);
        if (PEERS && ok) // the ranks' totals -> everybody's mailbox -> the totals over all ranks, in red[]
          ok = ((mb_base + k - 1) & 1) ? peer_exchange(a.peers, 1, mb_then1, total, red, abort_flag) : peer_exchange(a.peers, 0, mb_then0, total, red, abort_flag);
        WS_LSTAMP(2);
        if (!ok)
        {
          st.finished = 1;
          st.error = 1; // reported by the host
        }
        else
          gn_update_total(st, total, Tel, T_sh, TI_sh); // (red[] is only read again at the very end)
      }
      if (threadIdx.x == 0) stop_sh = (st.finished || st.iterations >= st.max_iterations) ? 1 : 0;
    }
    __syncthreads();
    WS_LSTAMP(3);
    if (stop_sh) break;

#ifdef WS_REG_TIMING
    const int32_t obx = cache[0].bx, oby = cache[0].by, obz = cache[0].bz;
    const bool ofilled = cache[0].filled;
#endif
    if (wave_has_points) // (uniform per wave; point_slot(): a small cloud or shard leaves whole waves of every workgroup without points)
      pass_sums<MFMA>(a.pts, lg, pref, stride, T_sh, TI_sh, cache, mf_stage, mfl, wg_sum, [&] { WS_LSTAMP(4); });
    __syncthreads();
    WS_LSTAMP(5);
    if (threadIdx.x < 64)
      counted_publish<MFMA>(a.accum + (size_t)(k & 1) * REG_GROUPS * REG_WORDS, wg_sum, !(a.debug_stall && blockIdx.x == 0 && k == 0), per_group, &mfl);
#ifdef WS_REG_TIMING
    WS_LSTAMP(6);
    for (int i = 0; i < 6; ++i) tot[i] += ts[i + 1] - ts[i];
#endif
#ifdef WS_REG_TIMING
    { // (after the stamps of the phases: the vote below costs a barrier)
      const bool changed = ofilled && cache[0].filled && (obx != cache[0].bx || oby != cache[0].by || obz != cache[0].bz);
      const int n_changed = __syncthreads_count(changed ? 1 : 0);
      if (n_changed > 0)
      {
        miss_its += 1;
        miss_ticks += ts[4] - ts[3];
        miss_lanes += n_changed;
      }
      else
        hit_ticks += ts[4] - ts[3];
    }
#endif
  }
#ifdef WS_REG_TIMING_GN
  if (blockIdx.x == 0 && threadIdx.x == 0)
    printf("gn_update x%lld, 10ns ticks: build %lld solve6 %lld xi_to_transform %lld pose+err %lld\n", g_gn_ticks[4], g_gn_ticks[0], g_gn_ticks[1],
           g_gn_ticks[2], g_gn_ticks[3]);
#endif
#ifdef WS_REG_TIMING
  if ((blockIdx.x % 37) == 0 && threadIdx.x == 0)
    printf("reg_loop wg %d iterations %u, 10ns ticks per phase: wait %lld sum %lld solve %lld accumulate %lld reduce %lld arrive %lld\n", (int)blockIdx.x, k,
           tot[0], tot[1], tot[2], tot[3], tot[4], tot[5]);
  if ((blockIdx.x % 37) == 0 && threadIdx.x == 0)
    printf("  wg %d: iterations with a moved point %d (%d lanes), accumulate ticks in those %lld, in the others %lld\n", (int)blockIdx.x, miss_its, miss_lanes,
           miss_ticks, hit_ticks);
#endif
  if (blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < a.clear_words; i += REG_THREADS) a.clear_next[i] = 0u; // nobody touches that set during this launch
  if (PEERS && blockIdx.x == 0 && threadIdx.x < 64 && !st.error)
  {
    a.peers->then[0][threadIdx.x] = mb_then0; // where the next launch starts counting
    a.peers->then[1][threadIdx.x] = mb_then1;
    if (threadIdx.x == 0) a.peers->exchanges = mb_base + k; // k exchanges in this launch (the same number on every rank)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
#pragma unroll
    for (int i = 0; i < 16; ++i) st.T[i] = T_sh[i];
    a.state[0].core = st;
    a.result_host->core = st;
    if (k > 0 && !st.error)
    {
      int64_t sums[44];
      expand_sums(red, sums); // the totals the last update was made from
#pragma unroll
      for (int i = 0; i < 44; ++i) a.state[0].sums[i] = sums[i]; // (the host copy carries the state only: 44 fewer writes over PCIe)
    }
    // release: the result above is visible to the host before the flag (ws_register_cloud spins on the flag instead of
    // sleeping in hipStreamSynchronize)
    if (a.host_flag) __hip_atomic_store(a.host_flag, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// 1 if the device can hold the whole grid of reg_loop_kernel at once (required by its grid barrier)
int reg_loop_supported(int device)
{
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reg_loop_kernel<false, true>, REG_THREADS, 0) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
  return (long long)per_cu * cus >= REG_BLOCKS ? 1 : 0;
}

// Two sets of {abort flag, counted accumulators}, used by alternate launches: a launch finds its set zero because the
// launch before it cleared it on its way out (block 0, after its own loop) -- no memset kernel in front of every launch.
constexpr size_t REG_ACCUM_BYTES = sizeof(uint64_t) * 2 * REG_GROUPS * REG_WORDS;
constexpr size_t REG_SET_BYTES = REG_ACCUM_OFFSET + REG_ACCUM_BYTES;

int launch_reg_loop(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, const GnCore &init, bool peers, size_t first, size_t count)
{
  ws_context *ctx = r->ctx;
  LoopArgs a;
  a.pts = make_point_args(r, m, res, flags, peers ? first : 0, peers ? count : r->n);
  a.init = init;
  a.state = r->state.as<GnState>();
  a.result_host = r->result_host.dev_as<GnState>();
  if (!r->loop_sets_clear)
  {
    WS_HIP(hipMemsetAsync(r->grid_bar.p, 0, 2 * REG_SET_BYTES, ctx->stream));
    r->loop_sets_clear = true;
  }
  char *mine = r->grid_bar.as<char>() + (r->loop_launches & 1u) * REG_SET_BYTES;
  char *other = r->grid_bar.as<char>() + ((r->loop_launches + 1) & 1u) * REG_SET_BYTES;
  r->loop_launches += 1;
  a.accum = reinterpret_cast<uint64_t *>(mine + REG_ACCUM_OFFSET); // (the abort flag is the first word of the set)
  a.peers = r->peer_block_dev.as<PeerBlock>();
  a.clear_next = reinterpret_cast<uint32_t *>(other);
  a.clear_words = (uint32_t)(REG_SET_BYTES / sizeof(uint32_t));
  a.host_flag = r->host_flag.dev_as<int32_t>();
  a.debug_stall = r->debug_stall_next;
  r->debug_stall_next = 0;
  prof_begin(ctx, WS_K_REG);
  const unsigned blocks = peers ? (unsigned)r->peer_blocks : (unsigned)REG_BLOCKS;
  // at most one point per lane (every scan the reference's 131 072-point buffers can hold): the sums come from the matrix cores
  const bool mfma = WS_REG_MFMA && (size_t)(a.pts.end - a.pts.first) <= (size_t)blocks * REG_THREADS;
  if (peers)
  {
    if (mfma)
      hipLaunchKernelGGL((reg_loop_kernel<true, true>), dim3(blocks), dim3(REG_THREADS), 0, ctx->stream, a);
    else
      hipLaunchKernelGGL((reg_loop_kernel<true, false>), dim3(blocks), dim3(REG_THREADS), 0, ctx->stream, a);
  }
  else
  {
    if (mfma)
      hipLaunchKernelGGL((reg_loop_kernel<false, true>), dim3(blocks), dim3(REG_THREADS), 0, ctx->stream, a);
    else
      hipLaunchKernelGGL((reg_loop_kernel<false, false>), dim3(blocks), dim3(REG_THREADS), 0, ctx->stream, a);
  }
  prof_end(ctx, WS_K_REG);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

// host image of PeerBlock (api_reg.hip fills it: the mailbox pointers are peer-mapped or local device addresses)
size_t reg_peer_block_bytes() { return sizeof(PeerBlock); }
void reg_peer_block_fill(void *host_image, void *const mailbox[8], int rank, int world)
{
  PeerBlock *pb = reinterpret_cast<PeerBlock *>(host_image);
  std::memset(pb, 0, sizeof(PeerBlock));
  for (int i = 0; i < 8; ++i) pb->mailbox[i] = reinterpret_cast<uint64_t *>(i < world ? mailbox[i] : nullptr);
  pb->rank = rank;
  pb->world = world;
  long long ticks = REG_PEER_TIMEOUT_TICKS;
  if (const char *ms = std::getenv("WS_REG_PEER_TIMEOUT_MS"))
  {
    const long long v = std::atoll(ms);
    if (v >= 1 && v <= 20000) ticks = v * 100000ll;
  }
  pb->timeout_ticks = (int32_t)ticks;
}
size_t reg_mailbox_bytes() { return sizeof(uint64_t) * 2 * REG_WORDS; }
int reg_groups() { return REG_GROUPS; }
int reg_default_blocks() { return REG_BLOCKS; }

size_t reg_barrier_bytes() { return 2 * REG_SET_BYTES; }

} // namespace ws
