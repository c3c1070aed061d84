// reg_launches.hip — the registration routes that are one launch per iteration or per call (see reg_loop.hip for all routes):
// reg_iter_kernel, reg_pass_kernel with reg_solve_kernel, and the test entry of the wave solver.  Compiled as a part of reg_routes.hip, which says why.
#include "reg_exchange.h"

namespace ws
{
struct IterArgs
{
  PointArgs pts;
  GnState *state;     // [2], double buffered by launch parity
  int64_t *partials;  // [2][REG_BLOCKS][REG_SLOTS]
  int32_t k;          // launch index 0 .. max_iterations
  int32_t *host_flag; // host-mapped: set when the loop has finished (lets the host stop enqueueing)
};

// One launch == one Gauss-Newton iteration (see the header of this file).
__global__ __launch_bounds__(REG_THREADS) void reg_iter_kernel(IterArgs a)
{
  __shared__ int64_t wave_part[REG_THREADS / 64][REG_SLOTS];
  __shared__ int64_t red[REG_SLOTS];
  __shared__ float T_sh[16];
  __shared__ int stop_sh;

#ifdef WS_REG_TIMING
  long long ts[6];
  ts[0] = wall_clock64();
#define WS_STAMP(i) ts[i] = wall_clock64()
#else
#define WS_STAMP(i)
#endif
  const GnState *prev = &a.state[(a.k + 1) & 1];
  GnState *cur = &a.state[a.k & 1];
  const bool need_update = a.k > 0 && !prev->core.finished && prev->core.iterations < prev->core.max_iterations;
  // this lane's points do not depend on the transform: fetch them now, under phase A
  const Prefetched pref = prefetch_points(a.pts);

  if (need_update)
  {
    // phase A: total of the previous launch's partials (every workgroup, redundantly)
    WS_STAMP(1);
    sum_partials(a.partials + (size_t)((a.k + 1) & 1) * REG_SLOTS * REG_BLOCKS, wave_part, red);
  }
  WS_STAMP(2);
  if (threadIdx.x < 64)
  {
    // the whole first wave: the 6x6 solve is lane-parallel, everything else is computed identically by every lane
    GnCore st = prev->core;
    if (need_update)
    {
      gn_update_terms(st, red);
      if (blockIdx.x == 0 && threadIdx.x == 0)
      {
        int64_t sums[44];
        expand_sums(red, sums);
#pragma unroll
        for (int i = 0; i < 44; ++i) cur->sums[i] = sums[i];
      }
    }
    if (threadIdx.x == 0)
    {
      const int stop = (st.finished || st.iterations >= st.max_iterations) ? 1 : 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) T_sh[i] = st.T[i];
      stop_sh = stop;
      if (blockIdx.x == 0)
      {
        cur->core = st;
        // a launch enqueued behind the end of the loop carries the sums of the last update along with the state: the host
        // reads both from the buffer of the last launch (ws_debug_reg_sums)
        if (a.k > 0 && !need_update)
          for (int i = 0; i < 44; ++i) cur->sums[i] = prev->sums[i];
        if (stop && a.host_flag) __hip_atomic_store(a.host_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
  __syncthreads();
  WS_STAMP(3);
  if (stop_sh) return;

  // phase B
  float T[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) T[i] = T_sh[i];
  int64_t acc[REG_SLOTS];
#pragma unroll
  for (int t = 0; t < REG_SLOTS; ++t) acc[t] = 0;
  accumulate_points(a.pts, T, pref, acc);
  WS_STAMP(4);
  block_reduce32(acc, wave_part, red);
  if (threadIdx.x < REG_SLOTS)
    a.partials[(size_t)(a.k & 1) * REG_SLOTS * REG_BLOCKS + (size_t)blockIdx.x * REG_SLOTS + threadIdx.x] = red[threadIdx.x];
#ifdef WS_REG_TIMING
  WS_STAMP(5);
  if (blockIdx.x == 7 && threadIdx.x == 0 && a.k == 20)
    printf("reg_iter k=%d ticks(100MHz): load %lld reduce %lld solve %lld accumulate %lld reduce %lld\n", a.k, ts[1] - ts[0], ts[2] - ts[1],
           ts[3] - ts[2], ts[4] - ts[3], ts[5] - ts[4]);
#endif
}

// the solve alone, fed with externally (all-)reduced sums (multi-GPU path: partials -> 44 sums in HBM -> RCCL all-reduce -> solve)
__global__ __launch_bounds__(64) void reg_solve_kernel(GnState *state, const int64_t *sums_dev)
{
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  GnCore st;
  load_core(st, &state->core);
  __shared__ int64_t s[44];
  if (threadIdx.x < 44) s[threadIdx.x] = coherent_i64(&sums_dev[threadIdx.x]);
  __syncthreads();
  gn_update(
      st, [](int r, int c) { return s[c * 6 + r]; }, [](int r) { return s[36 + r]; }, (int32_t)s[42], (int32_t)s[43]);
  if (threadIdx.x == 0) store_state(state, st, s);
}

// ---- one launch per call: the multi-GPU path and perform_registration without the server ------------------------------
// [apply the Gauss-Newton update from the sums of the previous iteration] -> stop test -> accumulate the cloud (or this rank's
// shard) -> the 44 sums.  Every workgroup repeats the (cheap) update from the same sums, like the resident loop does, and the
// last workgroup to arrive (an arrival counter, agent-scope accesses: no cache-wide fences) adds the partials up AND writes the
// updated state.  The routes:
//   ws_reg_iterate_shard_dev (apply as asked) and ws_reg_accumulate_dev (apply = 0): the multi-GPU path, sums all-reduced
//     between two launches;
//   ws_reg_iterate without the resident server: tsdf_registration.cpp:55-92 calls perform_registration once per iteration and
//     needs h, g, e, c on the host before it can go on.  The pose travels in the kernel arguments (no state), and the last
//     workgroup writes the 44 sums and, behind them, the call's sequence number into host-mapped memory, where the host spins.
// ONE state buffer, read by every workgroup before it arrives and written by the last one after all have arrived: the launch
// bakes in no buffer parity, so a batch of these launches captured into a HIP graph replays from whatever state the buffer holds
// (a host-side parity flip per launch made every replay restart from a stale buffer).  A launch after the loop is
// over changes neither the state nor the sums.  (ws_register_cloud's one launch per iteration stays with reg_iter_kernel: its
// partials are summed at the head of the next launch by every workgroup at once, where this kernel's last arriver adds an
// arrival round trip and a pass over the partials to every iteration -- 15.4 instead of 10.3 us per iteration, measured.)
// POSE (ws_reg_iterate): the pose comes in the arguments, there is no state and no update, and the sums go to host-mapped
// memory followed by the sequence number.  Two argument layouts, so the state route carries no pose.
template <bool POSE>
struct PassArgs
{
  PointArgs pts;      // first / end: this rank's shard
  GnState *state;     // in: the state before this launch; out (if apply): the state after the update
  int64_t *sums;      // in: the all-reduced sums of the previous iteration (if apply); out: this rank's 44 sums
  int64_t *partials;  // [REG_BLOCKS][REG_SLOTS]
  uint32_t *arrived;  // zero between launches
  int32_t apply;
};
template <>
struct PassArgs<true>
{
  PointArgs pts;
  float T[16];        // column-major
  int64_t *partials;  // [REG_BLOCKS][REG_SLOTS]
  uint32_t *arrived;  // zero between launches
  int64_t *sums;      // host-mapped: 44 sums, then (at [44]) the sequence number
  uint32_t seq;
};
static_assert(sizeof(PassArgs<false>) <= 256 && sizeof(PassArgs<true>) <= 256, "reg_pass_kernel: more than 256 bytes of kernel arguments (see LoopArgs)");

template <bool POSE>
__global__ __launch_bounds__(REG_THREADS) void reg_pass_kernel(PassArgs<POSE> a)
{
  __shared__ int64_t wave_part[REG_THREADS / 64][REG_SLOTS];
  __shared__ int64_t red[REG_SLOTS];
  __shared__ int64_t s44[44];
  __shared__ float T_sh[16];
  __shared__ int stop_sh, last_sh;
  const Prefetched pref = prefetch_points(a.pts);
  GnCore st; // first wave only, identical in all of its lanes
  if constexpr (!POSE)
  {
    if (threadIdx.x < 64)
    {
      load_core(st, &a.state->core);
      if (a.apply)
      {
        if (threadIdx.x < 44) s44[threadIdx.x] = coherent_i64(&a.sums[threadIdx.x]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // LDS written and read by this wave only
        __builtin_amdgcn_wave_barrier();
        gn_update(
            st, [&](int r, int c) { return s44[c * 6 + r]; }, [&](int r) { return s44[36 + r]; }, (int32_t)s44[42], (int32_t)s44[43]);
      }
      if (threadIdx.x == 0)
      {
#pragma unroll
        for (int i = 0; i < 16; ++i) T_sh[i] = st.T[i];
        stop_sh = (st.finished || st.iterations >= st.max_iterations) ? 1 : 0;
      }
    }
    __syncthreads();
  }
  const bool stop = !POSE && stop_sh != 0; // every workgroup alike
  if (!stop)
  {
    float T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
      if constexpr (POSE)
        T[i] = a.T[i];
      else
        T[i] = T_sh[i];
    }
    int64_t acc[REG_SLOTS];
#pragma unroll
    for (int t = 0; t < REG_SLOTS; ++t) acc[t] = 0;
    accumulate_points(a.pts, T, pref, acc);
    block_reduce32(acc, wave_part, red);
    if (threadIdx.x < REG_SLOTS) publish_i64(&a.partials[(size_t)blockIdx.x * REG_SLOTS + threadIdx.x], red[threadIdx.x]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the write-through stores above have been acknowledged ...
  }
  else if constexpr (!POSE)
  {
    if (!a.apply) return; // the loop was over before this launch: nothing to update, nothing to add (the sums stay as they are)
  }
  __syncthreads(); // ... for all 32 lanes that made them
  if (threadIdx.x == 0)
    last_sh = __hip_atomic_fetch_add(a.arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
  __syncthreads();
  if (!last_sh) return;
  // everybody has read the state and the all-reduced sums: both may change now
  if constexpr (!POSE)
  {
    if (a.apply && threadIdx.x == 0) store_state(a.state, st, s44);
  }
  if (!stop)
  {
    sum_partials<true>(a.partials, wave_part, red);
    if (threadIdx.x == 0)
    {
      int64_t sums[44];
      expand_sums(red, sums);
#pragma unroll
      for (int k = 0; k < 44; ++k)
      {
        if constexpr (POSE)
          __hip_atomic_store(&a.sums[k], sums[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else
          publish_i64(&a.sums[k], sums[k]);
      }
    }
  }
  if (threadIdx.x == 0)
  {
    __hip_atomic_store(a.arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (POSE) __hip_atomic_store(&a.sums[44], (int64_t)a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// test entry: the wave solver alone, one wave per system (A row-major 6x6, b) -> x, status
__global__ __launch_bounds__(64) void solve6_test_kernel(const double *A, const double *b, double *x, int32_t *status)
{
  const int lane = threadIdx.x, r = lane >> 3, c = lane & 7;
  const double *Ai = A + (size_t)blockIdx.x * 36, *bi = b + (size_t)blockIdx.x * 6;
  double a = 0.0;
  if (r < 6 && c < 6) a = Ai[r * 6 + c];
  if (r < 6 && c == 6) a = bi[r];
  double xi[6] = {0, 0, 0, 0, 0, 0};
  const int rc = solve6_wave(a, xi);
  if (lane == 0)
  {
    status[blockIdx.x] = rc;
    for (int k = 0; k < 6; ++k) x[(size_t)blockIdx.x * 6 + k] = xi[k];
  }
}

int launch_solve6_test(ws_context *ctx, const double *A_dev, const double *b_dev, size_t n, double *x_dev, int32_t *status_dev)
{
  if (n == 0) return WS_OK;
  hipLaunchKernelGGL(solve6_test_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, A_dev, b_dev, x_dev, status_dev);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

int launch_reg_solve(ws_reg *r, const int64_t *sums_dev)
{
  hipLaunchKernelGGL(reg_solve_kernel, dim3(1), dim3(64), 0, r->ctx->stream, &r->state.as<GnState>()[r->latest], sums_dev);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

int launch_reg_pass(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t first, size_t count, int64_t *sums, int apply,
                    const float *T, uint32_t seq)
{
  ws_context *ctx = r->ctx;
  prof_begin(ctx, WS_K_REG);
  if (T)
  {
    PassArgs<true> a;
    a.pts = make_point_args(r, m, res, flags, first, count);
    for (int i = 0; i < 16; ++i) a.T[i] = T[i];
    a.partials = r->partials.as<int64_t>();
    a.arrived = r->pass_arrived.as<uint32_t>();
    a.sums = sums;
    a.seq = seq;
    hipLaunchKernelGGL(reg_pass_kernel<true>, dim3(REG_BLOCKS), dim3(REG_THREADS), 0, ctx->stream, a);
  }
  else
  {
    PassArgs<false> a;
    a.pts = make_point_args(r, m, res, flags, first, count);
    a.state = &r->state.as<GnState>()[r->latest]; // one buffer, no parity: see reg_pass_kernel
    a.sums = sums;
    a.partials = r->partials.as<int64_t>();
    a.arrived = r->pass_arrived.as<uint32_t>();
    a.apply = apply ? 1 : 0;
    hipLaunchKernelGGL(reg_pass_kernel<false>, dim3(REG_BLOCKS), dim3(REG_THREADS), 0, ctx->stream, a);
  }
  prof_end(ctx, WS_K_REG);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

int launch_reg_iteration(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, int32_t k)
{
  ws_context *ctx = r->ctx;
  IterArgs a;
  a.pts = make_point_args(r, m, res, flags, 0, r->n);
  a.state = r->state.as<GnState>();
  a.partials = r->partials.as<int64_t>();
  a.k = k;
  a.host_flag = r->host_flag.dev_as<int32_t>();
  prof_begin(ctx, WS_K_REG);
  hipLaunchKernelGGL(reg_iter_kernel, dim3(REG_BLOCKS), dim3(REG_THREADS), 0, ctx->stream, a);
  prof_end(ctx, WS_K_REG);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

size_t reg_partials_bytes() { return sizeof(int64_t) * 2 * REG_SLOTS * REG_BLOCKS; }

} // namespace ws
