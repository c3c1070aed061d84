// reg_batch.hip — many start poses in one launch, a workgroup per pose (see reg_loop.hip for all routes): the host's records,
// the kernel and its launcher.
#include <cstring>

#include "reg_points.h"

namespace ws
{
#ifndef WS_REG_BATCH_VARIANT
#define WS_REG_BATCH_VARIANT 1 // reg_batch_kernel: 1: the first two points of every lane stay in registers with a voxel cache (16 384 points, K = 256: 22.7 ms against 24.3 ms with every point streamed; 131 072 points: no difference)
#endif

// ---- K registrations of one cloud in ONE launch: a workgroup per start pose (ws_register_cloud_batch) -----------------
// Re-localisation, a doubtful pre-transform, a pose lattice: K independent Gauss-Newton loops over the same cloud and map.
// One loop alone leaves the chip waiting on a single wave's solve and on the grid-wide exchange; K of them side by side fill
// those bubbles, and with a whole hypothesis inside ONE workgroup there is nothing left to exchange: workgroup k strides over
// all points, reduces its 29 terms through LDS, its first wave runs the update the other loops run (gn_update_terms) and hands
// the pose back through LDS.  No word of memory is shared between workgroups, nothing spins, nothing has to be co-resident:
// every loop below is bounded by max_iterations or the point count, and K may exceed the number of compute units.
// The sums are exact integers (order independent) and the update is the same code on the same values, so hypothesis k ends
// bit for bit where ws_register_cloud ends from the same start pose.  The pass that finds the loop over (converged,
// max_iterations, no correspondences, singular system) has just accumulated at the FINAL pose: its e and c are the score.
struct BatchIn // one per hypothesis, written by the host (host-mapped memory)
{
  float T[16];       // start pose, column-major
  int32_t center[3]; // gn_init's (int) translation, converted on the host like the single route's
  int32_t pad;
};
struct BatchOut
{
  float T[16];
  int32_t iterations, e, c, pad;
};
static_assert(sizeof(BatchIn) == 80 && sizeof(BatchOut) == 80, "batch records");
size_t reg_batch_record_bytes() { return sizeof(BatchIn) + sizeof(BatchOut); }
void reg_batch_write(void *records, size_t k, const float T[16])
{
  BatchIn *in = static_cast<BatchIn *>(records) + k;
  std::memcpy(in->T, T, sizeof in->T);
  for (int i = 0; i < 3; ++i) in->center[i] = (int32_t)T[12 + i];
  in->pad = 0;
}
void reg_batch_read(const void *records, size_t n, size_t k, float T[16], int32_t *iterations, int32_t *e, int32_t *c)
{
  const BatchOut *out = reinterpret_cast<const BatchOut *>(static_cast<const BatchIn *>(records) + n) + k;
  std::memcpy(T, out->T, sizeof out->T);
  if (iterations) *iterations = out->iterations;
  if (e) *e = out->e;
  if (c) *c = out->c;
}

struct BatchArgs
{
  PointArgs pts;
  const BatchIn *in; // [gridDim.x]
  BatchOut *out;     // [gridDim.x]
  int32_t max_iterations;
  float it_weight_gradient, epsilon;
};

constexpr int BATCH_UNROLL = 4; // points of a lane whose gathers are in flight together (4 x 7 loads before the first is consumed)

// THREADS: lanes of the workgroup.  NCACHE: the first NCACHE points of every lane stay in registers for the whole loop together
// with the voxel they fell into and its seven entries (gather_point<true>); the others are streamed from memory every iteration.
template <int THREADS, int NCACHE>
__global__ __launch_bounds__(THREADS) void reg_batch_kernel(BatchArgs a)
{
  constexpr int WAVES = THREADS / 64;
  __shared__ int64_t wave_part[WAVES][REG_SLOTS];
  __shared__ int64_t red[REG_SLOTS];
  __shared__ alignas(16) float T_sh[16];
  __shared__ alignas(16) int32_t TI_sh[16];
  __shared__ int stop_sh;
  const BatchIn *in = a.in + blockIdx.x;
  const int lane = threadIdx.x & 63;

  GnCore st; // first wave only, identical in all of its lanes: gn_init of the single route
#pragma unroll
  for (int i = 0; i < 16; ++i) st.T[i] = 0.f;
  st.center[0] = st.center[1] = st.center[2] = 0;
  if (threadIdx.x < 64)
  {
#pragma unroll
    for (int i = 0; i < 16; ++i) st.T[i] = in->T[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) st.center[i] = in->center[i];
  }
  st.alpha = 0.f;
  st.prev[0] = st.prev[1] = st.prev[2] = st.prev[3] = 0.f;
  st.it_weight_gradient = a.it_weight_gradient;
  st.epsilon = a.epsilon;
  st.max_iterations = a.max_iterations;
  st.iterations = 0;
  st.finished = 0;
  st.error = 0;
  if (threadIdx.x < 16)
  {
    const float v = in->T[threadIdx.x];
    T_sh[threadIdx.x] = v;
    if (threadIdx.x == 15) TI_sh[15] = 0; // (read by load_int_pose, used by nobody)
    store_int_pose(TI_sh, (int)threadIdx.x, v);
  }

  // the points that stay in registers
  constexpr int NC = NCACHE > 0 ? NCACHE : 1;
  int32_t cp[NC][3];
  bool cvalid[NC];
  VoxelCache cache[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u)
  {
    const uint32_t off = (uint32_t)(u * THREADS) + threadIdx.x;
    cvalid[u] = NCACHE > 0 && off < a.pts.end - a.pts.first; // (first <= end: make_point_args)
    const size_t o = cvalid[u] ? 3 * ((size_t)a.pts.first + off) : 0;
    cp[u][0] = cvalid[u] ? a.pts.points[o + 0] : 0;
    cp[u][1] = cvalid[u] ? a.pts.points[o + 1] : 0;
    cp[u][2] = cvalid[u] ? a.pts.points[o + 2] : 0;
    cache[u].bx = cache[u].by = cache[u].bz = 0;
    cache[u].cur = cache[u].xn = cache[u].xl = cache[u].yn = cache[u].yl = cache[u].zn = cache[u].zl = 0;
    cache[u].filled = false;
  }
  __syncthreads();

  for (;;) // at most max_iterations + 1 passes: every pass that does not stop adds one to st.iterations (gn_step)
  {
    const IntTransform t = load_int_pose(TI_sh);
    int64_t acc[REG_SLOTS];
#pragma unroll
    for (int s = 0; s < REG_SLOTS; ++s) acc[s] = 0;
    if constexpr (NCACHE > 0)
    {
      Gathered g[NC];
#pragma unroll
      for (int u = 0; u < NC; ++u) g[u] = gather_point<true>(a.pts, t, cp[u][0], cp[u][1], cp[u][2], cvalid[u], &cache[u]);
#pragma unroll
      for (int u = 0; u < NC; ++u) consume_point(g[u], acc);
    }
    // the streamed points: lane l takes first + NCACHE * THREADS + l, then every THREADS-th
    const uint32_t n_pts = a.pts.end - a.pts.first;
    for (uint32_t base = (uint32_t)(NCACHE * THREADS) + threadIdx.x; base < n_pts; base += (uint32_t)(BATCH_UNROLL * THREADS))
    {
      Gathered g[BATCH_UNROLL];
#pragma unroll
      for (int u = 0; u < BATCH_UNROLL; ++u)
      {
        const bool valid = (uint32_t)(u * THREADS) < n_pts - base;
        const size_t o = valid ? 3 * ((size_t)a.pts.first + base + (uint32_t)(u * THREADS)) : 0;
        const int32_t px = valid ? a.pts.points[o + 0] : 0, py = valid ? a.pts.points[o + 1] : 0, pz = valid ? a.pts.points[o + 2] : 0;
        g[u] = gather_point(a.pts, t, px, py, pz, valid);
      }
#pragma unroll
      for (int u = 0; u < BATCH_UNROLL; ++u) consume_point(g[u], acc);
    }
    block_reduce32<WAVES>(acc, wave_part, red);
    if (threadIdx.x < 64)
    {
      const bool stop = st.finished || st.iterations >= st.max_iterations; // (uniform)
      if (!stop)
      {
        gn_update_terms(st, red);
        float Tel = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) Tel = lane == i ? st.T[i] : Tel; // (a dynamic index would be a scratch copy)
        if (lane < 16)
        {
          T_sh[lane] = Tel;
          store_int_pose(TI_sh, lane, Tel);
        }
      }
      else if (threadIdx.x == 0)
      {
        BatchOut *out = a.out + blockIdx.x;
#pragma unroll
        for (int i = 0; i < 16; ++i) out->T[i] = st.T[i];
        out->iterations = st.iterations;
        out->e = (int32_t)red[word_slot(42)]; // the reference's `int` words, at the final pose
        out->c = (int32_t)red[word_slot(43)];
        out->pad = 0;
      }
      if (threadIdx.x == 0) stop_sh = stop ? 1 : 0;
    }
    __syncthreads();
    if (stop_sh) break;
  }
}

int reg_batch_default_variant() { return WS_REG_BATCH_VARIANT; }

int launch_reg_batch(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t k, int32_t max_iterations, float it_weight_gradient, float epsilon)
{
  ws_context *ctx = r->ctx;
  BatchArgs a;
  a.pts = make_point_args(r, m, res, flags, 0, r->n);
  a.in = r->batch.dev_as<BatchIn>();
  a.out = reinterpret_cast<BatchOut *>(r->batch.dev_as<BatchIn>() + k);
  a.max_iterations = max_iterations;
  a.it_weight_gradient = it_weight_gradient;
  a.epsilon = epsilon;
  prof_begin(ctx, WS_K_REG);
  const dim3 grid((unsigned)k);
  // 512 lanes: with 1024 the compiler has 128 vector registers per lane and spills 83 to 198 of them to scratch memory (the
  // update alone needs more), whatever the unrolling; with 512 there is no scratch use.
  if (r->batch_variant & 1)
    hipLaunchKernelGGL((reg_batch_kernel<REG_THREADS, 2>), grid, dim3(REG_THREADS), 0, ctx->stream, a);
  else
    hipLaunchKernelGGL((reg_batch_kernel<REG_THREADS, 0>), grid, dim3(REG_THREADS), 0, ctx->stream, a);
  prof_end(ctx, WS_K_REG);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
