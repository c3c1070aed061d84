// reg_server.hip — the resident server behind ws_reg_iterate (see reg_loop.hip for all routes): the host's half of its mailbox
// protocol, the kernel and its launcher.  Compiled as a part of reg_routes.hip, which says why.
#include <cstring>

#include "reg_exchange.h"

namespace ws
{
// ---- ... and WITHOUT a launch per call: a resident server (round 6) ----
// The reference's caller is unchanged -- perform_registration once per Gauss-Newton iteration, the solve on the host between
// two calls (tsdf_registration.cpp:55-92) -- and with one launch per call an iteration cost 19.8 us, of which the kernel is 3:
// the rest is the launch.  This kernel stays on the GPU ACROSS calls.  ws_reg_iterate writes the pose and a request number into
// one 64-byte line of host-mapped memory (ServerMail); workgroup 0 polls that line (one read gets request number and pose: only
// twelve of the pose's sixteen floats are used, cu_to_int_mat / registration.cu:208, the other slots carry the number, a stop
// word and a checksum of the snapshot), hands the pose to the other workgroups through device memory, every workgroup does its
// share of calc_jacobis + the reduction (the scan's points stay in registers from call to call), the last one to arrive writes
// the 44 sums and the request number back into host-mapped memory, where the host spins.  The server leaves when nothing has
// been asked for `idle_ticks` (50 us), or at once when the host says so (any other entry point that enqueues work on the
// stream: that work is ordered behind this kernel); ws_reg_iterate starts a new one when it finds none.  A request that
// meets a leaving server is not lost: the number stays in the line, the host sees `exited` without `done` and launches again.
struct ServerMail // host-mapped, 64-byte aligned
{
  uint32_t line[16];  // host -> device: pose words 0-2, 4-6, 8-10, 12-14 (column-major, rows 0-2); [3] request number (written
                      // last), [7] id of the launch the host wants gone, [11] checksum of the pose words and the number
  uint32_t pad[16];
  // device -> host: the 44 sums in seven 64-byte lines of 7 words + a TAG: request number << 32 | a hash of the line's seven words.
  // Every line validates itself, so nothing orders the lines against each other and the kernel does not wait for the writes'
  // acknowledgement before it says "done" (one fabric round trip less per request): the host takes an answer when all seven tags
  // carry its request number and match their lines.
  uint64_t answer[7][8];
  int64_t exited;     // device -> host: id of the last launch that has left the GPU
};
static_assert(offsetof(ServerMail, answer) == 128, "ServerMail");
__host__ __device__ inline uint64_t server_line_tag(uint32_t seq, const uint64_t *w /* 7 words */)
{
  uint64_t x = 0x9E3779B97F4A7C15ull;
#pragma unroll
  for (int k = 0; k < 7; ++k) x = (x << 7 | x >> 57) ^ w[k];
  return ((uint64_t)seq << 32) | (uint32_t)(x ^ (x >> 32));
}
size_t reg_server_mail_bytes() { return sizeof(ServerMail); }
// checksum of the request line: its number `seq` (word 3) and the pose words; word(i) gives word i of the line
template <typename Word>
__host__ __device__ __forceinline__ uint32_t server_checksum(uint32_t seq, Word word)
{
  uint32_t c = 0x5bd1e995u ^ seq;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) c = (c << 5 | c >> 27) ^ word(j * 4 + i);
  return c;
}
void reg_server_mail_write(void *mail, const float T[16], uint32_t seq)
{
  ServerMail *m = static_cast<ServerMail *>(mail);
  uint32_t line[16] = {};
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < 3; ++i) std::memcpy(&line[j * 4 + i], &T[j * 4 + i], 4);
  line[3] = seq;
  volatile uint32_t *dst = m->line;
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < 3; ++i) dst[j * 4 + i] = line[j * 4 + i];
  dst[11] = server_checksum(seq, [&](int i) { return line[i]; });
  std::atomic_thread_fence(std::memory_order_release);
  dst[3] = seq; // the request is complete
}
void reg_server_mail_stop(void *mail, uint32_t launch_id)
{
  volatile uint32_t *dst = static_cast<ServerMail *>(mail)->line;
  dst[7] = launch_id;
}
// the answer to request `seq`, if it is there completely: 1 and the 44 sums, else 0
int reg_server_mail_answer(const void *mail, uint32_t seq, int64_t sums[44])
{
  const ServerMail *m = static_cast<const ServerMail *>(mail);
  uint64_t w[7][8];
  for (int j = 0; j < 7; ++j)
  {
    const volatile uint64_t *src = m->answer[j];
    const uint64_t tag = src[7];
    if ((uint32_t)(tag >> 32) != seq) return 0;
    for (int k = 0; k < 7; ++k) w[j][k] = src[k];
    w[j][7] = tag;
  }
  for (int j = 0; j < 7; ++j)
    if (server_line_tag(seq, w[j]) != w[j][7] || const_cast<volatile uint64_t *>(m->answer[j])[7] != w[j][7]) return 0; // (torn, or being rewritten)
  for (int k = 0; k < 44; ++k) sums[k] = (int64_t)w[k / 7][k % 7];
  return 1;
}
// host half of the protocol without a GPU (tests): a mail block in ordinary memory, an answer written as the kernel writes it, then
// everything that must make the host wait -- a stale request number, a line of the previous answer, a torn line.  0: all as expected
int reg_server_mail_selftest()
{
  ServerMail *m = new ServerMail();
  std::memset(m, 0, sizeof *m);
  int64_t want[44], got[44];
  auto fill = [&](uint32_t seq, int64_t salt) {
    for (int k = 0; k < 44; ++k) want[k] = (int64_t)(0x9E3779B97F4A7C15ull * (uint64_t)(k + 1)) ^ (salt << 17);
    for (int j = 0; j < 7; ++j)
    {
      uint64_t w[7];
      for (int k = 0; k < 7; ++k) w[k] = 7 * j + k < 44 ? (uint64_t)want[7 * j + k] : 0ull;
      for (int k = 0; k < 7; ++k) m->answer[j][k] = w[k];
      m->answer[j][7] = server_line_tag(seq, w);
    }
  };
  int bad = 0;
  if (reg_server_mail_answer(m, 1, got)) bad |= 1; // nothing written yet
  fill(5, 1);
  if (!reg_server_mail_answer(m, 5, got) || std::memcmp(got, want, sizeof want) != 0) bad |= 2;
  if (reg_server_mail_answer(m, 6, got) || reg_server_mail_answer(m, 4, got)) bad |= 4; // another request's answer
  // the next answer arrives line by line: incomplete until the last line is there
  int64_t old[44];
  std::memcpy(old, want, sizeof old);
  const ServerMail before = *m;
  fill(6, 2);
  const ServerMail after = *m;
  for (int upto = 0; upto < 7; ++upto)
  {
    *m = before;
    for (int j = 0; j <= upto; ++j) std::memcpy(m->answer[j], after.answer[j], sizeof m->answer[j]);
    const int ok = reg_server_mail_answer(m, 6, got);
    if (upto < 6 ? ok != 0 : (ok == 0 || std::memcmp(got, want, sizeof want) != 0)) bad |= 8;
  }
  // a torn line: words of the new answer under the old tag, and the other way round
  *m = after;
  m->answer[3][2] = before.answer[3][2];
  if (reg_server_mail_answer(m, 6, got)) bad |= 16;
  *m = after;
  m->answer[3][7] = before.answer[3][7];
  if (reg_server_mail_answer(m, 6, got)) bad |= 32;
  // the request line: what the host writes is what the kernel's checksum accepts
  float T[16];
  for (int i = 0; i < 16; ++i) T[i] = 0.25f * (float)i - 1.f;
  reg_server_mail_write(m, T, 77);
  uint32_t line[16];
  for (int i = 0; i < 16; ++i) line[i] = m->line[i];
  if (line[3] != 77 || line[11] != server_checksum(line[3], [&](int i) { return line[i]; })) bad |= 64;
  delete m;
  return bad;
}
uint32_t reg_server_mail_exited(const void *mail) { return (uint32_t) * const_cast<volatile int64_t *>(&static_cast<const ServerMail *>(mail)->exited); }
// Device memory of the server (ws_reg::srv_ctl, zero at creation, never reset afterwards):
//   lines[REG_GROUPS][16]   the host's line as workgroup 0 has copied it, once per group of 32 workgroups: what a workgroup
//                           polls -- request number, stop word, checksum and pose in ONE 64-byte read, 32 pollers per line
//   accum[REG_GROUPS][64]   counted accumulators (as in reg_loop_kernel): every workgroup ADDS its 32 sums, as low / high
//                           halves whose top byte counts the additions; workgroup 0 polls them until every count has moved
//                           by 32 -- no arrival counter (256 returning atomics on one address are 10 us: tools/doorbell_bench.hip,
//                           12.5 us per round trip with them against 3.0 for the host <-> kernel hop alone), no partials, no second pass
//   then[REG_GROUPS][64]    the accumulators as they stood after the last answered request (kept from launch to launch)
struct ServerCtl
{
  uint32_t lines[REG_GROUPS][16];
  uint64_t accum[REG_GROUPS][REG_WORDS];
  uint64_t then[REG_GROUPS][REG_WORDS];
};
size_t reg_server_ctl_bytes() { return sizeof(ServerCtl); }
struct ServerArgs
{
  PointArgs pts;
  ServerCtl *ctl;
  ServerMail *mail;  // device view
  uint32_t launch_id;
  uint32_t served;   // the last request number that was answered before this launch
  uint32_t idle_ticks; // of the 100 MHz clock
};

// one poll of a 16-word line by lanes 0..15 of a wave: 0 = nothing new, 1 = a request (number in `seq`, pose in `w`), 2 = leave
__device__ __forceinline__ int server_line_state(uint32_t w /* lane l < 16: word l */, uint32_t served, uint32_t launch_id, uint32_t &seq)
{
  seq = (uint32_t)__builtin_amdgcn_readlane((int)w, 3);
  // A request that is waiting is answered BEFORE the server obeys a word to leave: the word comes from another thread's call, whose
  // work is ordered behind this kernel either way, and a caller whose every new server found that word already there (a thread that
  // uploads maps in a loop asks each of them to leave before it has started) would never be answered.
  const bool leave = (uint32_t)__builtin_amdgcn_readlane((int)w, 7) == launch_id;
  if (seq == served || seq == 0) return leave ? 2 : 0;
  // a consistent snapshot?  (the writer stores the number last; a read that saw it and not all of the pose -- torn in two on the
  // way -- fails the checksum and is simply repeated)
  const auto word = [w](int i) { return (uint32_t)__builtin_amdgcn_readlane((int)w, i); };
  return server_checksum(seq, word) == word(11) ? 1 : 0;
}

template <bool MFMA>
__global__ __launch_bounds__(REG_THREADS) void reg_server_kernel(ServerArgs a)
{
  __shared__ unsigned long long wg_sum[REG_SLOTS + MF_AUX]; // the workgroup's totals of a request (LDS atomics of the eight waves)
  __shared__ alignas(16) uint32_t mf_stage[MFMA ? (REG_THREADS / 64) * MF_STAGE_WORDS : 4];
  __shared__ alignas(16) float T_sh[16];
  __shared__ alignas(16) int32_t TI_sh[16];
  __shared__ uint32_t bell_sh; // 0: leave
  // the cloud does not change while a server lives (ws_reg_prepare* stops it): its points stay in registers from call to call,
  // and so do the voxels its first two points per lane fell into with their seven entries (the map does not change either: whoever
  // enqueues an update asks the server to leave first)
  const Prefetched f = prefetch_points(a.pts);
  const bool wave_has_points = __ballot(f.valid[0]) != 0ull;
  const MfLane mfl = make_mf_lane();
  const LoopGather lg = make_loop_gather(a.pts);
  VoxelCache cache[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
  {
    cache[u].bx = cache[u].by = cache[u].bz = 0;
    cache[u].cur = cache[u].xn = cache[u].xl = cache[u].yn = cache[u].yl = cache[u].zn = cache[u].zl = 0;
    cache[u].filled = false;
  }
  constexpr uint32_t per_group = REG_BLOCKS / REG_GROUPS;
  const int lane = threadIdx.x & 63;
  const int group = (int)(blockIdx.x / per_group);
  uint32_t served = a.served;
  uint64_t then[REG_GROUPS];
  if (blockIdx.x == 0 && threadIdx.x < 64)
  {
#pragma unroll
    for (int g = 0; g < REG_GROUPS; ++g) then[g] = a.ctl->then[g][lane];
  }
  if (threadIdx.x < REG_SLOTS + MF_AUX) wg_sum[threadIdx.x] = 0;
  for (;;)
  {
    // ---- wave 0 waits for a request
    if (threadIdx.x < 64)
    {
      uint32_t w = 0, seq = 0;
      int state;
      if (blockIdx.x == 0)
      {
        // the host's line: lanes 0..15 read one word each, in ONE instruction (a 64-byte read of host memory)
        const long long t0 = wall_clock64();
        for (;;)
        {
          if (lane < 16) w = __hip_atomic_load(&a.mail->line[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          state = server_line_state(w, served, a.launch_id, seq);
          if (state != 0) break;
          if (wall_clock64() - t0 > (long long)a.idle_ticks)
          {
            state = 2;
            w = lane == 7 ? a.launch_id : 0u; // (a line that says "leave" to the other workgroups)
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
        // hand it to the other workgroups: one copy per group
        if (lane < 16)
        {
#pragma unroll
          for (int g = 0; g < REG_GROUPS; ++g) __hip_atomic_store(&a.ctl->lines[g][lane], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      else
      {
        for (;;)
        {
          if (lane < 16) w = __hip_atomic_load(&a.ctl->lines[group][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          state = server_line_state(w, served, a.launch_id, seq);
          if (state != 0) break;
          __builtin_amdgcn_s_sleep(4);
        }
      }
      if (lane < 16)
      {
        T_sh[lane] = __uint_as_float(w);
        if (MFMA) store_int_pose(TI_sh, lane, __uint_as_float(w)); // (cu_to_int_mat of the twelve words that are the pose; the other four are never read)
      }
      if (lane == 0) bell_sh = state == 1 ? seq : 0u;
    }
    __syncthreads();
    const uint32_t bell = bell_sh;
    if (bell == 0) break;
    // ---- perform_registration (registration.cu:347-368) for that pose
    if (wave_has_points) pass_sums<MFMA>(a.pts, lg, f, REG_STRIDE, T_sh, TI_sh, cache, mf_stage, mfl, wg_sum, [] {});
    __syncthreads(); // (also keeps T_sh / TI_sh / bell_sh from being rewritten while anybody reads them)
    if (threadIdx.x < 64)
    {
      counted_publish<MFMA>(&a.ctl->accum[0][0], wg_sum, true, per_group, &mfl);
      if (blockIdx.x == 0)
      {
        // ---- all 256 additions, then the 44 words of the reference's h, g, e, c to the host
        uint64_t wv[REG_GROUPS];
        counted_poll<REG_GROUPS, __HIP_MEMORY_SCOPE_AGENT, false>(&a.ctl->accum[0][lane], then, per_group, wv);
        const int64_t total = counted_fold(wv, then); // lanes 0 .. 31: the total of slot `lane`
#pragma unroll
        for (int g = 0; g < REG_GROUPS; ++g) then[g] = wv[g];
        // expand_sums: word k of the reference's 44 comes from the lane that holds its term; lane 8 j + i (i < 7) of the answer holds
        // word 7 j + i, lane 8 j + 7 the tag of line j
        const int line = lane >> 3, wi = lane & 7, k = 7 * line + wi;
        int64_t v = word_value(k, shfl_i64(total, k < 44 ? word_slot(k) : 0));
        if (k >= 44 || wi == 7) v = 0;
        // the tag of a line: from its seven words, gathered into the line's last lane
        uint64_t x = 0x9E3779B97F4A7C15ull;
#pragma unroll
        for (int q = 0; q < 7; ++q) x = (x << 7 | x >> 57) ^ (uint64_t)shfl_i64(v, (lane & ~7) + q);
        const uint64_t tag = ((uint64_t)bell << 32) | (uint32_t)(x ^ (x >> 32));
        if (lane < 56) __hip_atomic_store(&a.mail->answer[line][wi], wi == 7 ? tag : (uint64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    served = bell;
  }
  // ---- workgroup 0 leaves the accumulators' state for the next launch and tells the host that this one is gone (the others
  // have seen the same line and do nothing more; the next launch is ordered behind the end of this kernel)
  if (blockIdx.x == 0 && threadIdx.x < 64)
  {
#pragma unroll
    for (int g = 0; g < REG_GROUPS; ++g) a.ctl->then[g][lane] = then[g];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(&a.mail->exited, (int64_t)a.launch_id, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

int launch_reg_server(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, uint32_t launch_id, uint32_t served, uint32_t idle_us)
{
  ws_context *ctx = r->ctx;
  ServerArgs a;
  a.pts = make_point_args(r, m, res, flags, 0, r->n);
  a.ctl = r->srv_ctl.as<ServerCtl>();
  a.mail = r->srv_mail.dev_as<ServerMail>();
  a.launch_id = launch_id;
  a.served = served;
  a.idle_ticks = idle_us * 100u; // wall_clock64: 100 MHz
  prof_begin(ctx, WS_K_REG);
  // at most one point per lane (every scan the reference's 131 072-point buffers can hold): the sums come from the matrix cores
  if (WS_REG_MFMA && (size_t)(a.pts.end - a.pts.first) <= (size_t)REG_BLOCKS * REG_THREADS)
    hipLaunchKernelGGL(reg_server_kernel<true>, dim3(REG_BLOCKS), dim3(REG_THREADS), 0, ctx->stream, a);
  else
    hipLaunchKernelGGL(reg_server_kernel<false>, dim3(REG_BLOCKS), dim3(REG_THREADS), 0, ctx->stream, a);
  prof_end(ctx, WS_K_REG);
  WS_HIP(hipGetLastError());
  return WS_OK;
}

} // namespace ws
