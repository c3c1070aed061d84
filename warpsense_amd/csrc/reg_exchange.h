// reg_exchange.h — how the registration kernels (gfx950) hand their sums to each other, fourth layer: the counted-word exchange of
// the resident kernels (loop, server, peers), and agent-scope loads and stores for what crosses a kernel boundary.
#pragma once

#include "reg_points.h"

namespace ws
{
// Exchange of the workgroups' partial sums inside the resident loop, WITHOUT a separate barrier.  Every workgroup ADDS
// its 32 values into one of REG_GROUPS accumulators (agent-scope atomic add, no return); a 64-bit value travels as two
// words -- its low and its high 32 bits -- whose top byte counts the additions: word += (1 << 56) | half.  The
// accumulators are never reset: a reader remembers the word it completed two iterations ago (same parity buffer), so
// (now - then) >> 56 is the number of workgroups that have added since, and the low 56 bits are the exact sum of their
// halves (32 workgroups x 2^32 never reaches bit 56; the differences are taken modulo 2^64, so wrapping is harmless).
// A reader therefore polls the DATA until every word's count is complete: no wait for the adds' acknowledgement, no
// arrival counter, no second read.  tools/barrier_bench.hip (256 workgroups, no work in between): counter + group sums
// 3.1 us per exchange, counted words polled by one wave 2.3 us -- and polling by all waves, more groups or 128-bit
// loads are all slower: the polling reads queue in front of the adds in the same memory channels.
// In the loop itself the polling matters even more than in the microbenchmark: a workgroup that starts to poll right
// after its own adds keeps 256 x 4 KB of coherent reads per round in flight while the adds of the others are still on
// their way, and the exchange takes 3.2 us; sleeping ~0.9 us (the time the adds need anyway) before the FIRST poll makes
// it 1.4 us, because that poll then usually succeeds (measured with -DWS_REG_TIMING, sleeps of 12 / 20 / 26 / 34 / 40 / 50
// x 64 clocks: 2.09 / 1.48 / 1.47 / 1.52 / 1.62 / 1.88 us).  Before: counter barrier + group sums 2.95 us.
// Safe against overtaking: a workgroup can only complete the poll of iteration i + 1 after every workgroup has added
// for i + 1, i.e. after every workgroup has finished reading iteration i, so nobody adds into a parity buffer (i + 2)
// that is still being read.
#ifndef WS_REG_GROUPS
#define WS_REG_GROUPS 8 // (round 5, in the loop itself, first poll after 16 / 26 / 36 x 64 clocks: 4 groups 5.71 / 5.20 / 4.91 us per iteration, 8 groups - / 4.39 / -, 16 groups 6.82 / 5.97 / -)
#endif
constexpr int REG_GROUPS = WS_REG_GROUPS;
constexpr int REG_WORDS = 2 * REG_SLOTS; // low halves, then high halves
constexpr uint64_t REG_COUNT_ONE = 1ull << 56;
constexpr uint64_t REG_SUM_MASK = REG_COUNT_ONE - 1;
static_assert(REG_WORDS == 64 && REG_BLOCKS % REG_GROUPS == 0 && REG_BLOCKS / REG_GROUPS < 256, "counted exchange");
#ifndef WS_REG_FIRST_POLL_SLEEP
#define WS_REG_FIRST_POLL_SLEEP 26 // (round 5, after the shorter solve: 16 / 22 / 25 / 26 / 28 / 30 / 34: 4.97 / 4.47 / 4.40 / 4.40 / 4.42 / 4.46 / 4.58 us per iteration)
#endif
constexpr int REG_FIRST_POLL_SLEEP = WS_REG_FIRST_POLL_SLEEP; // x 64 clocks before the first poll
constexpr int REG_POLL_SLEEP = 2;        // between polls
#ifndef WS_REG_PEER_POLL_SLEEP
#define WS_REG_PEER_POLL_SLEEP 8 // (two ranks on one GPU: 4 -> 6.7, 12 -> 6.9, 20 -> 7.1, 28 -> 7.3 us per iteration; the mailbox is local memory, its polls are cheap)
#endif
constexpr int REG_PEER_POLL_SLEEP = WS_REG_PEER_POLL_SLEEP; // x 64 clocks before the first poll of the mailbox
// Poll limits on the 100 MHz wall clock.  The workgroups of ONE launch start within microseconds of each other, so an on-chip
// exchange that is not complete after 5 ms means that some workgroup is not on the chip (another kernel holds its CU):
// ws_register_cloud then repeats the registration with one launch per iteration, which needs no co-residency -- half a
// frame at 100 Hz lost, not the 2.5 frames at 10 Hz the 0.25 s of round 2 cost.  Ranks of a multi-GPU loop are launched by
// different processes that have just been handed the same scan: their mailboxes wait 20 ms (round 3: 0.25 s; WS_REG_PEER_TIMEOUT_MS
// in the environment at connect time changes it -- ranks that SHARE a GPU in the tests start further apart), kept in the PeerBlock.
constexpr long long REG_BARRIER_TIMEOUT_TICKS = 500000ll;
constexpr long long REG_PEER_TIMEOUT_TICKS = 2000000ll;

// The three steps of a counted exchange, for a wave with all 64 lanes active: lane l < 32 deals in the low half of slot l,
// lane l + 32 in the high half of the same slot.
// counted_add: `total` (in every lane the total of slot lane & 31) into the REG_WORDS words at `row`
template <int SCOPE>
__device__ __forceinline__ void counted_add(uint64_t *row, uint64_t total)
{
  const int lane = threadIdx.x & 63;
  const uint32_t half = lane < REG_SLOTS ? (uint32_t)(total & 0xffffffffull) : (uint32_t)(total >> 32);
  __hip_atomic_fetch_add(&row[lane], REG_COUNT_ONE | half, __ATOMIC_RELAXED, SCOPE);
}

// counted_poll: read this lane's N words (word g at words[g * REG_WORDS]) into w until every word of every lane has counted
// `count` additions since then[g].  BOUNDED: false after `limit` ticks of the wall clock, or once another workgroup has given up
// (*abort_flag, which a workgroup that gives up sets for the others); unbounded polls wait for as long as it takes.
template <int N, int SCOPE, bool BOUNDED>
__device__ __forceinline__ bool counted_poll(uint64_t *words, const uint64_t (&then)[N], uint32_t count, uint64_t (&w)[N], long long limit = 0,
                                             uint32_t *abort_flag = nullptr)
{
  uint32_t spins = 0;
  long long t0 = 0;
  for (;;)
  {
    bool ok = true;
#pragma unroll
    for (int g = 0; g < N; ++g)
    {
      w[g] = __hip_atomic_load(&words[(size_t)g * REG_WORDS], __ATOMIC_RELAXED, SCOPE);
      ok &= ((w[g] - then[g]) >> 56) == (uint64_t)count; // (&=, not &&: && became a branch per word and spilled the loop kernels)
    }
    if (__all(ok)) break;
    __builtin_amdgcn_s_sleep(REG_POLL_SLEEP);
    if (BOUNDED && (++spins & 1023u) == 0)
    {
      const long long now = wall_clock64();
      if (t0 == 0) t0 = now;
      const bool give_up = now - t0 > limit || __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
      if (__any(give_up))
      {
        if ((threadIdx.x & 63) == 0) __hip_atomic_store(abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
    }
  }
  return true;
}

// counted_fold: lanes 0 .. 31 get the total of slot `lane` over the additions the words w have counted since then
template <int N>
__device__ __forceinline__ int64_t counted_fold(const uint64_t (&w)[N], const uint64_t (&then)[N])
{
  uint64_t s = 0;
#pragma unroll
  for (int g = 0; g < N; ++g) s += (w[g] - then[g]) & REG_SUM_MASK;
  const uint64_t high = (uint64_t)shfl_xor_i64((int64_t)s, 32);
  return (int64_t)(s + (high << 32));
}

// first wave (all 64 lanes), after the workgroup's sums are in wg_sum: its total of every slot into the group accumulator
template <bool MFMA = false>
__device__ __forceinline__ void counted_publish(uint64_t *accum /* [REG_GROUPS][REG_WORDS] */, unsigned long long *wg_sum, bool publish,
                                                const uint32_t per_group = REG_BLOCKS / REG_GROUPS, const MfLane *mf = nullptr)
{
  const int lane = threadIdx.x & 63, slot = lane & (REG_SLOTS - 1);
  unsigned long long s;
  if (MFMA)
    s = mfma_finalize(wg_sum, *mf);
  else
  {
    s = wg_sum[slot];
    if (lane < REG_SLOTS) wg_sum[slot] = 0; // for the next pass (the same wave read it one instruction ago)
  }
  if (!publish) return;
  counted_add<__HIP_MEMORY_SCOPE_AGENT>(accum + (size_t)(blockIdx.x / per_group) * REG_WORDS, s);
}

// first wave: poll the accumulators of one parity until all workgroups have added, then red[0..31] = the totals of the
// iteration (read by the same wave afterwards).  then_cur / then_other: this lane's words as they stood when this / the
// other parity was last complete (rotated here).  false: gave up (another kernel is holding CUs this grid needs, or
// another workgroup gave up) -- every workgroup then leaves the loop.
__device__ __forceinline__ bool counted_collect(uint64_t *accum, uint32_t *abort_flag, uint64_t (&then_cur)[REG_GROUPS], uint64_t (&then_other)[REG_GROUPS],
                                                int64_t *red, const uint32_t per_group = REG_BLOCKS / REG_GROUPS, int64_t *total_out = nullptr)
{
  const int lane = threadIdx.x & 63;
  uint64_t w[REG_GROUPS];
  __builtin_amdgcn_s_sleep(REG_FIRST_POLL_SLEEP); // see above: a poll that fails is worse than a poll that starts late
  if (!counted_poll<REG_GROUPS, __HIP_MEMORY_SCOPE_AGENT, true>(accum + lane, then_cur, per_group, w, REG_BARRIER_TIMEOUT_TICKS, abort_flag)) return false;
  const int64_t total = counted_fold(w, then_cur); // lanes 0 .. 31: the total of slot `lane`
#pragma unroll
  for (int g = 0; g < REG_GROUPS; ++g)
  {
    then_cur[g] = then_other[g]; // the other parity is read next
    then_other[g] = w[g];
  }
  if (lane < REG_SLOTS) red[lane] = total;
  if (total_out) *total_out = total;
  return true;
}

// ---- the same exchange ACROSS GPUs (point-sharded registration), inside the resident loop ---------------
// Every rank runs the resident loop on its shard.  After the on-chip exchange above, workgroup 0 of a rank ADDS the rank's 32
// totals -- again as low / high halves whose top byte counts the additions -- into a 2 x 64-word MAILBOX in every rank's
// HBM (its own included): fine-grained memory, peer-mapped (hipIpc) or local, system-scope atomics over xGMI.  Every
// workgroup then polls ITS OWN rank's mailbox (local memory) until the count says that all `world` ranks have added: the
// low 56 bits are the exact sums over the ranks, identical on every rank, and every rank goes on to the identical solve --
// no host, no launch, no RCCL call per iteration.  The words are never reset; what a parity held when it was last
// complete is carried in registers during a launch and in PeerBlock::then from launch to launch (all ranks run the same
// number of iterations, so at the end of a launch every addition ever made has been seen complete by every rank).
struct PeerBlock
{
  uint64_t *mailbox[8]; // [rank] -> that rank's mailbox: [2 parities][REG_WORDS]
  int32_t rank, world;
  uint32_t exchanges; // exchanges completed by all launches so far: the mailbox parity CONTINUES across launches (a rank that
                      // is already in the next registration adds into the parity its slower peers are NOT still polling)
  int32_t timeout_ticks; // poll limit of one exchange on the 100 MHz wall clock
  uint64_t then[2][REG_WORDS];
};
__device__ __forceinline__ bool peer_exchange(const PeerBlock *pb, int parity, uint64_t &then, int64_t &total /* lanes 0..31: in this rank's, out all ranks' */,
                                              int64_t *red, uint32_t *abort_flag)
{
  const int lane = threadIdx.x & 63;
  const int world = pb->world;
  const int64_t other = shfl_xor_i64(total, 32); // lanes 32 .. 63 take the total of slot lane - 32 from the lower half
  const uint64_t mine = (uint64_t)(lane < REG_SLOTS ? total : other);
  if (blockIdx.x == 0)
    for (int r = 0; r < world; ++r) counted_add<__HIP_MEMORY_SCOPE_SYSTEM>(pb->mailbox[r] + (size_t)parity * REG_WORDS, mine);
  const uint64_t before[1] = {then};
  uint64_t w[1];
  __builtin_amdgcn_s_sleep(REG_PEER_POLL_SLEEP);
  if (!counted_poll<1, __HIP_MEMORY_SCOPE_SYSTEM, true>(pb->mailbox[pb->rank] + (size_t)parity * REG_WORDS + lane, before, world, w, pb->timeout_ticks,
                                                        abort_flag))
    return false;
  then = w[0];
  total = counted_fold(w, before);
  if (lane < REG_SLOTS) red[lane] = total;
  return true;
}

// ---- kernels that hand small results to each other through HBM --------------------------------------------------------
// When they are replayed as nodes of a HIP graph, the runtime (ROCm 7.0) does not give a later node the cache maintenance a
// stream gives a later kernel: a batch of 16 iterations converged after ~25 instead of 178 because nodes read stale lines of
// their XCD's L2 (measured; one iteration per graph was fine).  So everything that crosses a kernel boundary here is written
// and read at agent scope (sc1: performed at the coherent level, like the exchange inside the resident loop).
__device__ __forceinline__ int32_t coherent_i32(const int32_t *p) { return __hip_atomic_load(const_cast<int32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int64_t coherent_i64(const int64_t *p) { return __hip_atomic_load(const_cast<int64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void publish_i64(int64_t *p, int64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the state the previous launch (or ws_reg_begin) left, read word by word at agent scope
__device__ __forceinline__ void load_core(GnCore &st, const GnCore *src)
{
  int32_t *w = reinterpret_cast<int32_t *>(&st);
  const int32_t *s = reinterpret_cast<const int32_t *>(src);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(GnCore) / 4); ++i) w[i] = coherent_i32(&s[i]);
}

// the updated state and the sums it was made from (e and c are `int` in the reference), written at agent scope
__device__ __forceinline__ void store_state(GnState *state, const GnCore &st, const int64_t *sums)
{
  const int32_t *w = reinterpret_cast<const int32_t *>(&st);
  int32_t *dst = reinterpret_cast<int32_t *>(&state->core);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(GnCore) / 4); ++i) __hip_atomic_store(&dst[i], w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int k = 0; k < 42; ++k) publish_i64(&state->sums[k], sums[k]);
  publish_i64(&state->sums[42], (int64_t)(int32_t)sums[42]);
  publish_i64(&state->sums[43], (int64_t)(int32_t)sums[43]);
}

} // namespace ws
