// exchange_units.hip — the counted-word exchange of reg_exchange.h, evaluated ON THE DEVICE by ONE wave that waits for nobody: it
// performs every addition of an exchange itself and then polls and folds.  The accumulator words are never reset by the resident
// kernels, so every case starts from preset words:
//   zero, all ones, low 56 bits 2^56 - 1 (the first addition carries into the count), count byte 0xff (the count wraps),
//   low 56 bits 2^56 - 2^37 and 2^56 - 2^36 (the carry happens in mid-exchange), random
// crossed with the totals that are added: random over all of int64, -1 (both halves all ones), zero, a single non-zero slot.
// Expected: the plain uint64 sum of the additions per slot.
//   counted_add/poll/fold   32 counted_add per group, 8 groups, then counted_poll<BOUNDED> and counted_fold
//   counted_publish<false>  the same additions through counted_publish out of wg_sum (left zero), and publish == false adds nothing
//   counted_collect         four consecutive exchanges on two parities with the then_cur / then_other rotation
//   peer_exchange           world 1, 2, 8 with every mailbox pointing to the same buffer (world additions), two exchanges per parity
//   counted_poll gives up   words one addition short, a limit of 2 000 ticks: false and the abort flag set
// Every poll is bounded; a poll that returns false is a mismatch.  Prints one line per helper, exits 1 on any mismatch.
#include <cstdint>
#include <cstring>
#include <vector>

#include "reg_exchange.h"

#include "unit_report.hpp"

using namespace ws;

constexpr uint32_t N_TOTALS = 4, N_PRESETS = 7, N_CASES = N_TOTALS * N_PRESETS; // case = preset * N_TOTALS + totals
constexpr uint32_t PER_GROUP = REG_BLOCKS / REG_GROUPS, ADDS = PER_GROUP * REG_GROUPS;
constexpr long long FAILED_POLL = -1;

// the total of `slot` that addition `call` of exchange `x` of a case adds
__host__ __device__ inline uint64_t total_of(uint32_t line, uint32_t cs, uint32_t x, uint32_t call, uint32_t slot)
{
  const uint64_t h = mix64(((uint64_t)line << 56) ^ ((uint64_t)cs << 44) ^ ((uint64_t)x << 36) ^ ((uint64_t)call << 8) ^ slot);
  switch (cs % N_TOTALS)
  {
  case 0: return h;
  case 1: return ~0ull;
  case 2: return 0;
  default: return slot == (cs / N_TOTALS * 5 + 3) % REG_SLOTS ? (h | 1ull) : 0;
  }
}
// the word at index i of a case's accumulators before anything is added
__host__ __device__ inline uint64_t preset_of(uint32_t line, uint32_t cs, uint32_t i)
{
  const uint64_t h = mix64(0xabcdull ^ ((uint64_t)line << 56) ^ ((uint64_t)cs << 44) ^ i);
  switch (cs / N_TOTALS)
  {
  case 0: return 0;
  case 1: return ~0ull;
  case 2: return (h & ~REG_SUM_MASK) | REG_SUM_MASK;
  case 3: return (0xffull << 56) | (h & REG_SUM_MASK);
  case 4: return (h & ~REG_SUM_MASK) | (REG_COUNT_ONE - (1ull << 37)); // 32 halves of all ones stop 32 short of the carry: the next exchange carries
  case 5: return (h & ~REG_SUM_MASK) | (REG_COUNT_ONE - (1ull << 36)); // the 17th of them carries
  default: return h;
  }
}
static uint64_t sum_of(uint32_t line, uint32_t cs, uint32_t x, uint32_t calls, uint32_t slot)
{
  uint64_t s = 0;
  for (uint32_t c = 0; c < calls; ++c) s += total_of(line, cs, x, c, slot);
  return s;
}

// ---- lines 1 and 2: one workgroup of one wave per case.  acc: [case][REG_GROUPS][REG_WORDS], out: [case][REG_SLOTS] (PUBLISH: x 2)
template <bool PUBLISH>
__global__ __launch_bounds__(64) void k_add_poll_fold(uint32_t line, uint32_t cs, uint64_t *acc_all, uint32_t *abort_flag, int64_t *out, Report *rep)
{
  __shared__ unsigned long long wg_sum[REG_SLOTS];
  const int lane = threadIdx.x & 63;
  uint64_t *acc = acc_all + (size_t)cs * REG_GROUPS * REG_WORDS;
  uint64_t then[REG_GROUPS], w[REG_GROUPS];
#pragma unroll
  for (int g = 0; g < REG_GROUPS; ++g) then[g] = acc[(size_t)g * REG_WORDS + lane];
  for (uint32_t g = 0; g < (uint32_t)REG_GROUPS; ++g)
    for (uint32_t i = 0; i < PER_GROUP; ++i)
    {
      const uint64_t total = total_of(line, cs, 0, g * PER_GROUP + i, (uint32_t)lane & 31u);
      if (PUBLISH)
      {
        // the launch has one workgroup: blockIdx.x / per_group is group 0 of the row that is passed
        if (lane < REG_SLOTS) wg_sum[lane] = total;
        __builtin_amdgcn_wave_barrier();
        counted_publish<false>(acc + (size_t)g * REG_WORDS, wg_sum, true);
        __builtin_amdgcn_wave_barrier();
        if (lane < REG_SLOTS && wg_sum[lane] != 0ull) fail(rep, cs, g, i, lane, (long long)wg_sum[lane], 0);
        if (lane < REG_SLOTS) wg_sum[lane] = ~total;
        __builtin_amdgcn_wave_barrier();
        counted_publish<false>(acc + (size_t)g * REG_WORDS, wg_sum, false); // adds nothing, zeroes all the same
        __builtin_amdgcn_wave_barrier();
        if (lane < REG_SLOTS && wg_sum[lane] != 0ull) fail(rep, cs, g, i, 100 + lane, (long long)wg_sum[lane], 0);
      }
      else
        counted_add<__HIP_MEMORY_SCOPE_AGENT>(acc + (size_t)g * REG_WORDS, total);
    }
  const bool ok = counted_poll<REG_GROUPS, __HIP_MEMORY_SCOPE_AGENT, true>(acc + lane, then, PER_GROUP, w, REG_BARRIER_TIMEOUT_TICKS, abort_flag);
  const int64_t total = ok ? counted_fold(w, then) : FAILED_POLL;
  if (lane < REG_SLOTS) out[(size_t)cs * REG_SLOTS + lane] = total;
  if (!ok && lane == 0) fail(rep, cs, 0, 0, 999, 0, 1);
}

// ---- line 3: counted_collect, exchanges 0 .. 3 on parity x & 1.  acc: [case][2][REG_GROUPS][REG_WORDS], out: [case][4][REG_SLOTS]
__global__ __launch_bounds__(64) void k_collect(uint32_t line, uint32_t cs, uint32_t exchanges, uint64_t *acc_all, uint32_t *abort_flag, int64_t *out, Report *rep)
{
  __shared__ int64_t red[REG_SLOTS];
  const int lane = threadIdx.x & 63;
  uint64_t *acc = acc_all + (size_t)cs * 2 * REG_GROUPS * REG_WORDS;
  uint64_t then_cur[REG_GROUPS], then_other[REG_GROUPS];
#pragma unroll
  for (int g = 0; g < REG_GROUPS; ++g)
  {
    then_cur[g] = acc[(size_t)g * REG_WORDS + lane];
    then_other[g] = acc[(size_t)(REG_GROUPS + g) * REG_WORDS + lane];
  }
  for (uint32_t x = 0; x < exchanges; ++x)
  {
    uint64_t *row = acc + (size_t)(x & 1u) * REG_GROUPS * REG_WORDS;
    for (uint32_t c = 0; c < ADDS; ++c) counted_add<__HIP_MEMORY_SCOPE_AGENT>(row + (size_t)(c / PER_GROUP) * REG_WORDS, total_of(line, cs, x, c, (uint32_t)lane & 31u));
    if (lane < REG_SLOTS) red[lane] = FAILED_POLL;
    __builtin_amdgcn_wave_barrier();
    int64_t total = 0;
    const bool ok = counted_collect(row, abort_flag, then_cur, then_other, red, PER_GROUP, &total);
    __builtin_amdgcn_wave_barrier();
    if (lane < REG_SLOTS)
    {
      out[((size_t)cs * exchanges + x) * REG_SLOTS + lane] = red[lane];
      if (ok && total != red[lane]) fail(rep, cs, x, lane, 998, total, red[lane]);
    }
    if (!ok)
    {
      if (lane == 0) fail(rep, cs, x, 0, 999, 0, 1);
      return;
    }
  }
}

// ---- line 4: peer_exchange, the PeerBlock in ordinary device memory, every mailbox the same buffer [2][REG_WORDS]
__global__ __launch_bounds__(64) void k_peer(uint32_t line, uint32_t cs, uint32_t exchanges, const PeerBlock *pb, uint32_t *abort_flag, int64_t *out, Report *rep)
{
  __shared__ int64_t red[REG_SLOTS];
  const int lane = threadIdx.x & 63;
  uint64_t then[2] = {pb->then[0][lane], pb->then[1][lane]};
  for (uint32_t x = 0; x < exchanges; ++x)
  {
    // lanes 0 .. 31 hold this rank's totals; what the upper lanes hold is nobody's business
    int64_t total = lane < REG_SLOTS ? (int64_t)total_of(line, cs, x, 0, (uint32_t)lane) : (int64_t)mix64(0x5eedull + (uint64_t)lane * 977u + x);
    if (lane < REG_SLOTS) red[lane] = FAILED_POLL;
    __builtin_amdgcn_wave_barrier();
    const bool ok = (x & 1u) ? peer_exchange(pb, 1, then[1], total, red, abort_flag) : peer_exchange(pb, 0, then[0], total, red, abort_flag);
    __builtin_amdgcn_wave_barrier();
    if (lane < REG_SLOTS)
    {
      out[((size_t)cs * exchanges + x) * REG_SLOTS + lane] = red[lane];
      if (ok && total != red[lane]) fail(rep, cs, x, lane, 998, total, red[lane]);
    }
    if (!ok)
    {
      if (lane == 0) fail(rep, cs, x, 0, 999, 0, 1);
      return;
    }
  }
}

// ---- line 5: the bounded poll gives up by itself.  result[0]: what counted_poll returned
__global__ __launch_bounds__(64) void k_give_up(uint64_t *acc, uint32_t *abort_flag, uint32_t *result)
{
  const int lane = threadIdx.x & 63;
  uint64_t then[REG_GROUPS], w[REG_GROUPS];
#pragma unroll
  for (int g = 0; g < REG_GROUPS; ++g) then[g] = acc[(size_t)g * REG_WORDS + lane];
  for (uint32_t c = 0; c + 1 < ADDS; ++c) counted_add<__HIP_MEMORY_SCOPE_AGENT>(acc + (size_t)(c / PER_GROUP) * REG_WORDS, mix64(c * 64u + (uint32_t)lane));
  const bool ok = counted_poll<REG_GROUPS, __HIP_MEMORY_SCOPE_AGENT, true>(acc + lane, then, PER_GROUP, w, 2000, abort_flag);
  if (lane == 0) result[0] = ok ? 1u : 0u;
}

static uint32_t *g_abort;
static void clear_abort() { CHECK_HIP(hipMemset(g_abort, 0, 4)); }
static uint32_t read_abort()
{
  uint32_t v;
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(&v, g_abort, 4, hipMemcpyDeviceToHost));
  return v;
}
// the device's own mismatches (a poll that failed, a slot left non-zero) join the host's comparison in one line
static void finish_line(const char *name, Report &r, unsigned long long expect)
{
  CHECK_HIP(hipDeviceSynchronize());
  Report d;
  CHECK_HIP(hipMemcpy(&d, g_rep, sizeof d, hipMemcpyDeviceToHost));
  for (uint32_t j = 0; j < d.n_rec && j < (uint32_t)MAX_REC; ++j) host_fail(r, d.rec[j][0], d.rec[j][1], d.rec[j][2], d.rec[j][3], d.rec[j][4], d.rec[j][5]);
  if (d.mismatches > d.n_rec) r.mismatches += d.mismatches - d.n_rec;
  if (read_abort() != 0u) host_fail(r, -1, -1, -1, 997, 1, 0); // somebody gave up
  finish_host(name, r, expect);
}

int main()
{
  CHECK_HIP(hipMalloc((void **)&g_rep, sizeof(Report)));
  CHECK_HIP(hipMalloc((void **)&g_abort, 256));
  std::vector<uint64_t> words;
  std::vector<int64_t> out;
  uint64_t *d_acc;
  int64_t *d_out;
  CHECK_HIP(hipMalloc((void **)&d_acc, (size_t)N_CASES * 2 * REG_GROUPS * REG_WORDS * 8));
  CHECK_HIP(hipMalloc((void **)&d_out, (size_t)N_CASES * 3 * 4 * REG_SLOTS * 8));

  // ---- counted_add / counted_publish<false> + counted_poll + counted_fold
  for (uint32_t line = 1; line <= 2; ++line)
  {
    words.resize((size_t)N_CASES * REG_GROUPS * REG_WORDS);
    for (uint32_t cs = 0; cs < N_CASES; ++cs)
      for (uint32_t i = 0; i < (uint32_t)(REG_GROUPS * REG_WORDS); ++i) words[(size_t)cs * REG_GROUPS * REG_WORDS + i] = preset_of(line, cs, i);
    CHECK_HIP(hipMemcpy(d_acc, words.data(), words.size() * 8, hipMemcpyHostToDevice));
    out.assign((size_t)N_CASES * REG_SLOTS, 0);
    CHECK_HIP(hipMemset(d_out, 0x55, out.size() * 8));
    begin();
    clear_abort();
    for (uint32_t cs = 0; cs < N_CASES; ++cs)
    {
      if (line == 1)
        k_add_poll_fold<false><<<dim3(1), dim3(64)>>>(line, cs, d_acc, g_abort, d_out, g_rep);
      else
        k_add_poll_fold<true><<<dim3(1), dim3(64)>>>(line, cs, d_acc, g_abort, d_out, g_rep);
    }
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
    Report r = {};
    for (uint32_t cs = 0; cs < N_CASES; ++cs)
      for (uint32_t s = 0; s < (uint32_t)REG_SLOTS; ++s)
      {
        const uint64_t want = sum_of(line, cs, 0, ADDS, s), got = (uint64_t)out[(size_t)cs * REG_SLOTS + s];
        if (got != want) host_fail(r, cs, s, 0, line, (long long)got, (long long)want);
        ++r.checked;
      }
    if (line == 2)
    {
      // publish == false added nothing, and every word counted exactly its group's additions: word = preset + 32 x 2^56 + halves
      std::vector<uint64_t> after(words.size());
      CHECK_HIP(hipMemcpy(after.data(), d_acc, after.size() * 8, hipMemcpyDeviceToHost));
      for (uint32_t cs = 0; cs < N_CASES; ++cs)
        for (uint32_t s = 0; s < (uint32_t)REG_SLOTS; ++s)
        {
          uint64_t lo = 0, hi = 0;
          for (uint32_t g = 0; g < (uint32_t)REG_GROUPS; ++g)
          {
            const size_t i = ((size_t)cs * REG_GROUPS + g) * REG_WORDS + s;
            lo += (after[i] - words[i]) - PER_GROUP * REG_COUNT_ONE;
            hi += (after[i + REG_SLOTS] - words[i + REG_SLOTS]) - PER_GROUP * REG_COUNT_ONE;
          }
          const uint64_t want = sum_of(line, cs, 0, ADDS, s), got = lo + (hi << 32);
          if (got != want) host_fail(r, cs, s, 1, line, (long long)got, (long long)want);
          ++r.checked;
        }
    }
    finish_line(line == 1 ? "counted_add/poll/fold" : "counted_publish<false>", r, (unsigned long long)N_CASES * REG_SLOTS * line);
  }

  // ---- counted_collect
  {
    const uint32_t line = 3, X = 4;
    words.resize((size_t)N_CASES * 2 * REG_GROUPS * REG_WORDS);
    for (uint32_t cs = 0; cs < N_CASES; ++cs)
      for (uint32_t i = 0; i < (uint32_t)(2 * REG_GROUPS * REG_WORDS); ++i) words[(size_t)cs * 2 * REG_GROUPS * REG_WORDS + i] = preset_of(line, cs, i);
    CHECK_HIP(hipMemcpy(d_acc, words.data(), words.size() * 8, hipMemcpyHostToDevice));
    out.assign((size_t)N_CASES * X * REG_SLOTS, 0);
    CHECK_HIP(hipMemset(d_out, 0x55, out.size() * 8));
    begin();
    clear_abort();
    for (uint32_t cs = 0; cs < N_CASES; ++cs) k_collect<<<dim3(1), dim3(64)>>>(line, cs, X, d_acc, g_abort, d_out, g_rep);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
    Report r = {};
    for (uint32_t cs = 0; cs < N_CASES; ++cs)
      for (uint32_t x = 0; x < X; ++x)
        for (uint32_t s = 0; s < (uint32_t)REG_SLOTS; ++s)
        {
          const uint64_t want = sum_of(line, cs, x, ADDS, s), got = (uint64_t)out[((size_t)cs * X + x) * REG_SLOTS + s];
          if (got != want) host_fail(r, cs, x, s, line, (long long)got, (long long)want);
          ++r.checked;
        }
    finish_line("counted_collect", r, (unsigned long long)N_CASES * X * REG_SLOTS);
  }

  // ---- peer_exchange
  {
    const uint32_t line = 4, X = 4;
    const int worlds[3] = {1, 2, 8};
    PeerBlock *d_pb;
    uint64_t *d_mail;
    CHECK_HIP(hipMalloc((void **)&d_pb, sizeof(PeerBlock)));
    CHECK_HIP(hipMalloc((void **)&d_mail, 2 * REG_WORDS * 8));
    out.assign((size_t)3 * N_CASES * X * REG_SLOTS, 0);
    CHECK_HIP(hipMemset(d_out, 0x55, out.size() * 8));
    begin();
    clear_abort();
    for (uint32_t wi = 0; wi < 3; ++wi)
      for (uint32_t cs = 0; cs < N_CASES; ++cs)
      {
        PeerBlock pb;
        std::memset(&pb, 0, sizeof pb);
        for (int r = 0; r < 8; ++r) pb.mailbox[r] = r < worlds[wi] ? d_mail : nullptr;
        pb.rank = worlds[wi] - 1;
        pb.world = worlds[wi];
        pb.timeout_ticks = (int32_t)REG_PEER_TIMEOUT_TICKS;
        for (uint32_t i = 0; i < (uint32_t)(2 * REG_WORDS); ++i) pb.then[i / REG_WORDS][i % REG_WORDS] = preset_of(line + wi, cs, i);
        CHECK_HIP(hipMemcpy(d_mail, pb.then, sizeof pb.then, hipMemcpyHostToDevice)); // the mailbox as it stood when last complete
        CHECK_HIP(hipMemcpy(d_pb, &pb, sizeof pb, hipMemcpyHostToDevice));
        k_peer<<<dim3(1), dim3(64)>>>(line + wi, cs, X, d_pb, g_abort, d_out + (size_t)wi * N_CASES * X * REG_SLOTS, g_rep);
        CHECK_HIP(hipDeviceSynchronize()); // (the next case overwrites the block and the mailbox)
      }
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
    Report r = {};
    for (uint32_t wi = 0; wi < 3; ++wi)
      for (uint32_t cs = 0; cs < N_CASES; ++cs)
        for (uint32_t x = 0; x < X; ++x)
          for (uint32_t s = 0; s < (uint32_t)REG_SLOTS; ++s)
          {
            const uint64_t want = (uint64_t)worlds[wi] * total_of(line + wi, cs, x, 0, s);
            const uint64_t got = (uint64_t)out[(((size_t)wi * N_CASES + cs) * X + x) * REG_SLOTS + s];
            if (got != want) host_fail(r, worlds[wi], cs, x, s, (long long)got, (long long)want);
            ++r.checked;
          }
    finish_line("peer_exchange", r, (unsigned long long)3 * N_CASES * X * REG_SLOTS);
    CHECK_HIP(hipFree(d_pb));
    CHECK_HIP(hipFree(d_mail));
  }

  // ---- the give-up path: one case
  {
    uint32_t *d_result, result = 7;
    CHECK_HIP(hipMalloc((void **)&d_result, 4));
    CHECK_HIP(hipMemcpy(d_result, &result, 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(d_acc, 0, (size_t)REG_GROUPS * REG_WORDS * 8));
    clear_abort();
    k_give_up<<<dim3(1), dim3(64)>>>(d_acc, g_abort, d_result);
    CHECK_HIP(hipGetLastError());
    const uint32_t flag = read_abort();
    CHECK_HIP(hipMemcpy(&result, d_result, 4, hipMemcpyDeviceToHost));
    Report r = {};
    if (result != 0u) host_fail(r, 0, 0, 0, 0, result, 0); // counted_poll returned false
    if (flag != 1u) host_fail(r, 1, 0, 0, 0, flag, 1);     // and left the abort flag set
    r.checked = 2;
    finish_host("counted_poll gives up", r, 2);
    CHECK_HIP(hipFree(d_result));
  }

  CHECK_HIP(hipFree(d_acc));
  CHECK_HIP(hipFree(d_out));
  CHECK_HIP(hipFree(g_abort));
  CHECK_HIP(hipFree(g_rep));
  printf(g_bad ? "FAILED\n" : "ok\n");
  return g_bad;
}
