// api_reg.hip — registration (ws_reg_*, ws_register_cloud*): create and prepare, one iteration through the resident server or one
// launch, the resident loop with its launch-per-iteration route, many start poses in one launch, the peers of a multi-GPU loop, and
// the test entries of all of them; the kernels and their launchers are in reg_loop.hip,
// reg_launches.hip, reg_server.hip and reg_batch.hip.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ws_api.h"

using namespace ws;

// the Gauss-Newton state a registration starts from (tsdf_registration.cpp:28-33)
static GnCore gn_init(const float T_in[16], int32_t max_iterations, float it_weight_gradient, float epsilon)
{
  GnCore c;
  std::memset(&c, 0, sizeof c);
  std::memcpy(c.T, T_in, 16 * sizeof(float));
  for (int k = 0; k < 3; ++k) c.center[k] = (int32_t)T_in[12 + k]; // Point center = total_transform.block<3,1>(0,3).cast<int>()
  c.it_weight_gradient = it_weight_gradient;
  c.epsilon = epsilon;
  c.max_iterations = max_iterations;
  return c;
}

// Spin until done() -- a word a kernel writes into host-mapped memory: a microsecond or two, where waking up from
// hipStreamSynchronize costs tens.  Bounded: after 20 ms the stream is synchronised the ordinary way (a kernel that never ends
// is the runtime's to report), and if done() is still false then, the wait fails with `what`.
template <typename Done>
static int spin_wait(ws_reg *r, Done done, const char *what)
{
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spins = 0; !done();)
    if ((++spins & 0xfffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20))
    {
      WS_HIP(hipStreamSynchronize(r->ctx->stream));
      if (done()) break;
      set_error(what);
      return WS_ERR_INTERNAL;
    }
  std::atomic_thread_fence(std::memory_order_acquire);
  return WS_OK;
}

// ------------------------------------------------------------------ registration
int ws_reg_destroy(ws_reg *r)
{
  if (!r) return WS_OK;
  servers_leave(r->ctx);
  {
    std::lock_guard<std::mutex> lock(r->ctx->lists_mu);
    auto &v = r->ctx->regs;
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i] == r)
      {
        v.erase(v.begin() + (long)i);
        break;
      }
  }
  (void)hipStreamSynchronize(r->ctx->stream);
  (void)ws_reg_peer_disconnect(r);
  r->release();
  delete r;
  return WS_OK;
}

static int reg_reserve(ws_reg *r, size_t n)
{
  if (n <= r->points.cap) return WS_OK;
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  return r->points.grow(n, 3 * sizeof(int32_t), DevBuf::EXACT);
}

// the allocations and first contents of a registration; on an error ws_reg_create frees what is there
static int reg_build(ws_reg *r, size_t max_points)
{
  WS_TRY(reg_reserve(r, max_points));
  WS_TRY(r->partials.alloc(reg_partials_bytes()));
  WS_TRY(r->state.alloc(2, sizeof(GnState)));
  WS_TRY(r->sums_dev.alloc(44, sizeof(int64_t)));
  WS_TRY(r->state_host.alloc(1, sizeof(GnState), HostBlock::PINNED));
  WS_TRY(r->host_flag.alloc(16, sizeof(int32_t), HostBlock::MAPPED));
  WS_TRY(r->result_host.alloc(1, sizeof(GnState), HostBlock::MAPPED));
  WS_TRY(r->iter_host.alloc(64, sizeof(int64_t), HostBlock::MAPPED, true));
  WS_HIP(hipMemsetAsync(r->state.p, 0, 2 * sizeof(GnState), r->ctx->stream));
  WS_TRY(r->grid_bar.alloc(reg_barrier_bytes()));
  WS_TRY(r->pass_arrived.alloc(1, sizeof(uint32_t)));
  WS_HIP(hipMemset(r->pass_arrived.p, 0, sizeof(uint32_t)));
  r->loop_supported = reg_loop_supported(r->ctx->device);
  WS_TRY(r->srv_mail.alloc(reg_server_mail_bytes(), 1, HostBlock::MAPPED, true));
  WS_TRY(r->srv_ctl.alloc(reg_server_ctl_bytes()));
  WS_HIP(hipMemset(r->srv_ctl.p, 0, reg_server_ctl_bytes()));
  if (const char *env = std::getenv("WS_REG_SERVER")) r->srv_enabled = std::atoi(env) != 0;
  if (const char *env = std::getenv("WS_REG_SERVER_IDLE_US")) r->srv_idle_us = (uint32_t)std::max(1, std::atoi(env));
  r->batch_variant = reg_batch_default_variant();
  if (const char *env = std::getenv("WS_REG_BATCH_VARIANT")) r->batch_variant = std::atoi(env) & 1;
  return WS_OK;
}

int ws_reg_create(ws_context *ctx, size_t max_points, ws_reg **out)
{
  if (!ctx || !out) return invalid("ws_reg_create: NULL argument");
  ws_reg *r = new (std::nothrow) ws_reg();
  if (!r) return invalid("ws_reg_create: out of host memory");
  r->ctx = ctx;
  if (max_points == 0) max_points = 128 * 1024; // registration.cu:261
  const int rc = reg_build(r, max_points);
  if (rc != WS_OK)
  {
    ws_reg_destroy(r);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lock(ctx->lists_mu);
    ctx->regs.push_back(r);
  }
  *out = r;
  return WS_OK;
}

int ws_reg_prepare(ws_reg *r, const int32_t *xyz_host, size_t n)
{
  if (!r || (!xyz_host && n)) return invalid("ws_reg_prepare: NULL argument");
  servers_leave(r->ctx); // (a resident server of ws_reg_iterate keeps the cloud in registers: the copy below is ordered behind it)
  int rc = reg_reserve(r, n);
  if (rc != WS_OK) return rc;
  r->n = n;
  if (n) WS_HIP(hipMemcpyAsync(r->points.p, xyz_host, n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, r->ctx->stream));
  return WS_OK;
}

int ws_reg_prepare_dev(ws_reg *r, const int32_t *xyz_dev, size_t n)
{
  if (!r || (!xyz_dev && n)) return invalid("ws_reg_prepare_dev: NULL argument");
  servers_leave(r->ctx);
  int rc = reg_reserve(r, n);
  if (rc != WS_OK) return rc;
  r->n = n;
  if (n) WS_HIP(hipMemcpyAsync(r->points.p, xyz_dev, n * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, r->ctx->stream));
  return WS_OK;
}

const int32_t *ws_reg_points_dev(const ws_reg *r, size_t *n)
{
  if (n) *n = r ? r->n : 0;
  return r ? r->points.as<int32_t>() : nullptr;
}

// ws_reg_iterate through the resident server (reg_server_kernel): see there.  Returns WS_OK with the 44 sums, or an error.
static int reg_iterate_served(ws_reg *r, const ws_map *m, const float T[16], int32_t res, uint32_t flags, int64_t sums[44])
{
  auto exited = [&]() { return reg_server_mail_exited(r->srv_mail.p); };
  uint32_t id = r->srv_launch.load(std::memory_order_acquire);
  bool alive = id != 0 && exited() != id;
  const MapParams &par = m->par[WS_MAP_AVG];
  const bool same = r->srv_sig.map == m && r->srv_sig.points == r->points.p && r->srv_sig.map_data == m->data[WS_MAP_AVG].p && r->srv_sig.n == r->n &&
                    r->srv_sig.res == res && r->srv_sig.flags == flags && std::memcmp(&r->srv_sig.par, &par, sizeof par) == 0;
  if (alive && (!same || r->srv_stopping.load(std::memory_order_acquire)))
  {
    // somebody has enqueued other work behind that server (or the call is for another map / cloud): it must be gone before a
    // request may be written -- it would answer from the state it was launched with
    reg_server_mail_stop(r->srv_mail.p, id);
    const int rc = spin_wait(r, [&] { return exited() == id; }, "ws_reg_iterate: the resident server did not leave");
    if (rc != WS_OK) return rc;
    alive = false;
  }
  uint32_t seq = r->srv_seq + 1;
  if (seq >= 0x7fffffffu) seq = 1;
  r->srv_seq = seq;
  reg_server_mail_write(r->srv_mail.p, T, seq);
  auto launch = [&]() -> int {
    id = ++r->srv_ids ? r->srv_ids : ++r->srv_ids;
    r->srv_sig.map = m;
    r->srv_sig.points = r->points.p;
    r->srv_sig.map_data = m->data[WS_MAP_AVG].p;
    r->srv_sig.n = r->n;
    r->srv_sig.res = res;
    r->srv_sig.flags = flags;
    r->srv_sig.par = par;
    r->srv_stopping.store(false, std::memory_order_release);
    r->srv_launch.store(id, std::memory_order_release);
    r->srv_launches += 1;
    return launch_reg_server(r, m, res, flags, id, r->srv_served, r->srv_idle_us);
  };
  if (!alive)
  {
    const int rc = launch();
    if (rc != WS_OK) return rc;
  }
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0;
  while (!reg_server_mail_answer(r->srv_mail.p, seq, sums))
  {
    if (exited() == id)
    {
      // the server left (idle for too long, or asked to by another thread's call) without having seen this request
      if (reg_server_mail_answer(r->srv_mail.p, seq, sums)) break;
      const int rc = launch();
      if (rc != WS_OK) return rc;
    }
    if ((++spins & 0xfffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20))
    {
      // Not an error yet: the server may be waiting in the stream behind somebody else's work (another thread's upload of a large
      // map takes longer than this).  Drain the stream the ordinary way -- a server that starts finds the request, answers it and
      // leaves when nothing else comes -- and only then look again; a kernel that never ends is the runtime's to report.
      WS_HIP(hipStreamSynchronize(r->ctx->stream));
      if (reg_server_mail_answer(r->srv_mail.p, seq, sums)) break;
      if (exited() == id)
      {
        // (it left on another thread's request without having seen this one: the next turn of the loop starts a new one)
        const int rc = launch();
        if (rc != WS_OK) return rc;
        WS_HIP(hipStreamSynchronize(r->ctx->stream));
        if (reg_server_mail_answer(r->srv_mail.p, seq, sums)) break;
      }
      set_error("ws_reg_iterate: the resident server did not answer");
      return WS_ERR_INTERNAL;
    }
  }
  r->srv_served = seq;
  return WS_OK;
}

int ws_reg_iterate(ws_reg *r, const ws_map *m, const float T[16], int32_t res, uint32_t flags, int64_t h[36], int64_t g[6],
                   int32_t *e, int32_t *c)
{
  if (!r || !m || !T || !h || !g || !e || !c) return invalid("ws_reg_iterate: NULL argument");
  if (res < 1) return invalid("ws_reg_iterate: map_resolution must be positive");
  int64_t sums[44];
  if (r->srv_enabled && r->loop_supported)
  {
    // (no WS_SETTLE here: that would ask the server to leave.  A scan whose verdict is open was enqueued by a call that has
    // already done so, and is settled now; a living server implies a settled map)
    const int rcs = ws::settle_tsdf(const_cast<ws_map *>(m));
    if (rcs != WS_OK) return rcs;
    const int rc = reg_iterate_served(r, m, T, res, flags, sums);
    if (rc != WS_OK) return rc;
  }
  else
  {
    WS_SETTLE(m);
    // One launch, nothing copied by the runtime: the pose travels in the kernel arguments (registration.cu:351 copies it), the
    // sums come back through host-mapped memory with the call's sequence number behind them (registration.cu:356-365 copies
    // four results and adds 32 partials up on the host).  The caller cannot go on without them, so the wait is a spin on that word.
    const uint32_t seq = ++r->iter_seq ? r->iter_seq : ++r->iter_seq; // (never 0: the block starts zeroed)
    int rc = launch_reg_pass(r, m, res, flags, 0, r->n, r->iter_host.dev_as<int64_t>(), 0, T, seq);
    if (rc != WS_OK) return rc;
    const volatile int64_t *done = r->iter_host.as<int64_t>() + 44;
    rc = spin_wait(r, [&] { return (uint32_t)*done == seq; }, "ws_reg_iterate: the launch ended without its result");
    if (rc != WS_OK) return rc;
    std::memcpy(sums, r->iter_host.p, sizeof sums);
  }
  std::memcpy(h, sums, 36 * sizeof(int64_t));
  std::memcpy(g, sums + 36, 6 * sizeof(int64_t));
  *e = (int32_t)sums[42];
  *c = (int32_t)sums[43];
  return map_take_error(const_cast<ws_map *>(m));
}

// test / tuning entry: the resident server of ws_reg_iterate on or off, its idle time; returns the servers launched so far
int ws_debug_reg_mail_selftest(void) { return reg_server_mail_selftest(); }

int ws_debug_reg_server(ws_reg *r, int32_t enable, int32_t idle_us, int32_t *launches)
{
  if (!r) return invalid("ws_debug_reg_server: reg is NULL");
  servers_leave(r->ctx);
  if (enable >= 0) r->srv_enabled = enable ? 1 : 0;
  if (idle_us > 0) r->srv_idle_us = (uint32_t)idle_us;
  if (launches) *launches = (int32_t)r->srv_launches;
  return WS_OK;
}

int ws_reg_begin(ws_reg *r, const float T_in[16], int32_t max_iterations, float it_weight_gradient, float epsilon)
{
  if (!r || !T_in) return invalid("ws_reg_begin: NULL argument");
  GnState *h = r->state_host.as<GnState>();
  // the pinned staging block may still be read by an earlier async copy
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  std::memset(h, 0, sizeof(GnState));
  h->core = gn_init(T_in, max_iterations, it_weight_gradient, epsilon);
  *r->host_flag.as<volatile int32_t>() = 0;
  WS_HIP(hipMemcpyAsync(&r->state.as<GnState>()[0], h, sizeof(GnState), hipMemcpyHostToDevice, r->ctx->stream));
  WS_HIP(hipMemcpyAsync(&r->state.as<GnState>()[1], h, sizeof(GnState), hipMemcpyHostToDevice, r->ctx->stream));
  r->latest = 0;
  return WS_OK;
}

int ws_reg_accumulate_dev(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t first, size_t count, int64_t *sums_dev)
{
  if (!r || !m || !sums_dev) return invalid("ws_reg_accumulate_dev: NULL argument");
  WS_SETTLE(m);
  return launch_reg_pass(r, m, res, flags, first, count, sums_dev, 0);
}

int ws_reg_iterate_shard_dev(ws_reg *r, const ws_map *m, int32_t res, uint32_t flags, size_t first, size_t count, int64_t *sums_dev,
                             int32_t apply_previous)
{
  if (!r || !m || !sums_dev) return invalid("ws_reg_iterate_shard_dev: NULL argument");
  WS_SETTLE(m);
  return launch_reg_pass(r, m, res, flags, first, count, sums_dev, apply_previous);
}

int ws_reg_solve_dev(ws_reg *r, const int64_t *sums_dev)
{
  if (!r || !sums_dev) return invalid("ws_reg_solve_dev: NULL argument");
  return launch_reg_solve(r, sums_dev);
}

int ws_reg_poll(ws_reg *r, int32_t *finished, int32_t *iterations, float T_out[16])
{
  if (!r) return invalid("ws_reg_poll: reg is NULL");
  WS_HIP(hipMemcpyAsync(r->state_host.p, &r->state.as<GnState>()[r->latest], sizeof(GnState), hipMemcpyDeviceToHost, r->ctx->stream));
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  const GnCore *h = &r->state_host.as<GnState>()->core;
  if (finished) *finished = (h->finished || h->iterations >= h->max_iterations) ? 1 : 0;
  if (iterations) *iterations = h->iterations;
  if (T_out) std::memcpy(T_out, h->T, 16 * sizeof(float));
  return WS_OK;
}

// the host side of one resident launch: spin on the flag the kernel raises behind its result (host-mapped memory)
static int wait_resident_loop(ws_reg *r)
{
  const volatile int32_t *done = r->host_flag.as<int32_t>();
  return spin_wait(r, [&] { return *done != 0; }, "the resident registration loop ended without its result");
}

int ws_register_cloud(ws_reg *r, const ws_map *m, const float T_in[16], int32_t max_iterations, float it_weight_gradient,
                      float epsilon, int32_t res, uint32_t flags, float T_out[16], int32_t *iterations)
{
  if (!r || !m || !T_in || !T_out) return invalid("ws_register_cloud: NULL argument");
  WS_SETTLE(m);
  if (res < 1) return invalid("ws_register_cloud: map_resolution must be positive");
  if (r->loop_mode == WS_REG_LOOP_RESIDENT && r->loop_supported)
  {
    // one launch: the 256 workgroups stay resident and meet at a grid barrier between iterations.  The initial state
    // travels in the kernel arguments and the final state comes back through host-mapped memory, so the host neither
    // waits for earlier work on the stream before enqueueing nor copies anything afterwards.
    *r->host_flag.as<volatile int32_t>() = 0; // nothing on the stream writes it any more: every earlier registration was waited for
    int rc = launch_reg_loop(r, m, res, flags, gn_init(T_in, max_iterations, it_weight_gradient, epsilon));
    if (rc != WS_OK) return rc;
    r->latest = 0;
    // The kernel raises the flag in host-mapped memory after its result (release at system scope).  Spinning on it instead of
    // hipStreamSynchronize: 84 -> ~35 us between the end of a registration and the first kernel of the next scan (measured).
    rc = wait_resident_loop(r);
    if (rc != WS_OK) return rc;
    const GnCore *h = &r->result_host.as<GnState>()->core;
    if (!h->error)
    {
      std::memcpy(T_out, h->T, 16 * sizeof(float));
      if (iterations) *iterations = h->iterations;
      return map_take_error(const_cast<ws_map *>(m));
    }
    // The grid barrier timed out: another kernel held compute units the resident grid needs (its workgroups must all
    // be on the chip at once).  Nothing was lost — the loop state is only ever produced from complete sums — so the
    // registration simply runs again with one launch per iteration, which needs no co-residency.
    r->resident_fallbacks += 1;
  }
  int rc = ws_reg_begin(r, T_in, max_iterations, it_weight_gradient, epsilon);
  if (rc != WS_OK) return rc;
  // One launch per iteration: launch k applies update k (from the partial sums launch k-1 left behind) and
  // accumulates for iteration k.  The host just enqueues; the device raises a flag in host-mapped memory on
  // convergence so the host can stop early (launches already enqueued exit at once).
  const volatile int32_t *flag = r->host_flag.as<int32_t>();
  int launched = 0;
  for (int k = 0; k <= max_iterations && !*flag; ++k)
  {
    rc = launch_reg_iteration(r, m, res, flags, k);
    if (rc != WS_OK) return rc;
    launched = k + 1;
  }
  r->latest = launched > 0 ? ((launched - 1) & 1) : 0;
  int fin = 0, iters = 0;
  rc = ws_reg_poll(r, &fin, &iters, T_out);
  if (rc != WS_OK) return rc;
  if (iterations) *iterations = iters;
  return map_take_error(const_cast<ws_map *>(m));
}

// ------------------------------------------------------------------ many start poses, one launch
static int reg_batch_reserve(ws_reg *r, size_t k)
{
  if (k <= r->batch.cap) return WS_OK;
  WS_HIP(hipStreamSynchronize(r->ctx->stream)); // (every batch call has waited for its kernel: nothing reads the old block)
  size_t cap = 64;
  while (cap < k) cap *= 2;
  return r->batch.grow(cap, reg_batch_record_bytes(), HostBlock::MAPPED);
}

int ws_register_cloud_batch(ws_reg *r, const ws_map *m, const float *T_in, size_t k, int32_t max_iterations, float it_weight_gradient,
                            float epsilon, int32_t res, uint32_t flags, float *T_out, int32_t *iterations, int32_t *e_out, int32_t *c_out)
{
  if (!r || !m || (k && (!T_in || !T_out))) return invalid("ws_register_cloud_batch: NULL argument");
  if (res < 1) return invalid("ws_register_cloud_batch: map_resolution must be positive");
  if (k > 0x7fffffffu) return invalid("ws_register_cloud_batch: more than 2^31 - 1 start poses");
  // (a living resident server of ws_reg_iterate is asked to leave here: the launch below is ordered behind it on the stream and
  // must not wait for its idle time to run out)
  WS_SETTLE(m);
  if (k == 0) return map_take_error(const_cast<ws_map *>(m));
  int rc = reg_batch_reserve(r, k);
  if (rc != WS_OK) return rc;
  for (size_t i = 0; i < k; ++i) reg_batch_write(r->batch.p, i, T_in + 16 * i);
  // One launch, nothing copied by the runtime: the start records are read from, and the results written to, host-mapped memory.
  // Neither the state buffers, the loop mode nor the sums of the single route are touched.
  rc = launch_reg_batch(r, m, res, flags, k, max_iterations, it_weight_gradient, epsilon);
  if (rc != WS_OK) return rc;
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  for (size_t i = 0; i < k; ++i)
    reg_batch_read(r->batch.p, k, i, T_out + 16 * i, iterations ? iterations + i : nullptr, e_out ? e_out + i : nullptr, c_out ? c_out + i : nullptr);
  return map_take_error(const_cast<ws_map *>(m));
}

int ws_reg_batch_best(const int32_t *e, const int32_t *c, size_t k, int32_t min_count, int64_t *best)
{
  if (!best || (k && (!e || !c))) return invalid("ws_reg_batch_best: NULL argument");
  int64_t b = -1;
  for (size_t i = 0; i < k; ++i)
  {
    if (c[i] < min_count || c[i] <= 0) continue; // (a mean over no points is no score)
    if (b < 0)
    {
      b = (int64_t)i;
      continue;
    }
    // e[i] / c[i] < e[b] / c[b] with positive counts, exactly: |e| and c are below 2^31, the products below 2^62
    const int64_t lhs = (int64_t)e[i] * (int64_t)c[b], rhs = (int64_t)e[b] * (int64_t)c[i];
    if (lhs < rhs || (lhs == rhs && c[i] > c[b])) b = (int64_t)i;
  }
  *best = b;
  return WS_OK;
}

// ------------------------------------------------------------------ multi-GPU resident loop
static int peer_own_mailbox(ws_reg *r)
{
  if (r->mailbox.p) return WS_OK;
  // fine-grained: coherent for system-scope atomics from every GPU that maps it (and for the polls of the owner).  The one
  // allocation DevBuf does not make itself; it frees it like any other
  WS_HIP(hipExtMallocWithFlags(&r->mailbox.p, 4096, hipDeviceMallocFinegrained));
  r->mailbox.cap = 4096;
  WS_HIP(hipMemset(r->mailbox.p, 0, 4096));
  return WS_OK;
}

int ws_reg_peer_mailbox(ws_reg *r, void *ipc_handle_out)
{
  if (!r) return invalid("ws_reg_peer_mailbox: reg is NULL");
  static_assert(sizeof(hipIpcMemHandle_t) == WS_IPC_HANDLE_BYTES, "WS_IPC_HANDLE_BYTES");
  int rc = peer_own_mailbox(r);
  if (rc != WS_OK) return rc;
  if (ipc_handle_out)
  {
    hipIpcMemHandle_t h;
    WS_HIP(hipIpcGetMemHandle(&h, r->mailbox.p));
    std::memcpy(ipc_handle_out, &h, sizeof h);
  }
  return WS_OK;
}

int ws_reg_peer_disconnect(ws_reg *r)
{
  if (!r) return WS_OK;
  if (r->peer_world) (void)hipStreamSynchronize(r->ctx->stream);
  for (int i = 0; i < 8; ++i)
  {
    if (r->peer_opened[i] && r->peer_mailbox[i]) (void)hipIpcCloseMemHandle(r->peer_mailbox[i]);
    r->peer_opened[i] = false;
    r->peer_mailbox[i] = nullptr;
  }
  r->peer_world = 0;
  return WS_OK;
}

static int peer_finish_connect(ws_reg *r, int rank, int world, int blocks)
{
  if (blocks <= 0) blocks = reg_default_blocks();
  if (blocks % reg_groups() != 0 || blocks > reg_default_blocks()) return invalid("ws_reg_peer_connect: blocks must be a multiple of 8, at most 256");
  std::vector<unsigned char> image(reg_peer_block_bytes());
  reg_peer_block_fill(image.data(), r->peer_mailbox, rank, world);
  if (!r->peer_block_dev.p) WS_TRY(r->peer_block_dev.alloc(reg_peer_block_bytes()));
  WS_HIP(hipMemcpy(r->peer_block_dev.p, image.data(), image.size(), hipMemcpyHostToDevice)); // also zeroes `then`: the mailboxes are fresh
  WS_HIP(hipMemset(r->mailbox.p, 0, reg_mailbox_bytes()));
  r->peer_rank = rank;
  r->peer_world = world;
  r->peer_blocks = blocks;
  r->peer_dirty = false;
  return WS_OK;
}

int ws_reg_peer_connect(ws_reg *r, int32_t rank, int32_t world, const void *ipc_handles, int32_t blocks)
{
  if (!r || !ipc_handles) return invalid("ws_reg_peer_connect: NULL argument");
  if (world < 1 || world > 8 || rank < 0 || rank >= world) return invalid("ws_reg_peer_connect: 1 <= world <= 8, 0 <= rank < world");
  int rc = peer_own_mailbox(r);
  if (rc != WS_OK) return rc;
  (void)ws_reg_peer_disconnect(r);
  // the mailboxes of ranks on other GPUs are reached over xGMI: peer access to every visible device (already enabled / not
  // possible are both fine here: the open below decides)
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess)
    for (int d = 0; d < n_dev; ++d)
      if (d != r->ctx->device)
      {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, r->ctx->device, d) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(d, 0);
      }
  (void)hipGetLastError();
  for (int i = 0; i < world; ++i)
  {
    if (i == rank)
    {
      r->peer_mailbox[i] = r->mailbox.p;
      continue;
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, static_cast<const unsigned char *>(ipc_handles) + (size_t)i * sizeof h, sizeof h);
    void *p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess)
    {
      (void)ws_reg_peer_disconnect(r);
      return hip_fail(e, "hipIpcOpenMemHandle (mailbox of a peer rank)", __FILE__, __LINE__);
    }
    r->peer_mailbox[i] = p;
    r->peer_opened[i] = true;
  }
  return peer_finish_connect(r, rank, world, blocks);
}

int ws_reg_peer_connect_local(ws_reg *r, int32_t rank, int32_t world, ws_reg *const *regs, int32_t blocks)
{
  if (!r || !regs) return invalid("ws_reg_peer_connect_local: NULL argument");
  if (world < 1 || world > 8 || rank < 0 || rank >= world || regs[rank] != r) return invalid("ws_reg_peer_connect_local: regs[rank] must be reg, world <= 8");
  (void)ws_reg_peer_disconnect(r);
  for (int i = 0; i < world; ++i)
  {
    if (!regs[i]) return invalid("ws_reg_peer_connect_local: NULL rank");
    const int rc = peer_own_mailbox(regs[i]);
    if (rc != WS_OK) return rc;
    r->peer_mailbox[i] = regs[i]->mailbox.p;
  }
  return peer_finish_connect(r, rank, world, blocks);
}

int ws_reg_peer_reset(ws_reg *r)
{
  if (!r || !r->peer_world) return invalid("ws_reg_peer_reset: not connected");
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  return peer_finish_connect(r, r->peer_rank, r->peer_world, r->peer_blocks);
}

int ws_register_cloud_peers(ws_reg *r, const ws_map *m, size_t first, size_t count, const float T_in[16], int32_t max_iterations,
                            float it_weight_gradient, float epsilon, int32_t res, uint32_t flags, float T_out[16], int32_t *iterations)
{
  if (!r || !m || !T_in || !T_out) return invalid("ws_register_cloud_peers: NULL argument");
  WS_SETTLE(m);
  if (!r->peer_world) return invalid("ws_register_cloud_peers: ws_reg_peer_connect first");
  // An exchange that was given up leaves partial additions in the mailboxes and no saved snapshot: a rank's stale addition
  // plus its next one would reach count == world and pass for the all-rank total.  Nothing runs until the mailboxes are fresh.
  if (r->peer_dirty) return invalid("ws_register_cloud_peers: the last exchange failed; call ws_reg_peer_reset on every rank (between two barriers) or reconnect first");
  if (res < 1) return invalid("ws_register_cloud_peers: map_resolution must be positive");
  *r->host_flag.as<volatile int32_t>() = 0;
  r->peer_dirty = true; // until this exchange has completed on this rank
  int rc = launch_reg_loop(r, m, res, flags, gn_init(T_in, max_iterations, it_weight_gradient, epsilon), true, first, count);
  if (rc != WS_OK) return rc;
  r->latest = 0;
  rc = wait_resident_loop(r);
  if (rc != WS_OK) return rc;
  const GnCore *h = &r->result_host.as<GnState>()->core;
  if (h->error)
  {
    // a rank did not deliver (its kernel was not on the chip, or the process is gone): every rank times out within one
    // exchange of the first.  The caller re-runs the registration through the RCCL route (warpsense_amd.dist does) after
    // ws_reg_peer_reset on every rank.
    set_error("ws_register_cloud_peers: the exchange with the peer ranks timed out");
    return WS_ERR_TIMEOUT;
  }
  r->peer_dirty = false;
  std::memcpy(T_out, h->T, 16 * sizeof(float));
  if (iterations) *iterations = h->iterations;
  return map_take_error(const_cast<ws_map *>(m));
}

int ws_reg_set_loop(ws_reg *r, int mode)
{
  if (!r || (mode != WS_REG_LOOP_RESIDENT && mode != WS_REG_LOOP_LAUNCHES)) return invalid("ws_reg_set_loop: bad argument");
  r->loop_mode = mode;
  return WS_OK;
}

int ws_debug_reg_stall(ws_reg *r, int32_t stall_next, int32_t *fallbacks)
{
  if (!r) return invalid("ws_debug_reg_stall: NULL argument");
  r->debug_stall_next = stall_next ? 1 : 0;
  if (fallbacks) *fallbacks = r->resident_fallbacks;
  return WS_OK;
}

int ws_debug_reg_sums(ws_reg *r, int64_t sums_out[44])
{
  if (!r || !sums_out) return invalid("ws_debug_reg_sums: NULL argument");
  WS_HIP(hipMemcpyAsync(sums_out, r->state.as<GnState>()[r->latest].sums, 44 * sizeof(int64_t), hipMemcpyDeviceToHost, r->ctx->stream));
  WS_HIP(hipStreamSynchronize(r->ctx->stream));
  return WS_OK;
}

int ws_debug_solve6(ws_context *ctx, const double *A, const double *b, size_t n, double *x, int32_t *status)
{
  if (!ctx || !A || !b || !x || !status) return invalid("ws_debug_solve6: NULL argument");
  DevBuf dA, db, dx, ds;
  const size_t k = n ? n : 1;
  int rc = dA.alloc(k, 36 * sizeof(double));
  if (rc == WS_OK) rc = db.alloc(k, 6 * sizeof(double));
  if (rc == WS_OK) rc = dx.alloc(k, 6 * sizeof(double));
  if (rc == WS_OK) rc = ds.alloc(k, sizeof(int32_t));
  if (rc == WS_OK && n)
  {
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA.p, A, n * 36 * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db.p, b, n * 6 * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) rc = launch_solve6_test(ctx, dA.as<double>(), db.as<double>(), n, dx.as<double>(), ds.as<int32_t>());
    if (e == hipSuccess && rc == WS_OK) e = hipMemcpyAsync(x, dx.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == WS_OK) e = hipMemcpyAsync(status, ds.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = hip_fail(e, "ws_debug_solve6", __FILE__, __LINE__);
  }
  for (DevBuf *buf : {&dA, &db, &dx, &ds}) buf->release();
  return rc;
}
