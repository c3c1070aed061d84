// api_core.hip — the ground the other host files of the C API stand on (include/warpsense_hip.h; api_map.hip, api_query.hip,
// api_store.hip, api_store_query.hip, api_store_pair.hip, api_pack.hip, api_tsdf.hip, api_reg.hip, api_scan.hip): the last error of a
// thread, the refusals, the context with its stream ordering and hipEvent profiling.  No kernels here or in any api_*.hip.  Entry points are defined at file scope: the header has
// declared each of them with C linkage, so no file wraps anything in a linkage block.  What the files share is in ws_api.h.
#include <cmath>
#include <new>

#include "ws_api.h"

namespace ws
{
// the one last-error slot of a thread: written through set_error, read through ws_last_error
static thread_local std::string g_last_error;

void set_error(const std::string &msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
  char buf[512];
  snprintf(buf, sizeof buf, "HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
  set_error(buf);
  return WS_ERR_HIP;
}

int invalid(const char *msg)
{
  set_error(msg);
  return WS_ERR_INVALID;
}
int invalid(const std::string &msg) { return invalid(msg.c_str()); }

int range_error(const char *name, const char *what)
{
  set_error(std::string(name) + what);
  return WS_ERR_RANGE;
}

static hipEvent_t take_event(ws_context *ctx)
{
  if (!ctx->pool.empty())
  {
    hipEvent_t e = ctx->pool.back();
    ctx->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void prof_begin(ws_context *ctx, int cls)
{
  if (!(ctx->prof_mask & (1u << cls))) return;
  ws_context::Span sp;
  sp.a = take_event(ctx);
  sp.b = take_event(ctx);
  sp.cls = cls;
  (void)hipEventRecord(sp.a, ctx->stream);
  ctx->spans.push_back(sp);
}

void prof_end(ws_context *ctx, int cls)
{
  if (!(ctx->prof_mask & (1u << cls))) return;
  for (size_t i = ctx->spans.size(); i-- > 0;)
  {
    if (ctx->spans[i].cls == cls)
    {
      (void)hipEventRecord(ctx->spans[i].b, ctx->stream);
      return;
    }
  }
}

static void prof_resolve(ws_context *ctx)
{
  for (auto &sp : ctx->spans)
  {
    float ms = 0.f;
    if (hipEventSynchronize(sp.b) == hipSuccess && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess)
    {
      ctx->prof_ms[sp.cls] += ms;
      ctx->prof_n[sp.cls] += 1;
    }
    ctx->pool.push_back(sp.a);
    ctx->pool.push_back(sp.b);
  }
  ctx->spans.clear();
}

// A resident server of ws_reg_iterate (reg_server_kernel) holds the context's stream until it has been idle for 50 us: whoever
// enqueues other work there asks it to leave first (one store into host-mapped memory; the work is ordered behind the kernel
// anyway).  The next ws_reg_iterate waits until that server is really gone and starts a new one -- behind the other work.
void servers_leave(ws_context *ctx)
{
  if (!ctx) return;
  std::lock_guard<std::mutex> lock(ctx->lists_mu);
  for (ws_reg *r : ctx->regs)
  {
    const uint32_t id = r->srv_launch.load(std::memory_order_acquire);
    if (id == 0 || reg_server_mail_exited(r->srv_mail.p) == id) continue;
    reg_server_mail_stop(r->srv_mail.p, id);
    r->srv_stopping.store(true, std::memory_order_release);
  }
}

int ctx_take_errors(ws_context *ctx)
{
  int rc = WS_OK;
  std::lock_guard<std::mutex> lock(ctx->lists_mu);
  for (ws_map *m : ctx->maps)
  {
    const int r = map_take_error(m);
    if (rc == WS_OK) rc = r;
  }
  return rc;
}
} // namespace ws

using namespace ws;

const char *ws_last_error(void) { return g_last_error.c_str(); }
int ws_version(void) { return 1; }

int ws_ctx_create(int device_id, ws_context **out)
{
  if (!out) return invalid("ws_ctx_create: out is NULL");
  // the constant the kernels use for dz_per_distance must be what the reference computes (update_tsdf.cu:49-50)
  {
    float angle = 45.f / 128.f;
    int dz = (int)(std::tan(angle / 180 * M_PI) / 2.0 * MATRIX_RESOLUTION);
    if (dz != DZ_PER_DISTANCE) return invalid("ws_ctx_create: dz_per_distance constant mismatch");
  }
  if (device_id >= 0) WS_HIP(hipSetDevice(device_id));
  int dev = 0;
  WS_HIP(hipGetDevice(&dev));
  ws_context *ctx = new (std::nothrow) ws_context();
  if (!ctx) return invalid("ws_ctx_create: out of host memory");
  ctx->device = dev;
  hipError_t e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess)
  {
    delete ctx;
    return hip_fail(e, "hipStreamCreateWithFlags", __FILE__, __LINE__);
  }
  ctx->stream = ctx->own_stream;
  *out = ctx;
  return WS_OK;
}

int ws_ctx_destroy(ws_context *ctx)
{
  if (!ctx) return WS_OK;
  (void)hipStreamSynchronize(ctx->stream);
  prof_resolve(ctx);
  for (auto e : ctx->pool) (void)hipEventDestroy(e);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  return WS_OK;
}

int ws_ctx_set_stream(ws_context *ctx, void *hip_stream)
{
  if (!ctx) return invalid("ws_ctx_set_stream: ctx is NULL");
  servers_leave(ctx);
  hipStream_t next = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  // work already enqueued on the old stream finishes before anything goes to the new one -- unless one of them is
  // being captured into a graph (a synchronisation would invalidate the capture; the graph orders its own nodes)
  hipStreamCaptureStatus a = hipStreamCaptureStatusNone, b = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(ctx->stream, &a);
  (void)hipStreamIsCapturing(next, &b);
  if (a == hipStreamCaptureStatusNone && b == hipStreamCaptureStatusNone) WS_HIP(hipStreamSynchronize(ctx->stream));
  ctx->stream = next;
  return WS_OK;
}

int ws_sync(ws_context *ctx)
{
  if (!ctx) return invalid("ws_sync: ctx is NULL");
  servers_leave(ctx);
  std::vector<ws_map *> maps;
  {
    std::lock_guard<std::mutex> lock(ctx->lists_mu);
    maps = ctx->maps;
  }
  for (ws_map *m : maps)
  {
    const int rc = settle_tsdf(m); // (an aborted scan is repeated before the stream is drained)
    if (rc != WS_OK) return rc;
  }
  WS_HIP(hipStreamSynchronize(ctx->stream));
  return ctx_take_errors(ctx);
}

int ws_device_reset(void)
{
  WS_HIP(hipDeviceReset());
  return WS_OK;
}

// ------------------------------------------------------------------ measurement
int ws_prof_enable(ws_context *ctx, uint32_t class_mask)
{
  if (!ctx) return invalid("ws_prof_enable: ctx is NULL");
  WS_HIP(hipStreamSynchronize(ctx->stream));
  prof_resolve(ctx);
  ctx->prof_mask = class_mask;
  return WS_OK;
}

int ws_prof_read(ws_context *ctx, int cls, double *total_ms, int64_t *launches)
{
  if (!ctx || cls < 0 || cls >= WS_K_COUNT) return invalid("ws_prof_read: bad argument");
  WS_HIP(hipStreamSynchronize(ctx->stream));
  prof_resolve(ctx);
  if (total_ms) *total_ms = ctx->prof_ms[cls];
  if (launches) *launches = ctx->prof_n[cls];
  return WS_OK;
}

int ws_prof_reset(ws_context *ctx)
{
  if (!ctx) return invalid("ws_prof_reset: ctx is NULL");
  WS_HIP(hipStreamSynchronize(ctx->stream));
  prof_resolve(ctx);
  for (int k = 0; k < WS_K_COUNT; ++k)
  {
    ctx->prof_ms[k] = 0;
    ctx->prof_n[k] = 0;
  }
  return WS_OK;
}
