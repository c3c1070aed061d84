// api_scan.hip — scan pre-processing (ws_scan_*, ws_sweep_poses): one pose per scan, or one per time bin of a sweep; the kernels
// and their launcher are in scan_preprocess.hip.
#include <cmath>
#include <cstring>
#include <new>

#include "ws_api.h"

using namespace ws;

int ws_scan_destroy(ws_scan *sc)
{
  if (!sc) return WS_OK;
  (void)hipStreamSynchronize(sc->ctx->stream);
  sc->release();
  delete sc;
  return WS_OK;
}

// the allocations of a scan pre-processor; on an error ws_scan_create frees what is there
static int scan_build(ws_scan *sc)
{
  const size_t blocks = (sc->cap + 255) / 256;
  WS_TRY(sc->tmp.alloc(sc->cap, 3 * sizeof(int32_t)));
  WS_TRY(sc->out.alloc(sc->cap, 3 * sizeof(int32_t)));
  WS_TRY(sc->slot_of.alloc(sc->cap, sizeof(uint32_t)));
  WS_TRY(sc->keys.alloc(sc->table_slots, sizeof(uint64_t)));
  WS_TRY(sc->first.alloc(sc->table_slots, sizeof(uint32_t)));
  WS_TRY(sc->wg_count.alloc(blocks, sizeof(uint32_t)));
  WS_TRY(sc->wg_off.alloc(blocks, sizeof(uint32_t)));
  WS_TRY(sc->counters.alloc(16, sizeof(uint32_t)));
  return sc->host_count.alloc(16, sizeof(uint32_t), HostBlock::MAPPED);
}

int ws_scan_create(ws_context *ctx, size_t max_points, ws_scan **out)
{
  if (!ctx || !out) return invalid("ws_scan_create: NULL argument");
  if (max_points == 0) max_points = 128 * 1024;
  if (max_points > (1u << 30)) return invalid("ws_scan_create: too many points");
  ws_scan *sc = new (std::nothrow) ws_scan();
  if (!sc) return invalid("ws_scan_create: out of host memory");
  sc->ctx = ctx;
  sc->cap = max_points;
  sc->table_slots = pre_table_slots(max_points);
  const int rc = scan_build(sc);
  if (rc != WS_OK)
  {
    ws_scan_destroy(sc);
    return rc;
  }
  *out = sc;
  return WS_OK;
}

// to_int_mat, util/util.h:8-11
static void scan_int_mat(const float pose[16], int32_t M[16])
{
  for (int k = 0; k < 16; ++k) M[k] = (int32_t)(pose[k] * (float)MATRIX_RESOLUTION);
}

// the count and the error bits of the launches before it
static int scan_finish(ws_scan *sc, size_t *n_out)
{
  uint32_t counters[2] = {0, 0};
  WS_HIP(hipMemcpyAsync(counters, sc->counters.p, sizeof counters, hipMemcpyDeviceToHost, sc->ctx->stream));
  WS_HIP(hipStreamSynchronize(sc->ctx->stream));
  sc->n_out = counters[0];
  if (n_out) *n_out = sc->n_out;
  if (counters[1] & 1u)
  {
    set_error("ws_scan_preprocess: a transformed coordinate is beyond +-2^20 mm");
    return WS_ERR_RANGE;
  }
  return WS_OK;
}

static int scan_run(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const float pose[16], int32_t res, size_t *n_out)
{
  int32_t M[16];
  scan_int_mat(pose, M);
  int rc = launch_scan_preprocess(sc, xyz_dev, n, stride, M, res);
  if (rc != WS_OK) return rc;
  return scan_finish(sc, n_out);
}

int ws_scan_preprocess_dev(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const float pose[16], int32_t res, size_t *n_out)
{
  if (!sc || (!xyz_dev && n) || !pose) return invalid("ws_scan_preprocess_dev: NULL argument");
  if (stride < 3) return invalid("ws_scan_preprocess_dev: a point needs at least 3 floats");
  if (res < 1) return invalid("ws_scan_preprocess_dev: map_resolution must be positive");
  if (n > sc->cap) return invalid("ws_scan_preprocess_dev: more points than ws_scan_create reserved");
  return scan_run(sc, xyz_dev, n, stride, pose, res, n_out);
}

int ws_scan_preprocess(ws_scan *sc, const float *xyz_host, size_t n, size_t stride, const float pose[16], int32_t res, size_t *n_out)
{
  if (!sc || (!xyz_host && n) || !pose) return invalid("ws_scan_preprocess: NULL argument");
  if (stride < 3) return invalid("ws_scan_preprocess: a point needs at least 3 floats");
  if (res < 1) return invalid("ws_scan_preprocess: map_resolution must be positive");
  if (n > sc->cap) return invalid("ws_scan_preprocess: more points than ws_scan_create reserved");
  const size_t floats = n * stride;
  if (floats > sc->in_stage.cap)
  {
    WS_HIP(hipStreamSynchronize(sc->ctx->stream));
    WS_TRY(sc->in_stage.grow(floats, sizeof(float), DevBuf::EXACT));
  }
  if (floats) WS_HIP(hipMemcpyAsync(sc->in_stage.p, xyz_host, floats * sizeof(float), hipMemcpyHostToDevice, sc->ctx->stream));
  return scan_run(sc, sc->in_stage.as<float>(), n, stride, pose, res, n_out);
}

// ---- the sweep form: one pose per time bin
static int sweep_check(const char *who, ws_scan *sc, const float *xyz, size_t n, size_t stride, const float *poses, uint32_t k, const ws_sweep_t *rule, int32_t res)
{
  const std::string w(who);
  if (!sc || (!xyz && n) || !poses || !rule) return invalid(w + ": NULL argument");
  if (stride < 3) return invalid(w + ": a point needs at least 3 floats");
  if (res < 1) return invalid(w + ": map_resolution must be positive");
  if (n > sc->cap) return invalid(w + ": more points than ws_scan_create reserved");
  if (k < 1 || k > WS_SWEEP_MAX_BINS) return invalid(w + ": 1 <= k <= 4096 poses");
  if (rule->time_field == -1)
  {
    if (rule->columns < 1 || n % rule->columns != 0) return invalid(w + ": the point count is not a multiple of the sweep's columns");
  }
  else
  {
    if (rule->time_field < 3 || (size_t)rule->time_field >= stride) return invalid(w + ": time_field must be -1 or an index of the record after x y z");
    if (!std::isfinite(rule->t_begin) || !std::isfinite(rule->t_end) || rule->t_begin == rule->t_end) return invalid(w + ": t_begin and t_end must be finite and differ");
  }
  return WS_OK;
}

static int sweep_run(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const float *poses, uint32_t k, const ws_sweep_t *rule, int32_t res, size_t *n_out)
{
  hipStream_t s = sc->ctx->stream;
  if (!sc->sweep_table.p || !sc->sweep_stage.p)
  {
    WS_HIP(hipStreamSynchronize(s));
    WS_TRY(sc->sweep_table.alloc(WS_SWEEP_MAX_BINS, 16 * sizeof(int32_t)));
    WS_TRY(sc->sweep_stage.alloc(WS_SWEEP_MAX_BINS, 16 * sizeof(int32_t), HostBlock::PINNED));
  }
  // (every call on `sc` ends with a stream synchronise: the staging block of the call before has been read)
  int32_t *rows = sc->sweep_stage.as<int32_t>();
  for (uint32_t b = 0; b < k; ++b) scan_int_mat(poses + 16 * (size_t)b, rows + 16 * (size_t)b);
  WS_HIP(hipMemcpyAsync(sc->sweep_table.p, rows, (size_t)k * 16 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  PreSweep w;
  w.table = sc->sweep_table.as<int32_t>();
  w.k = k;
  const bool by_index = rule->time_field == -1;
  w.columns = by_index ? rule->columns : 1u;
  w.rows = by_index ? (uint32_t)(n / rule->columns) : (uint32_t)n;
  if (w.rows == 0) w.rows = 1; // (n == 0: nothing is launched)
  w.ring_major = rule->ring_major;
  w.time_field = rule->time_field;
  w.t_begin = rule->t_begin;
  w.t_end = rule->t_end;
  int rc = launch_scan_preprocess(sc, xyz_dev, n, stride, nullptr, res, &w);
  if (rc != WS_OK) return rc;
  return scan_finish(sc, n_out);
}

int ws_scan_preprocess_sweep_dev(ws_scan *sc, const float *xyz_dev, size_t n, size_t stride, const float *poses_host, uint32_t k, const ws_sweep_t *rule,
                                 int32_t res, size_t *n_out)
{
  WS_TRY(sweep_check("ws_scan_preprocess_sweep_dev", sc, xyz_dev, n, stride, poses_host, k, rule, res));
  return sweep_run(sc, xyz_dev, n, stride, poses_host, k, rule, res, n_out);
}

int ws_scan_preprocess_sweep(ws_scan *sc, const float *xyz_host, size_t n, size_t stride, const float *poses_host, uint32_t k, const ws_sweep_t *rule,
                             int32_t res, size_t *n_out)
{
  WS_TRY(sweep_check("ws_scan_preprocess_sweep", sc, xyz_host, n, stride, poses_host, k, rule, res));
  const size_t floats = n * stride;
  if (floats > sc->in_stage.cap)
  {
    WS_HIP(hipStreamSynchronize(sc->ctx->stream));
    WS_TRY(sc->in_stage.grow(floats, sizeof(float), DevBuf::EXACT));
  }
  if (floats) WS_HIP(hipMemcpyAsync(sc->in_stage.p, xyz_host, floats * sizeof(float), hipMemcpyHostToDevice, sc->ctx->stream));
  return sweep_run(sc, sc->in_stage.as<float>(), n, stride, poses_host, k, rule, res, n_out);
}

// pure host code, in double (warpsense_hip.h)
int ws_sweep_poses(const float pose_end[16], const float motion[16], uint32_t k, float *poses_out)
{
  if (!pose_end || !motion || !poses_out) return invalid("ws_sweep_poses: NULL argument");
  if (k < 1 || k > WS_SWEEP_MAX_BINS) return invalid("ws_sweep_poses: 1 <= k <= 4096 poses");
  bool identity = true;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
    {
      if (!std::isfinite(pose_end[4 * c + r]) || !std::isfinite(motion[4 * c + r])) return invalid("ws_sweep_poses: non-finite input");
      identity = identity && motion[4 * c + r] == (r == c ? 1.f : 0.f);
    }
  if (identity)
  {
    for (uint32_t b = 0; b < k; ++b) std::memcpy(poses_out + 16 * (size_t)b, pose_end, 16 * sizeof(float));
    return WS_OK;
  }
  // Q = R_motion^T, u = -Q t_motion: the begin frame seen from the end frame (Q(r, c) = motion[4 r + c])
  double Q[3][3], u[3], P[4][4];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Q[r][c] = (double)motion[4 * r + c];
  for (int r = 0; r < 3; ++r) u[r] = -(Q[r][0] * (double)motion[12] + Q[r][1] * (double)motion[13] + Q[r][2] * (double)motion[14]);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) P[r][c] = (double)pose_end[4 * c + r];
  const double v[3] = {0.5 * (Q[2][1] - Q[1][2]), 0.5 * (Q[0][2] - Q[2][0]), 0.5 * (Q[1][0] - Q[0][1])};
  const double sn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), cs = 0.5 * (Q[0][0] + Q[1][1] + Q[2][2] - 1.0);
  if (cs < 0.0) return invalid("ws_sweep_poses: a rotation of more than 90 degrees within one sweep");
  const double angle = std::atan2(sn, cs);
  double a[3] = {0.0, 0.0, 0.0};
  if (sn > 0.0)
    for (int r = 0; r < 3; ++r) a[r] = v[r] / sn;
  const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
  double K2[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K2[r][c] = K[r][0] * K[0][c] + K[r][1] * K[1][c] + K[r][2] * K[2][c];
  for (uint32_t b = 0; b < k; ++b)
  {
    const double w = 1.0 - ((double)b + 0.5) / (double)k, sw = std::sin(w * angle), cw = 1.0 - std::cos(w * angle);
    double rel[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 1}};
    for (int r = 0; r < 3; ++r)
    {
      for (int c = 0; c < 3; ++c) rel[r][c] = (r == c ? 1.0 : 0.0) + sw * K[r][c] + cw * K2[r][c]; // Rodrigues
      rel[r][3] = w * u[r];
    }
    float *out = poses_out + 16 * (size_t)b;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) out[4 * c + r] = (float)(P[r][0] * rel[0][c] + P[r][1] * rel[1][c] + P[r][2] * rel[2][c] + P[r][3] * rel[3][c]);
  }
  return WS_OK;
}

const int32_t *ws_scan_points_dev(const ws_scan *sc) { return sc ? sc->out.as<int32_t>() : nullptr; }

int ws_scan_download(ws_scan *sc, int32_t *xyz_host, size_t capacity_points, size_t *n_out)
{
  if (!sc || !n_out) return invalid("ws_scan_download: NULL argument");
  *n_out = sc->n_out;
  if (sc->n_out == 0) return WS_OK;
  if (!xyz_host || capacity_points < sc->n_out) return invalid("ws_scan_download: buffer too small");
  WS_HIP(hipMemcpyAsync(xyz_host, sc->out.p, sc->n_out * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, sc->ctx->stream));
  WS_HIP(hipStreamSynchronize(sc->ctx->stream));
  return WS_OK;
}
