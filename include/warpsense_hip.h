/*
 * warpsense_hip.h — C ABI of libwarpsense_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for warpsense's data-parallel hot path: every entry point below replaces one
 * member of the reference's CUDA device API (file:line under the reference tree given per function).
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.  The header-only C++
 * classes with the reference's names (cuda::TSDFCuda, cuda::RegistrationCuda, cuda::DeviceMap,
 * cuda::DeviceMapMemWrapper, cuda::pause/cleanup) live in include/warpsense_hip/compat.hpp and forward
 * to these functions; INTEGRATION.md shows the reference-side wiring.
 *
 * Conventions
 *   - all geometry is integer millimetres / voxel indices exactly as in the reference
 *     (include/warpsense/consts.h: MATRIX_RESOLUTION 32768, WEIGHT_RESOLUTION 64);
 *   - a voxel is a packed TSDFEntry: low 16 bits value, high 16 bits weight (include/map/tsdf.h:16-23);
 *   - matrices are column-major like rmagine::Matrix4x4f / Matrix6x6l and Eigen
 *     (include/warpsense/math/matrix4x4.h:175-185, matrix6x6.h:112-115);
 *   - every function returns WS_OK (0) or a negative ws_status; ws_last_error() gives the message of
 *     the calling thread's last failure.  Nothing throws across the ABI.
 *   - work is stream-ordered on the context's HIP stream; functions that return host data synchronise.
 *   - threads and devices: like the reference's CUDA classes the library launches on the CALLING thread's current device.
 *     ws_ctx_create(device_id) makes that device current for the creating thread; a further thread that uses the context's
 *     handles on a multi-GPU node calls hipSetDevice(device_id) once first (HIP's current device is per thread and starts
 *     at 0).  ws_shift_wait / _slab / _end only wait on streams and may be called from any thread as they are.
 *
 * Result semantics: the TSDF scatter is resolved in the canonical serial order of the reference kernel
 * (ascending point index, ray step, fan step — SURVEY.md §7 H1), so results are deterministic and
 * bit-identical to oracle/ws_oracle.c.
 */
#ifndef WARPSENSE_HIP_H
#define WARPSENSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ws_context ws_context; /* one per (process, GPU): device id + stream                          */
typedef struct ws_map ws_map;         /* cuda::TSDFCuda: avg_map_ + new_map_ + scan buffer (update_tsdf.h:9-34) */
typedef struct ws_scan ws_scan;       /* scan pre-processing buffers: App::preprocess (src/warpsense/app.cpp:119-148)   */
typedef struct ws_reg ws_reg;         /* cuda::RegistrationCuda (registration.h:10-45)                          */

typedef enum
{
  WS_OK = 0,
  WS_ERR_INVALID = -1,     /* bad argument                                             */
  WS_ERR_HIP = -2,         /* HIP runtime error (message in ws_last_error)              */
  WS_ERR_TOO_MANY_POINTS = -3, /* scan larger than the 1 000 000-point buffer (update_tsdf.h:33) */
  WS_ERR_CAPACITY = -4,    /* a scan that needs more than 2^27 record sub-chunks: returned by the NEXT call that takes the map (the one
                              that looks at the scan's verdict; the record pool itself cannot overflow: a scan that exhausts it is
                              repeated with a larger one) */
  WS_ERR_RANGE = -5,       /* a ray of more than 65 536 ray steps or 255 fan steps: beyond what the record's key holds even with the
                              widest split; the ray was dropped (sticky).  (A scan whose OWN split is narrower -- 32 768 / 63 for the
                              reference's 131 072-point scans, 8192 / 31 at a million points -- is repeated in pieces of 16 384
                              points with the widest split instead: exact) */
  WS_ERR_TIMEOUT = -6,     /* ws_register_cloud_peers: a peer rank did not deliver (ws_register_cloud itself retries with one
                              launch per iteration instead of returning this) */
  WS_ERR_INTERNAL = -7     /* a device-side consistency check failed (sticky)            */
} ws_status;

/* Sticky device-side errors.  ws_tsdf_update* return after ENQUEUEING the kernels (like the reference,
 * update_tsdf.cu:165), so a problem found by the later kernels (WS_ERR_RANGE / INTERNAL: the
 * map is then not bit-exact) cannot come back from that call.  It is kept in host-visible memory and returned ONCE by the
 * first call on the same map that synchronises afterwards: ws_sync, ws_map_download, ws_register_cloud, ws_tsdf_stats.
 * compat.hpp turns it into the reference's print-and-exit (common.cuh:10-21).  Capacity is not among them: a scan that does
 * not fit the record pool is aborted without touching the maps and repeated with a larger pool by the next call that takes the
 * map, before that call's own work (every such entry point looks at the verdict first; two readers that get there at once -- the
 * reference runs register_cloud and the shift thread's to_host under a SHARED lock -- are serialised inside the library). */

#define WS_MAP_AVG 0 /* TSDFCuda::avg_map() */
#define WS_MAP_NEW 1 /* TSDFCuda::new_map() */

/* integrate pass selection, ws_tsdf_set_integrate() */
#define WS_INTEGRATE_SPARSE 0 /* default: touched 4x4x64-voxel tiles only, folded into the scatter's tile resolve      */
#define WS_INTEGRATE_DENSE 1  /* stream every voxel like cu_avg_tsdf_krnl (update_tsdf.cu:13-43)                      */
#define WS_INTEGRATE_SPARSE_SEPARATE 2 /* touched tiles only, as a separate pass over new_map (the resolve writes new_map) */

/* registration flags */
#define WS_REG_ALL_POINTS 0u
#define WS_REG_COMPAT_REFERENCE_LAUNCH 1u /* reproduce the <<<128,512>>> / N%32 coverage of registration.cu:353-356 */

/* how ws_register_cloud runs the Gauss-Newton loop, ws_reg_set_loop() */
#define WS_REG_LOOP_RESIDENT 0 /* one launch for the whole loop, grid barrier between iterations (default;
                                  falls back to LAUNCHES when the device cannot hold the grid at once) */
#define WS_REG_LOOP_LAUNCHES 1 /* one launch per iteration */

const char *ws_last_error(void);
int ws_version(void);

/* ------------------------------------------------------------------ context ---- */
/* cuda runtime implicit context of the reference; device_id < 0 -> current device */
int ws_ctx_create(int device_id, ws_context **out);
int ws_ctx_destroy(ws_context *ctx);
/* Run all work of this context on a caller-owned hipStream_t (e.g. torch's current stream). NULL restores the own stream. */
int ws_ctx_set_stream(ws_context *ctx, void *hip_stream);
/* cuda::pause()  — src/warpsense/cuda/cleanup.cu:3-6 */
int ws_sync(ws_context *ctx);
/* cuda::cleanup() — src/warpsense/cuda/cleanup.cu:8-11 (hipDeviceReset; invalidates every handle) */
int ws_device_reset(void);

/* ------------------------------------------------------------------ maps ---- */
/* TSDFCuda::TSDFCuda(existing_map, tau, max_weight, map_resolution) — update_tsdf.cu:130-141.
 * Like the reference, BOTH device maps start as copies of host_data (DeviceMapMemWrapper ctor,
 * device_map_wrapper.cu:20-24). host_data may be NULL: both maps are then filled with (tau, 0). */
int ws_map_create(ws_context *ctx, const int32_t size[3], const int32_t pos[3], const int32_t offset[3],
                  const uint32_t *host_data, int32_t tau, int32_t max_weight, int32_t map_resolution, ws_map **out);
int ws_map_destroy(ws_map *map); /* TSDFCuda::~TSDFCuda + ~DeviceMapMemWrapper */
/* DeviceMapMemWrapper::to_device — device_map_wrapper.cu:35-45 (params + all voxels, host -> HBM) */
int ws_map_upload(ws_map *map, int which, const int32_t size[3], const int32_t pos[3], const int32_t offset[3],
                  const uint32_t *host_data);
/* DeviceMapMemWrapper::update_params — device_map_wrapper.cu:47-56 (params only) */
int ws_map_set_params(ws_map *map, int which, const int32_t size[3], const int32_t pos[3], const int32_t offset[3]);
/* DeviceMapMemWrapper::to_host — device_map_wrapper.cu:85-92 (synchronises) */
int ws_map_download(ws_map *map, int which, int32_t size[3], int32_t pos[3], int32_t offset[3], uint32_t *host_data);
/* Device side of TSDFMapping::map_shift (src/warpsense/tsdf_mapping.cpp:97-136 + HDF5LocalMap::shift,
 * src/map/hdf5_local_map.cpp:53-118): instead of moving the WHOLE map through the host, only the slabs that leave
 * or enter the window are packed / unpacked.  Boxes are inclusive world-voxel ranges inside the current window;
 * the host buffer is dense, x major, z fastest.  The caller updates pos/offset with ws_map_set_params in between
 * (exactly the three steps of HDF5LocalMap::shift: save, move window, load).  Both synchronise.
 * The window is pos - size/2 .. pos - size/2 + size - 1 per axis: every ring cell once.  For the reference's odd sizes that is
 * pos - size/2 .. pos + size/2.  An even size (which this ABI admits, the reference's maps never have one) has no centre voxel:
 * its window ends at pos + size/2 - 1, and world voxel pos + size/2 is the ring cell of pos - size/2 again.  A box passes if
 * every corner is within size/2 of pos AND it has no more voxels along any axis than the ring has cells (otherwise
 * WS_ERR_INVALID, nothing is moved): no box addresses a ring cell twice.  ws_map_surface, _mesh, _distance use the same rule.
 * Where a window may be: pos - size/2 .. pos - size/2 + size - 1 must lie in int32 on every axis (the last voxel may be INT32_MAX,
 * the first INT32_MIN).  A map whose window does not (ws_map_create, ws_map_set_params and ws_map_upload do not ask) is refused
 * here, by the three queries, by ws_map_frontier, ws_map_view_gain and ws_map_sample (which takes no box: its kernel forms the
 * window's ends in int32) and by ws_store_save_box / ws_store_load_box with WS_ERR_RANGE before anything is allocated or
 * launched; the inside-the-window test itself is made in 64 bits. */
int ws_map_extract_box(ws_map *map, int which, const int32_t lo[3], const int32_t hi[3], uint32_t *host_out);
int ws_map_insert_box(ws_map *map, int which, const int32_t lo[3], const int32_t hi[3], const uint32_t *host_in);
/* The geometry of a map shift, for every route (the box calls above, ws_shift_begin, ws_shift_device).  Host only: no map, no
 * context, no GPU.  Per axis that moves (x, y, z, like HDF5LocalMap::shift, hdf5_local_map.cpp:53-118), with the window as it is
 * when that axis moves: the box that leaves -- the voxels of the window before the axis step that the window after it no longer
 * holds -- and the box that enters.  The window is the one above (pos - size/2 .. pos - size/2 + size - 1, also for an even
 * size), so no slab is wider than `size` along an axis.  pos / offset: the window's parameters after the last step.
 * A step of up to `size` voxels per axis is accepted, a larger one refused (WS_ERR_INVALID, as is a NULL argument);
 * new_pos == pos gives n = 0.
 * Every window of the plan -- the one at `pos`, the one behind each axis step, the one at new_pos -- must lie in int32 on every
 * axis (the rule stated at ws_map_extract_box), else WS_ERR_RANGE.  Per axis in the order x, y, z the size of the step is tested
 * first and the window behind it second, so a step that is both too large and out of range is WS_ERR_INVALID.  ws_shift_begin and
 * ws_shift_device refuse the same way, in their own name, before anything is allocated or launched: both maps, the store and its
 * directory stay as they were. */
typedef struct
{
  int32_t n;                                /* steps: 0 .. 3 */
  int32_t axis[3], d[3];                    /* of step i: the axis that moves and by how much */
  int32_t leave_lo[3][3], leave_hi[3][3];   /* world boxes that leave (coordinates of the window before that axis moved) */
  int32_t enter_lo[3][3], enter_hi[3][3];   /* world boxes that enter */
  int32_t pos[3], offset[3];                /* of the window after the shift */
} ws_shift_plan_t;
int ws_shift_plan(const int32_t size[3], const int32_t pos[3], const int32_t offset[3], const int32_t new_pos[3], ws_shift_plan_t *out);
/* The same shift OFF the scan path (in the reference TSDFMapping::map_shift runs on its own thread and only blocks the
 * scans while it swaps the maps, tsdf_mapping.cpp:97-136).  ws_shift_begin is stream-ordered on the map's stream and
 * returns without waiting: per step of ws_shift_plan the slab of avg_map that leaves the window is
 * packed into a device staging buffer, pos/offset of BOTH device maps move, and the slab that enters is filled with
 * `fill_entry` (the global map's default entry).  The staged slabs then travel to pinned host memory on a SECOND stream
 * while the next scans already run against the new window.  The caller
 *   - overwrites, with ws_map_insert_box, those parts of the entering slabs the global map already holds (revisits),
 *   - and, typically on a worker thread: ws_shift_wait (blocks on the second stream only), ws_shift_slab for each
 *     leaving slab -> global map, ws_shift_end.
 * The slabs and the refusals of a step larger than the window (WS_ERR_INVALID) and of a window outside int32 (WS_ERR_RANGE) are
 * ws_shift_plan's.
 * new_pos equal to pos gives a ticket without slabs that is ended like any other.
 * One shift can be in flight per map: ws_shift_begin and ws_shift_reserve fail with WS_ERR_INVALID while a ticket is open, and
 * ws_shift_begin while new_map holds entries that have not been integrated.  A refusal leaves both maps as they were. */
typedef struct ws_shift ws_shift;
int ws_shift_begin(ws_map *map, const int32_t new_pos[3], uint32_t fill_entry, ws_shift **out);
/* staging (device + pinned host) for shifts of up to `voxels` leaving voxels, so that no shift has to allocate */
int ws_shift_reserve(ws_map *map, uint64_t voxels);
int ws_shift_count(const ws_shift *shift);                                              /* slabs: 0 .. 3 */
int ws_shift_entering(const ws_shift *shift, int i, int32_t lo[3], int32_t hi[3]);      /* box filled with fill_entry (world voxels) */
int ws_shift_wait(ws_shift *shift);                                                     /* the host copies are complete */
int ws_shift_slab(const ws_shift *shift, int i, int32_t lo[3], int32_t hi[3], const uint32_t **host_data); /* after ws_shift_wait */
int ws_shift_end(ws_shift *shift);
/* the ring-buffer parameters the kernels currently use for `which` (no synchronisation; any of the outputs may be NULL) */
int ws_map_get_params(const ws_map *map, int which, int32_t size[3], int32_t pos[3], int32_t offset[3]);
/* device pointer of the voxel array (uint32 per voxel, z fastest) — what DeviceMap::data_ is on the device */
void *ws_map_device_data(ws_map *map, int which);
int64_t ws_map_n_voxels(const ws_map *map);

/* The surface cloud of a device map: publish_local_map (include/warpsense/visualization/map.h:14-121; called after every map
 * update, src/cpu/fastsense.cpp:115, and for all four maps in test/pcd2tsdf.cpp:134-137) without the whole-map download.  Every
 * voxel of an inclusive world-voxel box with weight > 0 && abs(value) < band (map.h:45; abs on the value as int32, so -32768 never
 * qualifies) becomes one 16-byte RECORD: int32 x, y, z in world voxels, then uint32 raw, the packed entry.  Records come in
 * ascending world (x, y, z), z fastest -- the order of the reference's collapse(3) schedule(static) loop -- so two calls on the
 * same map give identical bytes.  With WS_SURFACE_MARKER the reference's marker is computed as well, 7 float32 per record in a
 * second array of the same order: x y z r g b a, with x = (float)x * (float)map_resolution / 1000.f (two IEEE single roundings,
 * map.h:51-53; geometry_msgs::Point widens these floats to double, which is lossless), r = value / (float)tau, g = 0 for
 * value >= 0, else r = 0, g = -value / (float)tau, b = 0, a = 1 (map.h:55-64; tau is the map's, whatever `band` is).
 *   lo / hi: the box, under the rule of ws_map_extract_box (outside the window: WS_ERR_INVALID); both NULL: the whole window,
 *     [pos - size/2, pos - size/2 + size - 1] per axis.  For the reference's odd sizes that is its left..right loop; for an even size
 *     it visits each ring cell once, where the reference's loop (size + 1 steps) would visit one cell twice -- an explicit box of
 *     more voxels than the ring holds along an axis is refused for the same reason.
 *   band <= 0: the map's tau.
 * Synchronises (the count comes back).  The result buffers belong to the map, grow on demand and stay valid until the next
 * ws_map_surface on it; a result of zero points is WS_OK with *n_out = 0 (the reference only logs).  Read-only on the maps: may run
 * next to ws_register_cloud under the reference's shared lock; calls that use the result buffers are serialised inside the library. */
#define WS_SURFACE_RECORDS 0u /* 16-byte records: x, y, z (world voxels), raw entry */
#define WS_SURFACE_MARKER 1u  /* + the reference's float point and colour per record */
int ws_map_surface(ws_map *map, int which, const int32_t lo[3], const int32_t hi[3], int32_t band, uint32_t flags, size_t *n_out);
const void *ws_map_surface_records_dev(const ws_map *map, size_t *n); /* device memory, n x 16 bytes; NULL when n == 0 */
const float *ws_map_surface_marker_dev(const ws_map *map, size_t *n); /* device memory, n x 7 floats; NULL unless the last call asked for it */
/* copies at most capacity_points points and always reports the total in *n_out; either host pointer may be NULL */
int ws_map_surface_download(ws_map *map, void *records_host, float *marker_host, size_t capacity_points, size_t *n_out);
/* Measurement entry: with enable != 0 the calls above record events around their three launches; ms_out (may be NULL) receives the
 * device time of the count pass, the scan and the emit pass of the last such call.  enable < 0 leaves the setting as it is. */
int ws_debug_surface_timing(ws_map *map, int32_t enable, float ms_out[3]);

/* A triangle mesh of a device map by naive surface nets: one vertex per cell the surface passes through, one quad (two triangles)
 * per lattice edge that crosses the surface.  No table, integers only: the result is exact and the same bytes on every run.
 *   value, weight: the entry's two int16.  A voxel is VALID iff weight > 0; with WS_MESH_ANY_WEIGHT iff weight != 0 (the rule the
 *     registration uses: the fan of the update writes negative weights).  A voxel is INSIDE iff value < 0.
 *   box: inclusive world voxels [lo, hi] under the rules of ws_map_surface (both NULL: the whole window, each ring cell once;
 *     outside the window, hi < lo or more voxels than the ring holds along an axis: WS_ERR_INVALID).
 *   cell c = (x, y, z): the cube with corner voxels c + {0,1}^3, for lo <= c <= hi - 1 per axis (a box one voxel thick along an
 *     axis has no cells: WS_OK, zero vertices, zero faces).  A cell is valid iff its 8 corners are valid, ACTIVE iff valid and its
 *     corners are neither all inside nor all outside.
 *   crossing of the lattice edge from voxel a to b = a + e_k (owner a, axis k): exists iff inside(a) != inside(b).  Its offset
 *     from a along k in mm: o = (2 |va| res + m) / (2 m), m = |va| + |vb| (int64, floor; |-32768| is 32768); 0 <= o <= res.
 *   vertex of an active cell: over the cell's n crossing edges (n >= 3 of its 12) the sum of the crossings' local positions --
 *     per axis 0 or res across the edge, o along it -- divided per axis by n (floor).  World position in mm per axis:
 *     c res + res / 2 + local (res / 2 truncated: the voxel centre of the update).  Record, 16 bytes: int32 x_mm, y_mm, z_mm;
 *     uint32 weight = the smallest corner weight of the cell (of |weight| under WS_MESH_ANY_WEIGHT).
 *     Order: ascending cell (x, y, z), z fastest; a vertex's index is its position in that order.
 *   faces: for every crossing edge (owner a, axis k; i = (k + 1) % 3, j = (k + 2) % 3) whose four cells q0 = a - e_i - e_j,
 *     q1 = a - e_j, q2 = a, q3 = a - e_i all lie in the box's cell range and are all valid, two triangles: (q0, q1, q2), (q0, q2, q3)
 *     if inside(a), else (q0, q2, q1), (q0, q3, q2) -- normals point to the outside, towards the sensor.  Record: 3 uint32 vertex
 *     indices, 12 bytes.  Order: ascending owner voxel (x, y, z), z fastest, then axis 0, 1, 2; the two triangles of a quad adjacent.
 *   A vertex at the rim of the observed region (or of the box) may be referenced by no face; it stays.  Faces of a box refer to
 *     vertices of that box only: the mesh of a box is not a subset of the mesh of the window at its rim.
 * WS_ERR_RANGE: (|coordinate| + 1) res of a box corner does not fit int32, or more than 2^32 - 1 vertices.
 * Synchronises (the two counts come back).  The result buffers belong to the map, grow on demand and stay valid until the next
 * ws_map_mesh on it; they are apart from those of ws_map_surface, neither call invalidates the other's result.  Read-only on the
 * maps: may run next to ws_register_cloud under the reference's shared lock; calls that use the result buffers are serialised
 * inside the library.  Nothing is allocated before the first call. */
#define WS_MESH_DEFAULT 0u
#define WS_MESH_ANY_WEIGHT 1u
int ws_map_mesh(ws_map *map, int which, const int32_t lo[3], const int32_t hi[3], uint32_t flags, size_t *n_vertices, size_t *n_faces);
const void *ws_map_mesh_vertices_dev(const ws_map *map, size_t *n);  /* device memory, n x 16 bytes; NULL when n == 0 */
const uint32_t *ws_map_mesh_faces_dev(const ws_map *map, size_t *n); /* device memory, n x 3 uint32; NULL when n == 0 */
/* copies at most cap_vertices vertices and cap_faces faces (prefixes) and always reports the totals; either host pointer may be NULL */
int ws_map_mesh_download(ws_map *map, void *vertices_host, uint32_t *faces_host, size_t cap_vertices, size_t cap_faces, size_t *n_vertices, size_t *n_faces);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the count passes, the scan and the emit passes */
int ws_debug_mesh_timing(ws_map *map, int32_t enable, float ms_out[3]);

/* Ray cast of a device map: what the sensor would see from a pose -- per ray the first crossing of the surface from the outside,
 * as hit point and range, and on request the TSDF gradient there.  Integers only: the result is exact and the same bytes on every
 * run.  All products and quotients below are int64; "trunc" is C division, "floor" is floor division.
 *   value, weight: the entry's two int16.  A voxel is VALID iff it lies in the window [pos - size/2, pos - size/2 + size - 1] per
 *     axis (the window of ws_map_surface: each ring cell once) and weight > 0; with WS_RAYCAST_ANY_WEIGHT iff weight != 0 (the
 *     registration's rule, as WS_MESH_ANY_WEIGHT).  The sample of voxel v sits at v res + h mm per axis, h = res / 2 truncated (the
 *     voxel centre of the update, the lattice of the mesh).
 *   field at a point p (mm): q = p - h, base voxel b = floor(q / res), f = q - b res (0 <= f < res, per axis).  The cell is the 8
 *     voxels b + {0,1}^3; it is valid iff all 8 are valid.  T(p) = sum over the corners c of value(c) wx wy wz, with w = f on the
 *     far side and res - f on the near side of each axis: the trilinear interpolant times res^3, never divided.  res <= 1024
 *     (else WS_ERR_RANGE), so |T| < 2^46.
 *   ray i: origin o (int32 mm, one for all rays of a call), direction d_i (3 int32, any length, |component| < 2^30; a ray with a
 *     larger component is a no-hit).  L = floor(sqrt(dx^2 + dy^2 + dz^2)) exactly (integer square root).  L == 0: no hit.
 *     Samples k = 0, 1, ..., K, K = max_range / step, step = max(res / 2, 1) (the update's march step), at s_k = k step,
 *     p_k = o + trunc(d s_k / L) per axis (the update's pos + dir * len / distance).
 *   hit: the first k >= 1 with: cell of p_{k-1} valid and T(p_{k-1}) > 0, cell of p_k valid and T(p_k) <= 0 -- a crossing from
 *     outside to inside, seen from the front.  Crossings from inside to outside and anything next to an invalid cell are walked
 *     past; the march goes on to K.  Range t = s_{k-1} + floor(step T_{k-1} / (T_{k-1} - T_k)) (so s_{k-1} <= t <= s_k), hit point
 *     o + trunc(d t / L).
 *   record, 16 bytes, one per ray, in ray order (index i of the input): int32 x_mm, y_mm, z_mm, range_mm; no hit: 0, 0, 0, -1.
 *     With WS_RAYCAST_GRADIENT a second array, 3 int32 per ray in the same order: at g = floor(hit / res) per axis,
 *     value(g + e_k) - value(g - e_k) for k = 0, 1, 2 if all six neighbours are valid, else 0, 0, 0 (also for no hit).  It points
 *     to the outside, towards the sensor; it is not normalised.
 *   WS_RAYCAST_TARGETS: the n x 3 int32 are not directions but map-frame points in mm, d_i = point_i - origin (int64; a component
 *     with |d| >= 2^30 makes that ray a no-hit): a scan left on the device by ws_scan_preprocess or ws_reg_prepare_dev
 *     (ws_scan_points_dev, ws_reg_points_dev) is ray cast where it lies.
 *   A ray may start or run outside the window: those cells are invalid, nothing more.
 * max_range <= 0: WS_ERR_INVALID.  |o| + max_range + 2 res does not fit int32 on an axis, n > 2^27 or res > 1024: WS_ERR_RANGE.
 * n == 0: WS_OK, nothing written.  The walk above defines the records; the implementation shortens it only where they stay the same.
 * Synchronises (*n_hits, may be NULL, is the number of records with range_mm >= 0).  The result buffers belong to the map, grow on
 * demand and stay valid until the next ray cast on it; they are apart from those of ws_map_surface and ws_map_mesh, none of the
 * three calls invalidates another's result.  Read-only on the maps: may run next to ws_register_cloud under the reference's shared
 * lock; calls that use the result buffers are serialised inside the library.  Nothing is allocated before the first call.
 * ws_map_raycast_dev takes an array that is already in device memory (it must stay untouched until the call returns). */
#define WS_RAYCAST_DEFAULT 0u
#define WS_RAYCAST_ANY_WEIGHT 1u
#define WS_RAYCAST_GRADIENT 2u
#define WS_RAYCAST_TARGETS 4u
int ws_map_raycast(ws_map *map, int which, const int32_t origin_mm[3], const int32_t *dirs_host, size_t n, int32_t max_range_mm, uint32_t flags, size_t *n_hits);
int ws_map_raycast_dev(ws_map *map, int which, const int32_t origin_mm[3], const int32_t *dirs_dev, size_t n, int32_t max_range_mm, uint32_t flags, size_t *n_hits);
const void *ws_map_raycast_records_dev(const ws_map *map, size_t *n);     /* device memory, n x 16 bytes; NULL when n == 0 */
const int32_t *ws_map_raycast_gradient_dev(const ws_map *map, size_t *n); /* n x 3 int32; NULL unless the last call asked for it */
/* copies at most capacity_rays records (and gradients: a prefix) and always reports the number of rays; either host pointer may be NULL */
int ws_map_raycast_download(ws_map *map, void *records_host, int32_t *gradient_host, size_t capacity_rays, size_t *n_out);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the upload of the directions (0 for the _dev
 * form), of the march and of the gradient pass of the last call */
int ws_debug_raycast_timing(ws_map *map, int32_t enable, float ms_out[3]);

/* Point sample of a device map: what the map says at n given points -- the fifth query, after surface cloud, mesh, ray cast and
 * distance field.  Integers only.  All products and quotients are int64, "floor" is floor division.  The result is exact and the same
 * bytes on every run.
 *   validity, sample lattice and T(p): those of ws_map_raycast: h = res / 2 truncated, q = p - h, b = floor(q / res), f = q - b res.
 *     The cell is b + {0,1}^3 and is valid iff all 8 voxels are valid.  WS_SAMPLE_ANY_WEIGHT works as WS_RAYCAST_ANY_WEIGHT.
 *   input: n x 3 int32, map-frame points in mm, host or device (_dev form; the array must stay untouched until the call returns).  A
 *     point with a component of magnitude >= 2^30 is a dead point: class 0, record all zero.
 *   record, 16 bytes per point, in input order:
 *     int32 d_mm = floor(T(p) / res^3), or 0 if the cell is not valid.
 *     int32 weight, the smallest corner weight of the cell (of |weight| under ANY_WEIGHT), or 0 if the cell is not valid.
 *     uint32 cls.
 *     uint32 raw, the packed entry of the nearest voxel g = floor(p / res) per axis.  g is always one of the cell's corners, so this
 *       costs no extra load.  It is given whenever g lies in the field, valid or not: inside the window.  Otherwise it is 0.  This is
 *       the voxel the registration itself looks up.
 *   classes, decided by band_mm (band_mm <= 0 means the map's tau):
 *     0 UNKNOWN  cell not valid
 *     1 FREE     d_mm >= band
 *     2 SURFACE  -band < d_mm < band
 *     3 INSIDE   d_mm <= -band
 *     counts[4] (uint64, may be NULL) receives the number of points per class.  The call synchronises, as the other queries do.
 *   WS_SAMPLE_GRADIENT: a second array, 3 int32 per point in input order.  It uses the gradient rule of ws_map_raycast at
 *     g = floor(p / res): value(g + e_k) - value(g - e_k) if all six neighbours are valid, else 0, 0, 0.  Dead points also get 0, 0, 0.
 *   WS_SAMPLE_SELECT_UNKNOWN / _FREE / _SURFACE / _INSIDE (four flag bits): with any of them set, a third array holds the input points
 *     whose class is selected, 3 int32 each, in input order.  It is an ordered compaction.  Its length is the sum of the selected
 *     counts.  It is device memory fit to be handed to ws_tsdf_update_dev, ws_reg_prepare_dev or
 *     ws_map_raycast_dev(..., WS_RAYCAST_TARGETS).
 *   errors: WS_ERR_INVALID: unknown flag bits, bad `which`.  WS_ERR_RANGE: res > 1024, n > 2^27, a window that does not lie in int32
 *     (the rule stated at ws_map_extract_box).  On a refusal nothing is launched and
 *     the last result stays.  n == 0 is WS_OK, counts zero, nothing written; the result is then that of a call without points (the
 *     earlier one is gone, as after any accepted call).  A call that was accepted and then fails (WS_ERR_HIP: an allocation, a
 *     launch) also leaves no result: the earlier one is dropped before the buffers grow.
 *   ownership and ordering: the buffers belong to the map and are not allocated before the first call.  They grow on demand and stay
 *     valid until the next sample call on the same map.  They are apart from the buffers of the other four queries.  The calls are
 *     read-only on the maps and stream-ordered on the context's stream.  They are serialised inside the library like the other
 *     queries.  Every output write is bounded by the buffers' capacities. */
#define WS_SAMPLE_DEFAULT 0u
#define WS_SAMPLE_ANY_WEIGHT 1u
#define WS_SAMPLE_GRADIENT 2u
#define WS_SAMPLE_SELECT_UNKNOWN 4u
#define WS_SAMPLE_SELECT_FREE 8u
#define WS_SAMPLE_SELECT_SURFACE 16u
#define WS_SAMPLE_SELECT_INSIDE 32u
#define WS_SAMPLE_UNKNOWN 0u
#define WS_SAMPLE_FREE 1u
#define WS_SAMPLE_SURFACE 2u
#define WS_SAMPLE_INSIDE 3u
int ws_map_sample(ws_map *map, int which, const int32_t *points_host, size_t n, int32_t band_mm, uint32_t flags, uint64_t counts[4]);
int ws_map_sample_dev(ws_map *map, int which, const int32_t *points_dev, size_t n, int32_t band_mm, uint32_t flags, uint64_t counts[4]);
const void *ws_map_sample_records_dev(const ws_map *map, size_t *n);     /* device memory, n x 16 bytes; NULL when n == 0 */
const int32_t *ws_map_sample_gradient_dev(const ws_map *map, size_t *n); /* n x 3 int32; NULL unless the last call asked for it */
const int32_t *ws_map_sample_selected_dev(const ws_map *map, size_t *n); /* n_selected x 3 int32; NULL unless asked for, or empty */
/* copies at most capacity_points records (and gradients) and capacity_selected selected points (prefixes) and always reports the
 * totals; any host pointer may be NULL, and so may n_selected */
int ws_map_sample_download(ws_map *map, void *records_host, int32_t *gradient_host, int32_t *selected_host, size_t capacity_points, size_t capacity_selected,
                           size_t *n_out, size_t *n_selected);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the upload of the points (0 for the _dev form), of
 * the sample pass and of the select passes (scan and emit) of the last call */
int ws_debug_sample_timing(ws_map *map, int32_t enable, float ms_out[3]);

/* Distance field of a device map: per voxel of a box the squared Euclidean distance, in voxels, to the nearest obstacle of that
 * box -- the untruncated distance a planner, a collision checker or a cost map asks for, which the TSDF (truncated at tau) cannot
 * give.  Integers only: the result is exact and the same bytes on every run.  "d2" is a squared distance in voxels.
 *   box: inclusive world voxels [lo, hi] under the rules of ws_map_surface (both NULL: the whole window,
 *     [pos - size/2, pos - size/2 + size - 1] per axis, each ring cell once; outside the window, hi < lo or more voxels than the
 *     ring holds along an axis: WS_ERR_INVALID).  n = (nx, ny, nz) its extent.
 *   classes of a voxel of the box, from its entry's two int16: VALID iff weight > 0; with WS_DISTANCE_ANY_WEIGHT iff weight != 0
 *     (the registration's rule, as WS_MESH_ANY_WEIGHT).  class 2 = OCCUPIED: valid and value < 0 (the mesh's "inside");
 *     class 1 = FREE: valid and value >= 0; class 0 = UNKNOWN: not valid.
 *   sites: the occupied voxels of the box; with WS_DISTANCE_UNKNOWN_OCCUPIED also its unknown voxels (the conservative planner's
 *     reading: what was never seen is not free).  Voxels outside the box are never sites: the field of a box is NOT the
 *     restriction of the field of the window to it -- an obstacle just beyond a face of the box does not show (as with the rim of
 *     the mesh of a box).
 *   field: R = max_dist_vox, 1 <= R <= 255 (else WS_ERR_RANGE; R^2 = 65 025 fits 16 bits, which is what lets the passes over the
 *     box carry 2 bytes per voxel).  For every voxel v of the box d2(v) = min(R², min over sites s of |v - s|²); no site in
 *     reach: R².  A site has d2 = 0.
 *   record, one uint32 per voxel: bits 0..23 d2, bits 30..31 the class, the rest 0.  Order: the dense box, x major, z fastest --
 *     the order of ws_map_extract_box.  nx ny nz records.
 *   WS_DISTANCE_COLUMNS (the 2-D cost map of a ground robot; the box's z range is the robot's height band): a column (x, y) is a
 *     site iff any voxel of it in the box is a site; its class is that of a site's (2, or 0 if only unknown voxels made it a site),
 *     else 1 if any voxel of it is free, else 0.  d2 is the 2-D squared distance between columns, same clamp.  nx ny records, y
 *     fastest.
 * A box without any site is WS_OK, every d2 = R².  More than 2^32 - 1 records: WS_ERR_RANGE.  Unknown flag bits: WS_ERR_INVALID.
 * The minimum above defines the records; the implementation (three separable line passes) gets there another way and leaves
 * them the same.
 * Synchronises (*n_sites, may be NULL, receives the number of site voxels / site columns).  The result buffer belongs to the map,
 * grows on demand, stays valid until the next ws_map_distance on it and is apart from those of ws_map_surface, ws_map_mesh and
 * ws_map_raycast: none of the four calls invalidates another's result.  Read-only on the maps: may run next to ws_register_cloud
 * under the reference's shared lock; calls that use the result buffer are serialised inside the library.  Nothing is allocated
 * before the first call; an allocation that fails returns WS_ERR_HIP and leaves the map usable. */
#define WS_DISTANCE_DEFAULT 0u
#define WS_DISTANCE_ANY_WEIGHT 1u
#define WS_DISTANCE_UNKNOWN_OCCUPIED 2u
#define WS_DISTANCE_COLUMNS 4u
int ws_map_distance(ws_map *map, int which, const int32_t lo[3], const int32_t hi[3], int32_t max_dist_vox, uint32_t flags, size_t *n_sites);
const uint32_t *ws_map_distance_dev(const ws_map *map, size_t *n); /* device memory, n records; NULL before the first call (n == 0) */
/* copies at most `capacity` records (a prefix) and always reports the total in *n_out; host may be NULL */
int ws_map_distance_download(ws_map *map, uint32_t *host, size_t capacity, size_t *n_out);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of pass 0 (classification) and of the x, y and z
 * line passes of the last call (under WS_DISTANCE_COLUMNS: pass 0, the x pass, the y pass, 0) */
int ws_debug_distance_timing(ws_map *map, int32_t enable, float ms_out[4]);

/* Ground of a device map: per (x, y) column of a box the one level something can stand on, its sub-voxel height and the largest
 * height step to the neighbouring columns -- the elevation layer a ground robot plans on.  WS_DISTANCE_COLUMNS models one flat
 * floor: a ramp is a wall where it enters the height band, a kerb blocks or vanishes with the band, a hole or a stair head reads as
 * free ground, a table blocks only if the band cuts it.  The TSDF holds what is needed to do better: a zero crossing with free space
 * above it is a place to stand.  Integers only: the result is exact and the same bytes on every run.
 *   box: inclusive world voxels [lo, hi] under the box rules of ws_map_distance (both NULL: the whole window; outside the window,
 *     hi < lo, exactly one NULL or more voxels than the ring holds along an axis: WS_ERR_INVALID).  More than 2^32 - 1 columns:
 *     WS_ERR_RANGE.
 *   classes of a voxel: those of ws_map_distance, 0 UNKNOWN, 1 FREE (valid, value >= 0), 2 OCCUPIED (valid, value < 0).  VALID iff
 *     weight > 0; with WS_GROUND_ANY_WEIGHT iff weight != 0.
 *   headroom: clear_vox = H, 1 <= H <= 64, else WS_ERR_RANGE.  (The walk goes down a column in steps of 64 voxels and carries ONE
 *     64-bit word of the step above: headroom of up to 64 voxels above a voxel of a step ends in the step above at the latest.)
 *   level: voxel z of column (x, y) is a level iff z and z + H lie in the box's z range, class(z) = OCCUPIED, class(z + 1) = FREE and
 *     class(z + k) = FREE for k = 2 .. H.  With WS_GROUND_UNKNOWN_HEADROOM, UNKNOWN is accepted as well for k = 2 .. H; z + 1 must be
 *     FREE in every case, because the height needs its value.  Voxels outside the box never count: as with the frontier and the
 *     distance field, the result of a box is NOT the restriction of a larger box's result to it.
 *   the level of a column: its lowest level; under WS_GROUND_TOP its highest.  One level per column: a caller who wants one storey
 *     of several cuts it with the box's z range.
 *   height: with v0 = value(z) < 0 and v1 = value(z + 1) >= 0, frac = min(255, floor(256 (-v0) / (v1 - v0))) and h = 256 z + frac as
 *     int64: the zero crossing in 1/256 voxel, between voxel centres.
 *   class of a column: 1 GROUND if it has a level; else 2 BLOCKED if any voxel of it in the box is OCCUPIED; else 3 VOID if any is
 *     FREE (a hole, a stair head: seen, and nothing to stand on); else 0 UNKNOWN.
 *   step, defined for a GROUND column c only: min(65535, max |h(c) - h(n)|) over the up to 8 neighbouring columns n of the box that
 *     are GROUND; 0 if there is none.
 *   record, 8 bytes per column in the column order of ws_map_distance (x major, y fastest): int32 z, the level's voxel (0 without a
 *     level); uint32 w: bits 0..7 frac, bits 8..23 step, bits 30..31 the column's class, the rest 0.  nx ny records.
 *   counts[4] (may be NULL) receives the columns per class.  A box of zero columns is WS_OK.
 * Every refusal comes before the first launch and leaves the last result in place.  Synchronises.  The result buffer belongs to the
 * map, grows on demand, stays valid until the next ws_map_ground on it and is apart from every other query's: neither invalidates
 * the other.  Read-only on the maps; calls that use the result buffer are serialised inside the library.  Nothing is allocated before
 * the first call; an allocation that fails returns WS_ERR_HIP and leaves the map usable. */
#define WS_GROUND_DEFAULT 0u
#define WS_GROUND_ANY_WEIGHT 1u
#define WS_GROUND_UNKNOWN_HEADROOM 2u
#define WS_GROUND_TOP 4u
#define WS_GROUND_CLASS_UNKNOWN 0u
#define WS_GROUND_CLASS_GROUND 1u
#define WS_GROUND_CLASS_BLOCKED 2u
#define WS_GROUND_CLASS_VOID 3u
int ws_map_ground(ws_map *map, int which, const int32_t lo[3], const int32_t hi[3], int32_t clear_vox, uint32_t flags, uint64_t counts[4]);
const void *ws_map_ground_dev(const ws_map *map, size_t *n); /* device memory, n 8-byte records; NULL before the first call (n == 0) */
/* copies at most `capacity` records (a prefix) and always reports the total in *n_out; host may be NULL */
int ws_map_ground_download(ws_map *map, void *host, size_t capacity, size_t *n_out);
/* the box of the last ground result: its first world voxel and its extent (ext[2] saturates at 2^32 - 1); either may be NULL.  No
 * ground result yet: WS_ERR_INVALID */
int ws_map_ground_box(ws_map *map, int32_t lo[3], uint32_t ext[3]);
/* Measurement entry, as ws_debug_distance_timing: ms_out receives the device time of pass 1 (levels) and pass 2 (steps) of the last call */
int ws_debug_ground_timing(ws_map *map, int32_t enable, float ms_out[2]);
/* The bridge to the planner: a ws_map_distance(..., WS_DISTANCE_COLUMNS) in every respect -- the same checks of max_dist_vox and of
 * the record counts, the same line passes, the map's distance result is REPLACED, and the box and flags it publishes let ws_map_reach
 * treat it as a column map -- except that pass 0 reads the records of the last ws_map_ground instead of the TSDF:
 *   FREE (1): a GROUND column with step <= max_step_q8 (1/256 voxel).  OCCUPIED (2), a site: BLOCKED, VOID, or GROUND above the step.
 *   UNKNOWN (0): a site iff WS_DISTANCE_UNKNOWN_OCCUPIED.
 *   flags: WS_DISTANCE_UNKNOWN_OCCUPIED is the one accepted bit (WS_DISTANCE_COLUMNS is implied, and is what the published flags
 *     hold); anything else is WS_ERR_INVALID.  No ground result yet: WS_ERR_INVALID.  max_step_q8 outside 0 .. 65535: WS_ERR_RANGE.
 * The box is that of the ground result (its z range is kept as the published box's).  A refusal launches nothing and leaves the last
 * distance result in place.  The ground result stays as it is. */
int ws_map_ground_distance(ws_map *map, int32_t max_step_q8, int32_t max_dist_vox, uint32_t flags, size_t *n_sites);

/* Frontier of a device map: where the known world ends.  The update writes observed free space explicitly (weight > 0, value = tau);
 * a voxel no ray reached keeps weight 0.  The frontier of a box is the set of its observed-free voxels that touch a never-observed
 * voxel of the box, and with WS_FRONTIER_CLUSTERS its connected patches with size, bounding box and coordinate sum -- a planner
 * consumes goals, not voxels.  Integers only; the same bytes on every run.
 *   box: inclusive world voxels [lo, hi] under the rules of ws_map_surface (both NULL: the whole window, each ring cell once; outside
 *     the window, hi < lo or more voxels than the ring holds along an axis: WS_ERR_INVALID).
 *   classes of a voxel, from its entry's two int16: VALID iff weight > 0; with WS_FRONTIER_ANY_WEIGHT iff weight != 0 (as
 *     WS_DISTANCE_ANY_WEIGHT).  FREE iff valid and value >= min_value.  UNKNOWN iff not valid.
 *   min_value: 0 means any non-negative value, the FREE of ws_map_distance; the map's tau keeps the frontier a truncation distance
 *     away from surfaces (only the free-space candidates carry value = tau).  min_value < 0 or > 32767: WS_ERR_RANGE.
 *   frontier voxel: a voxel v of the box that is FREE and has at least one of its six face neighbours INSIDE THE BOX UNKNOWN.  A
 *     neighbour outside the box is ignored: it is neither known nor unknown, and the rim of a box is not a frontier because of the
 *     rim.  As with ws_map_distance, the result of a box is NOT the restriction of a larger box's result to it.
 *   record, 16 bytes: int32 x, y, z in world voxels, then uint32 mask: bits 0..5 are set for an UNKNOWN neighbour at -x, +x, -y, +y,
 *     -z, +z, the other bits are 0.  Records come in ascending world (x, y, z), z fastest, the order of ws_map_surface.
 *   WS_FRONTIER_CLUSTERS adds two arrays.  Two frontier voxels are connected if they differ by at most 1 on every axis (the
 *     26-neighbourhood); a cluster is a connected component of the records OF THIS CALL.  Clusters are numbered 0 .. K - 1 by the
 *     record index of their first member, ascending: record 0 is in cluster 0.  labels: one uint32 per record, in record order, the
 *     number of its cluster.  cluster table, K rows of 64 bytes: uint32 first (record index of the first member), uint32 count,
 *     int32 lo[3], int32 hi[3] (the bounding box in world voxels), int64 sum[3] at offset 32 (the sum of the members' coordinates:
 *     |coordinate| < 2^31 and count < 2^31, it cannot overflow), 8 zero bytes.  With this flag more than 2^31 - 1 records is
 *     WS_ERR_RANGE and leaves an empty result.  No size filter runs on the device: the table is small, callers filter it.
 *   errors: unknown flag bits, bad `which`, exactly one NULL box pointer: WS_ERR_INVALID.  On a refusal nothing is launched and the
 *     last result stays.  Zero records is WS_OK with NULL device pointers.
 * Synchronises (*n_out and *n_clusters, either may be NULL, receive the numbers of records and of clusters; without the flag
 * *n_clusters = 0).  The buffers belong to the map, grow on demand and stay valid until the next ws_map_frontier on it; they are apart
 * from those of every other query, none of which invalidates this result.  Every output write is bounded by the buffers' capacities.
 * Read-only on the maps; calls that use the buffers are serialised inside the library.  Nothing is allocated before the first call;
 * an allocation that fails returns WS_ERR_HIP and leaves the map usable.
 * The implementation: the count / scan / emit compaction of ws_map_surface with a 7-point stencil, then a union-find over the sorted
 * records (neighbours by binary search, hooks by compare-and-swap of the larger root under the smaller, so the root of a component is
 * its smallest record index whatever the order of execution), an ordered scan of the roots and integer atomics for the table. */
#define WS_FRONTIER_DEFAULT 0u
#define WS_FRONTIER_ANY_WEIGHT 1u
#define WS_FRONTIER_CLUSTERS 2u
int ws_map_frontier(ws_map *map, int which, const int32_t lo[3], const int32_t hi[3], int32_t min_value, uint32_t flags, size_t *n_out, size_t *n_clusters);
const void *ws_map_frontier_records_dev(const ws_map *map, size_t *n);     /* device memory, n x 16 bytes; NULL when n == 0 */
const uint32_t *ws_map_frontier_labels_dev(const ws_map *map, size_t *n);  /* n uint32; NULL unless the last call asked for clusters */
const void *ws_map_frontier_clusters_dev(const ws_map *map, size_t *n);    /* n x 64 bytes; NULL unless the last call asked for them */
/* copies at most cap_records records (and labels) and cap_clusters rows (prefixes) and always reports the totals; any host pointer
 * may be NULL, and so may n_clusters.  Asking for labels or rows that the last call did not produce: WS_ERR_INVALID */
int ws_map_frontier_download(ws_map *map, void *records_host, uint32_t *labels_host, void *clusters_host, size_t cap_records, size_t cap_clusters, size_t *n_out,
                             size_t *n_clusters);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the count pass, the scan, the emit pass and the
 * clustering of the last call (the clustering spans one host read, of the number of clusters; 0 without WS_FRONTIER_CLUSTERS) */
int ws_debug_frontier_timing(ws_map *map, int32_t enable, float ms_out[4]);

/* Reach of a device map: the geodesic field.  Per record of the map's last distance result the cost of the cheapest path from a set of
 * seeds (the robot) that keeps a given clearance from the obstacles -- whether a frontier goal can be reached, how far it is along
 * free space, and by which way.  Integers only: the costs are exact and the same bytes on every run.
 *   input: the dense result of the LAST ws_map_distance on this map as it lies in device memory: its box (lo and extent), its
 *     `class | d2` records and whether it was made under WS_DISTANCE_COLUMNS.  No distance call yet: WS_ERR_INVALID.  The reach never
 *     reads the TSDF itself.
 *   traversable: a record is traversable iff its class is FREE (1) and d2 >= clear_d2; with WS_REACH_UNKNOWN_FREE (the optimistic
 *     planner) class UNKNOWN (0) counts as well.  0 <= clear_d2 <= 65025, else WS_ERR_RANGE.  Under WS_DISTANCE_UNKNOWN_OCCUPIED an
 *     unknown voxel is a site, d2 = 0: it is not traversable for any clear_d2 >= 1.
 *   steps: between two records that differ by at most 1 on every axis (the 26-neighbourhood of a volume, the 8-neighbourhood between
 *     columns), both traversable.  A face step weighs 10, an edge step 14, a corner step 17.  A neighbour outside the box does not
 *     exist, as with ws_map_frontier.  clear_d2 >= 2 keeps a diagonal step from passing between two face-adjacent sites, that
 *     is sites that are face neighbours of its ends: such an end has d2 = 1 and is not traversable.
 *   seeds: n_seeds world voxels (n x 3 int32 in host memory), 1 <= n_seeds <= 2^20; under WS_DISTANCE_COLUMNS z is ignored.  A seed
 *     outside the box or on a record that is not traversable is dropped; *n_seeded receives the number of seeds kept (a voxel given
 *     twice counts twice).  No seed kept is WS_OK with every cost unreachable, like a distance box without sites.
 *   field: one uint32 per record of the distance result, in its order: the minimum over all step sequences from any kept seed of
 *     the sum of the weights, 0xFFFFFFFF where there is none; a kept seed has 0.  More than (2^32 - 2) / 17 records: WS_ERR_RANGE
 *     (the cost could overflow).  The minimum defines the bytes; the implementation gets there another way and leaves them the same.
 *   *n_reached: the records with a finite cost.  *rounds: the relaxation rounds that ran (this number, unlike the costs, may differ
 *     between two runs).  Any of the three may be NULL.
 *   max_rounds: the cap on the rounds, 0 for the default of 64 x tiles of the box + 64.  A round settles at least every record whose
 *     cheapest path has that many steps, so records + 1 rounds always suffice -- which is 512 x tiles: the default is the TIGHTER of
 *     the two, and a legitimate labyrinth can hit it (a one-voxel corridor that crosses a tile face on nearly every step needs
 *     about one round per step).  A caller who expects such a map passes max_rounds, up to the number of records + 1.  At the cap
 *     with tiles still listed: WS_ERR_RANGE, "not converged" in ws_last_error; the call leaves NO result, the previous reach
 *     result is gone too, and ws_debug_reach_timing reads zeros.
 *   errors: unknown flag bits, NULL seeds, n_seeds = 0 or > 2^20, no distance result: WS_ERR_INVALID before anything is launched; the
 *     last reach result stays (also after a clear_d2 out of range).
 * The implementation (map_reach.hip): the box is cut into tiles of 512 records (8 x 8 x 8; 16 x 32 columns).  A round is one launch
 * with one workgroup per listed tile: it loads the tile and a halo of one record into LDS, relaxes there until nothing changes or 32
 * sweeps are used up, writes its own tile and lists for the next round every tile across whose face, edge or corner it lowered a
 * cost, and itself if it ran out of sweeps.  The host reads one word per round, the length of the next list.
 * Synchronises.  The result belongs to the map, is allocated on first use, and carries its own box: a later ws_map_distance does not
 * invalidate it, and it invalidates no other query's result.  An allocation that fails returns WS_ERR_HIP and leaves the map usable.
 * Calls that use the result are serialised inside the library. */
#define WS_REACH_DEFAULT 0u
#define WS_REACH_UNKNOWN_FREE 1u
#define WS_REACH_UNREACHABLE 0xFFFFFFFFu
int ws_map_reach(ws_map *map, const int32_t *seeds_host, size_t n_seeds, int32_t clear_d2, uint32_t flags, uint32_t max_rounds, size_t *n_seeded, size_t *n_reached,
                 uint32_t *rounds);
const uint32_t *ws_map_reach_dev(const ws_map *map, size_t *n); /* device memory, n costs; NULL when n == 0 */
/* copies at most `capacity` costs (a prefix) and always reports the total in *n_out; host may be NULL */
int ws_map_reach_download(ws_map *map, uint32_t *host, size_t capacity, size_t *n_out);
/* The box the last reach result carries: its first world voxel, its extent (nx, ny, nz; under columns nx, ny, 1) and whether it is a
 * column map; all zero without a result or without records.  Any pointer may be NULL. */
int ws_map_reach_box(ws_map *map, int32_t lo[3], uint32_t ext[3], int32_t *columns);
/* The costs of the last reach result at n world voxels: int32 triples, `stride` int32 words apart (3, or 4: the 16-byte records of
 * ws_map_frontier in device memory feed straight into the _dev form); under columns z is ignored.  A voxel outside the box of the
 * result: 0xFFFFFFFF.  n <= 2^27.  The first form takes and fills host memory, the _dev form device memory.  Both synchronise.  No
 * reach result, a stride other than 3 or 4, a NULL pointer with n > 0: WS_ERR_INVALID. */
int ws_map_reach_lookup(ws_map *map, const int32_t *points_host, size_t n, int32_t stride, uint32_t *cost_host);
int ws_map_reach_lookup_dev(ws_map *map, const int32_t *points_dev, size_t n, int32_t stride, uint32_t *cost_dev);
/* The paths of the last reach result from g goal voxels (g x 3 int32 in host memory, 1 <= g <= 2^20) back to a seed, one wave per goal.
 * The predecessor of a reached voxel v is the FIRST neighbour p in ascending (dx, dy, dz) order with cost[p] + w(p, v) == cost[v]; one
 * exists at every reached voxel that is no seed, the cost falls with every step, and the walk is bounded by cost / 10 steps besides.
 *   headers_host, g x 16 bytes: uint32 cost, steps (of the whole path), written (records of this goal), status: 0 reached, 1 not
 *     reachable, 2 outside the box (cost 0xFFFFFFFF, steps = written = 0 for both).
 *   records_host, g x cap_steps x 16 bytes, may be NULL when cap_steps = 0 (a pure cost query): int32 x, y, z, cost -- the goal first,
 *     the seed last (steps + 1 records); a longer path leaves its first cap_steps records and still reports its true steps.  Records
 *     beyond `written` are zero.  Under columns z is the goal's.  g x cap_steps <= 2^26, else WS_ERR_RANGE.  Synchronises. */
int ws_map_reach_paths(ws_map *map, const int32_t *goals_host, size_t g, uint32_t cap_steps, void *headers_host, void *records_host);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the seeding (clears, upload, seed pass), of all
 * rounds as one span (it includes the host's read per round) and of the count pass of the last ws_map_reach */
int ws_debug_reach_timing(ws_map *map, int32_t enable, float ms_out[3]);
/* Measurement entry: the number of tiles each round of the last ws_map_reach listed, in round order (at most `capacity` of them, a
 * prefix; *n_out receives the number of rounds; host may be NULL) */
int ws_debug_reach_active(ws_map *map, uint32_t *host, size_t capacity, size_t *n_out);
/* The constants of the implementation: out[0] the sweeps per round and tile, out[1..3] the tile of a volume along x, y, z, out[4..5]
 * the tile of a column map along x, y, out[6] the default rounds per tile, out[7] = 0 */
int ws_debug_reach_params(int32_t out[8]);

/* View gain of a device map: what the sensor would see from there.  For m candidate origins and one fan of n directions shared by all
 * of them, per view the UNKNOWN and the FREE samples its rays meet before an OCCUPIED voxel blocks them, as counts and weighted by k^2
 * -- the unknown volume a pose opens onto, for many poses in one launch.  Integers only: the same bytes on every run.  All products
 * are int64; "trunc" is C division, "floor" is floor division.
 *   box: inclusive world voxels [lo, hi] under the rules of ws_map_frontier (both NULL: the whole window, each ring cell once; exactly
 *     one NULL, outside the window, hi < lo or more voxels than the ring holds along an axis: WS_ERR_INVALID).
 *   classes of a voxel, the frontier's, from its entry's two int16: VALID iff weight > 0; with WS_GAIN_ANY_WEIGHT iff weight != 0.
 *     FREE iff valid and value >= min_value, OCCUPIED iff valid and value < min_value, UNKNOWN iff not valid.  min_value < 0 or
 *     > 32767: WS_ERR_RANGE.
 *   views: m origins o_j (int32 mm, map frame, m x 3 in host memory).  fan: n directions d_i (3 int32, n x 3 in host memory) under the
 *     rules of ws_map_raycast: any length; a ray with |component| >= 2^30 or L == 0 is DEAD.
 *   samples, exactly those of ws_map_raycast: step = max(res / 2, 1), K = max_range / step, L = floor(sqrt(dx^2 + dy^2 + dz^2)),
 *     p_k = o_j + trunc(d_i k step / L) per axis for k = 0 .. K; the voxel of a sample is v_k = floor(p_k / res) per axis (ONE entry:
 *     a class lookup, no interpolation).
 *   walk of (view j, ray i), k ascending: v_k outside the box counts for nothing and blocks nothing, the walk goes on (the ray may
 *     enter the box later).  v_k OCCUPIED: the ray is BLOCKED at k, this and all later samples count for nothing.  v_k UNKNOWN:
 *     unknown += 1, unknown_k2 += k^2.  v_k FREE: free += 1, free_k2 += k^2.  Unknown voxels do not block.
 *   k^2: the rays of a fan own disjoint solid angles, and a sample at range k step stands for a volume proportional to
 *     (k step)^2 step: unknown_k2 step^3 dOmega is the unknown volume the view would see, without counting a voxel near the origin
 *     once per ray.
 *   record per view, 32 bytes, in view order: uint64 unknown_k2, uint64 free_k2, uint32 unknown, uint32 free, uint32 blocked (rays
 *     that ended at an OCCUPIED voxel), uint32 live (rays that are not dead).
 *   WS_GAIN_RAYS adds m x n records of 8 bytes, view-major: uint32 unknown (the UNKNOWN samples of that ray), int32 stop (the k of the
 *     blocking sample, -1 for none, -2 for a dead ray).
 *   limits: max_range <= 0, m == 0 with a non-NULL best_unknown_k2, unknown flag bits, bad `which`, a NULL array with a non-zero
 *     count: WS_ERR_INVALID.  Otherwise n == 0 or m == 0: WS_OK, nothing written, the last result stays.  WS_ERR_RANGE: K > 8191,
 *     n > 2^19, m > 65535, m n > 2^27 under WS_GAIN_RAYS, res > 1024, |o| + max_range + 2 res does not fit int32 on an axis.  With
 *     these bounds no counter can overflow (the sum of k^2 of a ray is below 2^38, times 2^19 rays below 2^57).  On a refusal nothing
 *     is launched and the last result stays.
 * Synchronises (*best_unknown_k2, may be NULL, receives the largest unknown_k2 of the views).  The result buffers belong to the map,
 * grow on demand and stay valid until the next view-gain call on it; they are apart from those of every other query, none of which
 * invalidates this result.  Read-only on the maps; calls that use the buffers are serialised inside the library.  Nothing is allocated
 * before the first call; an allocation that fails returns WS_ERR_HIP and leaves the map usable.
 * The walk above defines the bytes; the implementation shortens it only where they stay the same: it keeps the class while the voxel
 * stays, and ends a ray once it has left the box for good.  map_gain.hip: L, the per-step quotient and remainder and the signs
 * depend on the direction alone and are prepared once per fan; then grid (ceil(n / 64), m), one lane per ray, the wave's lanes summed
 * across lanes (ballot and popcount for the ray counts) and one integer atomic add per wave and field into the view's record. */
#define WS_GAIN_DEFAULT 0u
#define WS_GAIN_ANY_WEIGHT 1u
#define WS_GAIN_RAYS 2u
int ws_map_view_gain(ws_map *map, int which, const int32_t lo[3], const int32_t hi[3], const int32_t *origins_host, size_t m, const int32_t *dirs_host, size_t n,
                     int32_t max_range_mm, int32_t min_value, uint32_t flags, uint64_t *best_unknown_k2);
const void *ws_map_view_gain_records_dev(const ws_map *map, size_t *n); /* device memory, n x 32 bytes; NULL when n == 0 */
const void *ws_map_view_gain_rays_dev(const ws_map *map, size_t *n);    /* n = views x rays records of 8 bytes; NULL unless the last call asked for them */
/* copies at most cap_views view records and cap_rays ray records (prefixes) and always reports the totals; either host pointer may be
 * NULL, and so may n_rays.  Asking for ray records that the last call did not produce: WS_ERR_INVALID */
int ws_map_view_gain_download(ws_map *map, void *records_host, void *rays_host, size_t cap_views, size_t cap_rays, size_t *n_views, size_t *n_rays);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the upload of origins and fan (with the clearing
 * of the records), of the fan preparation and the march (which holds the wave-level reduction), and of the pass over the records
 * that finds the maximum */
int ws_debug_view_gain_timing(ws_map *map, int32_t enable, float ms_out[3]);

/* Clearance of candidate trajectories: does a body keep clear of the obstacles along a motion?  For T trajectories of P poses each and a
 * body of K spheres, per trajectory the smallest margin between a sphere and the nearest obstacle, the first colliding pose, the counts
 * and a soft cost, and the index of the best trajectory -- the scoring step of a local planner (DWA, MPPI, lattice primitives) for a few
 * thousand rollouts in one launch.  Integers only: the same bytes on every run.  All products and sums are int64; "floor" is floor
 * division.
 *   input: the dense result of the LAST distance call on this map (ws_map_distance or ws_map_ground_distance) as it lies in device
 *     memory: its box (lo and extent), its `class | d2` records, whether it was made under WS_DISTANCE_COLUMNS, and its clamp
 *     R = max_dist_vox.  No distance result yet: WS_ERR_INVALID.  The TSDF is never read.
 *   resolution: res is the map's (ws_map_create), as for ws_map_sample; res > 1024: WS_ERR_RANGE.
 *   body: K spheres, 1 <= K <= 64, K x 4 int32 in host memory: off_mm[3], the centre in the body frame with |component| <= 2^20, and
 *     radius_mm in 0 .. 65535.
 *   poses: T x P records of 12 int32, trajectory-major: rot_q30[9], row-major, every entry in [-2^30, 2^30] (the convention of
 *     ws_fuse_pose; orthonormality is not required), then pos_mm[3] with |component| < 2^30.  1 <= P <= 65535, T <= 2^20,
 *     T P <= 2^21.  The device calls do not read the poses on the host and so do not check these two domains: the arithmetic below is
 *     int64 and, the body being checked (|off| <= 2^20: |sum| <= 3 * 2^51), total over all int32 values of a pose, and inside the domains every centre fits int32.
 *   sample (t, p, k): the centre c_a = pos_a + floor((sum_j rot[a][j] off_j + 2^29) / 2^30) on each axis a; its voxel v = floor(c / res)
 *     per axis.  Under columns z is ignored.  The sample is OUTSIDE when v lies outside the box of the distance result.  Otherwise, with
 *     class and d2 of the record at v: margin = isqrt(d2 res^2) - radius_k, isqrt the exact floor square root (its argument is below
 *     2^36).  HIT iff margin < 0.  UNKNOWN iff the class is 0 -- counted, nothing more; under WS_DISTANCE_UNKNOWN_OCCUPIED an unknown
 *     record is a site, d2 = 0, so it is a HIT as well.  penalty = max(0, soft_mm - margin)^2, soft_mm in 0 .. 65535.
 *   The distance is between voxel CENTRES: the obstacle's surface may be up to half a voxel diagonal nearer than the records say, and the
 *     sphere's centre up to half a diagonal from its voxel's centre.  A caller who must not touch pads the radii by res sqrt(3) (by
 *     res sqrt(2) under columns).
 *   R res < max radius + soft_mm: WS_ERR_RANGE -- the clamp of d2 at R^2 could hide a penalty.
 *   record per trajectory, 32 bytes, in trajectory order, all fields over the samples of the trajectory that are not OUTSIDE:
 *     int32 min_margin (INT32_MAX without such a sample), int32 first_hit (the smallest pose index with a HIT, -1 for none),
 *     uint32 argmin (p * 64 + k of the first sample in (p, k) order that attains min_margin, 0xFFFFFFFF for none), uint32 hits,
 *     uint32 outside (the OUTSIDE samples), uint32 unknown, uint64 cost (the sum of the penalties).
 *   WS_CLEARANCE_POSES adds T x P records of 8 bytes, trajectory-major: int32 the smallest margin of the pose (INT32_MAX for none),
 *     uint16 hits, uint16 outside.
 *   *best (int64, may be NULL): the index of the trajectory with no hit and no outside sample whose (cost, index) is smallest, -1 when
 *     there is none.  With WS_CLEARANCE_OUTSIDE_OK outside samples do not disqualify.  It is found on the device in a last pass.
 *   limits: unknown flag bits, a NULL array with a non-zero count: WS_ERR_INVALID.  K, P, T, T P, soft_mm, an offset or a radius out of
 *     range: WS_ERR_RANGE.  With these limits no counter or cost can overflow (2^22 samples times a penalty below 2^34).  T == 0 (behind
 *     those checks of the arguments, in front of the look at the distance result: it is WS_OK without one, and whatever its R): WS_OK,
 *     nothing is written, the last result stays, *best is left alone.  Every refusal comes before the first launch
 *     and leaves the last result in place.
 * Synchronises.  The result buffers belong to the map, grow on demand and stay valid until the next clearance call on it; they are apart
 * from those of every other query, none of which invalidates this result.  Read-only on the maps and on the distance result; calls are
 * serialised inside the library.  Nothing is allocated before the first call; an allocation that fails returns WS_ERR_HIP and leaves
 * the map usable.
 * The implementation (map_clearance.hip): one workgroup of 256 lanes per trajectory, the body in LDS; G, the power of two >= K,
 * consecutive lanes take one pose, lane k sphere k, and the groups stride over the poses; a lane rotates its own offset and gathers one
 * record.  The wave folds a biased 64-bit (margin, index) key by min, first_hit by min, counts and cost by adds, the four waves meet in
 * LDS, one record store per trajectory: no atomics and nothing to clear.  The float in isqrt is an estimate that two integer loops
 * correct; no result depends on it. */
#define WS_CLEARANCE_DEFAULT 0u
#define WS_CLEARANCE_POSES 1u
#define WS_CLEARANCE_OUTSIDE_OK 2u
int ws_map_clearance(ws_map *map, const int32_t *poses_host, size_t n_traj, size_t n_poses, const int32_t *body_host, size_t k, int32_t soft_mm, uint32_t flags,
                     int64_t *best);
/* the same with the poses already in device memory (the body stays a host array) */
int ws_map_clearance_dev(ws_map *map, const int32_t *poses_dev, size_t n_traj, size_t n_poses, const int32_t *body_host, size_t k, int32_t soft_mm, uint32_t flags,
                         int64_t *best);
const void *ws_map_clearance_records_dev(const ws_map *map, size_t *n); /* device memory, n x 32 bytes; NULL when n == 0 */
const void *ws_map_clearance_poses_dev(const ws_map *map, size_t *n);   /* n = T x P records of 8 bytes; NULL unless the last call asked for them */
/* copies at most cap_traj trajectory records and cap_poses pose records (prefixes) and always reports the totals; either host pointer
 * may be NULL, and so may n_poses.  Asking for pose records that the last call did not produce: WS_ERR_INVALID */
int ws_map_clearance_download(ws_map *map, void *records_host, void *poses_host, size_t cap_traj, size_t cap_poses, size_t *n_traj, size_t *n_poses);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the upload of body and poses, of the trajectory
 * pass, and of the pass over the records that finds the best */
int ws_debug_clearance_timing(ws_map *map, int32_t enable, float ms_out[3]);
/* ws_clearance_centres, ws_clearance_margin: host only, no GPU and no context -- the CPU statement of the two rules above, for tools and
 * tests.  ws_clearance_centres writes the voxel (3 int32) of every sample of n_poses poses (12 int32 each) and a body of k spheres,
 * n_poses x k x 3, pose-major; it checks k, res (1 .. 1024), the body and here also the domains of the poses (WS_ERR_RANGE).
 * ws_clearance_margin returns isqrt(d2 res^2) - radius_mm; arguments outside d2 <= 65025, 1 <= res <= 1024, 0 <= radius_mm <= 65535
 * are clamped to these ranges. */
int ws_clearance_centres(const int32_t *poses, size_t n_poses, const int32_t *body, size_t k, int32_t res, int32_t *voxels_out);
int32_t ws_clearance_margin(uint32_t d2, int32_t res, int32_t radius_mm);

/* ------------------------------------------------------------------ the global map in device memory ---- */
/* ws_store: the device twin of HDF5GlobalMap (src/map/hdf5_global_map.cpp) -- a pool of 64^3-voxel chunks in HBM, so that a map shift
 * is a device-to-device copy in stream order: the leaving slabs, the window move and the entering slabs with revisits and corners,
 * without a PCIe transfer, pinned staging or a worker thread.  The host global map and its file are written from the store when the
 * caller asks (ws_store_get_chunk per key of ws_store_keys).
 *   chunk: 262 144 uint32, index x * 4096 + y * 64 + z (hdf5_global_map.cpp:53-57); its key is floor(world voxel / 64) per axis, for
 *     negative coordinates too.  A chunk the store has never seen holds `fill_entry` everywhere.
 *   directory: key -> slot lives on the HOST and slots are handed out before anything is launched: which chunks exist, and every
 *     byte of them, is the same on every run, and a call that cannot get its chunks is refused before it changes anything.
 *   pool: grows in segments of `segment_chunks` chunks (0: 256; rounded up to a power of two).  Growing never copies or moves a chunk,
 *     so ws_store_chunk_dev pointers stay valid until the chunk is dropped.  max_chunks: 0 = no limit but the device's memory.
 *   boxes: inclusive world voxels of the window of `map` under the rule of ws_map_extract_box (even sizes included; otherwise
 *     WS_ERR_INVALID and nothing moves; a window that does not lie in int32: WS_ERR_RANGE, likewise).
 *   ws_store_save_box: LocalMap._area(save) on the device.  Every chunk the box overlaps exists afterwards (HDF5GlobalMap's
 *     activate_chunk); a chunk this call creates holds fill_entry wherever the box does not cover it; an existing chunk keeps its
 *     voxels outside the box.
 *   ws_store_load_box: voxels of present chunks are copied into the ring, voxels of absent chunks become fill_entry, and NO chunk
 *     is created (the bytes of ws_map_insert_box after a plain fill).  Loading into WS_MAP_NEW clears the map's "new_map is default".
 *   ws_shift_device: HDF5LocalMap::shift (hdf5_local_map.cpp:53-118) wholly on the device -- per axis x, y, z the leaving slab is
 *     saved, pos / offset of BOTH maps move, the entering slab is loaded.  The slabs are those of ws_shift_plan.  A pending scan is
 *     settled first.  WS_ERR_INVALID, nothing changed: a ws_shift_begin ticket is open, new_map holds entries that have not been
 *     integrated, a step larger than the window, a store of another context.  WS_ERR_RANGE, nothing changed: a window of the plan
 *     does not lie in int32 (ws_shift_plan).  new_pos == pos: WS_OK, nothing happens.  The
 *     parameters of both maps are committed only after every launch is enqueued.
 *   planning before launching: the new chunks of ALL axes of a call are counted before its first launch.  If they do not fit under
 *     max_chunks: WS_ERR_CAPACITY; if a segment cannot be allocated: WS_ERR_HIP; both maps and the store stay as they were.  Only
 *     these planning failures (and the WS_ERR_INVALID refusals) are free of side effects: a HIP error while the launches are being
 *     enqueued takes the chunks the call created out of the directory again and leaves the maps' parameters as they were, but
 *     launches already enqueued still run and may have overwritten existing chunks and parts of the ring.
 *   no waiting: save_box, load_box and the shift are stream-ordered on the context's stream and return after enqueueing.  They wait
 *     for the device only where a segment has to be allocated (ws_store_reserve does that up front), or where a box overlaps more
 *     than 8192 chunks (a whole 1025^3 window overlaps 4913): its slot table grows inside the call.  The slot tables of a call --
 *     dense over the chunk range of its box, one word per chunk with a "new chunk" bit -- travel through a ring of eight pinned
 *     tables, allocated with the store, each guarded by an event behind the launch that read it.
 *   ws_store_get_chunk / _put_chunk synchronise.  ws_store_drop_chunk does not: the slot goes to whichever later call needs one,
 *     whose work is ordered behind everything enqueued so far.
 *   ws_store_keys: ascending (cx, cy, cz); copies at most `capacity` keys and always reports the count.
 *   threads: calls on one store are serialised by a mutex inside the library; a shift is a writer on the map, as in the reference
 *     (tsdf_mapping.cpp:114-124). */
typedef struct ws_store ws_store;
int ws_store_create(ws_context *ctx, uint32_t fill_entry, uint64_t max_chunks, uint32_t segment_chunks, ws_store **out);
int ws_store_destroy(ws_store *st);
int ws_store_reserve(ws_store *st, uint64_t chunks); /* segments for that many chunks now, so that no shift allocates */
int ws_store_count(const ws_store *st, uint64_t *chunks, uint64_t *capacity_chunks);
int ws_store_keys(const ws_store *st, int32_t *keys /* n x 3 */, size_t capacity, size_t *n_out);
int ws_store_has(const ws_store *st, const int32_t key[3]); /* 1 / 0 */
int ws_store_get_chunk(ws_store *st, const int32_t key[3], uint32_t *host /* 262144 */, int32_t *found); /* absent: found = 0, host untouched */
int ws_store_put_chunk(ws_store *st, const int32_t key[3], const uint32_t *host); /* create or overwrite */
int ws_store_drop_chunk(ws_store *st, const int32_t key[3]); /* absent: WS_ERR_INVALID */
const uint32_t *ws_store_chunk_dev(const ws_store *st, const int32_t key[3]); /* device memory, 262144 words; NULL if absent */
int ws_store_save_box(ws_store *st, ws_map *map, int which, const int32_t lo[3], const int32_t hi[3]);
int ws_store_load_box(ws_store *st, ws_map *map, int which, const int32_t lo[3], const int32_t hi[3]);
int ws_shift_device(ws_map *map, ws_store *st, const int32_t new_pos[3]);
/* host only: the chunk keys an inclusive world box overlaps, ascending (cx, cy, cz); at most `capacity` are copied, the count is
 * always reported.  hi < lo: WS_ERR_INVALID */
int ws_store_chunks_of_box(const int32_t lo[3], const int32_t hi[3], int32_t *keys, size_t capacity, size_t *n_out);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the save launches and of the load launches of the
 * last save_box / load_box / shift on the store (summed over the axes of a shift) */
int ws_debug_store_timing(ws_store *st, int32_t enable, float ms_out[2]);

/* The surface cloud of the store: ws_map_surface over the chunks of the global map, wherever they lie -- the point cloud of everything
 * mapped, including what the window has left -- on the device, without a chunk leaving HBM.
 *   field: that of ws_store_mesh: a voxel of a present chunk holds that chunk's entry.  A voxel of an absent chunk never qualifies,
 *     whatever fill_entry is.
 *   predicate, record and marker: word for word those of ws_map_surface.  A voxel qualifies iff weight > 0 && abs(value) < band (abs
 *     on the value as int32, so -32768 never qualifies); the 16-byte record is int32 x, y, z in world voxels, then uint32 raw; with
 *     WS_SURFACE_MARKER 7 float32 per record in a second array of the same order, (float)x * (float)map_resolution / 1000.f per axis,
 *     then r, g, b, a from value / (float)tau.  The store knows neither tau nor the resolution, the caller passes both: tau <= 0 or
 *     map_resolution <= 0 is WS_ERR_INVALID; band <= 0 means tau.  The flag values are WS_SURFACE_RECORDS and WS_SURFACE_MARKER;
 *     unknown flag bits: WS_ERR_INVALID.
 *   box: inclusive world voxels [lo, hi], anywhere in int32 voxel space; it need not lie in any window.  Extents are formed in 64 bits.
 *     Both NULL: every present chunk, i.e. the bounding box of the present chunks, as for ws_store_mesh.  Exactly one NULL, or
 *     hi < lo: WS_ERR_INVALID.  An empty store, or a box that meets no present chunk, is WS_OK with *n_out = 0.
 *   order: records in ascending world (x, y, z), z fastest -- over the whole box, across chunk borders.  Consequence: if a window
 *     holds the same voxels as the store inside a box, and tau and map_resolution are the map's, ws_map_surface on that window and box
 *     returns the same bytes, records and marker (what ws_store_load_box writes for an absent chunk must not qualify either: a
 *     fill_entry of weight 0).
 *   limits: a box that overlaps 2^19 present chunks or more (512 GB of voxels) is WS_ERR_RANGE.  On a refusal nothing is launched, and
 *     the last result stays.  Counts and offsets are 64-bit: there is no 2^32 record limit.  An allocation that fails is WS_ERR_HIP
 *     and leaves the store usable.
 *   ordering: the work is stream-ordered behind every save, load and shift already enqueued on the store's context; the call
 *     synchronises (the count comes back), is read-only on the chunks and is serialised with the other store calls by the store's
 *     mutex.
 *   result buffers: they belong to the store, are not allocated before the first call and grow on demand; they stay valid until
 *     the next ws_store_surface on the store -- later saves, loads, shifts and drops leave them untouched -- and are apart from
 *     those of ws_store_mesh, ws_store_raycast and ws_store_distance.  Every output write is bounded by the buffers' capacities.
 *   cost: scratch, tables and work follow the number of present chunks the box overlaps (4096 words of 64 voxels per chunk, 8 bytes
 *     of scratch per word plus 12 bytes per 256 words: 32 KB per chunk, plus 32 bytes of tables), never the volume of the box: three
 *     chunks a million voxels apart cost three chunks, and nothing is refused because the bounding box is large. */
int ws_store_surface(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t band, int32_t tau, int32_t map_resolution, uint32_t flags, size_t *n_out);
const void *ws_store_surface_records_dev(const ws_store *st, size_t *n); /* device memory, n x 16 bytes; NULL when n == 0 */
const float *ws_store_surface_marker_dev(const ws_store *st, size_t *n); /* device memory, n x 7 floats; NULL unless the last call asked for it */
/* copies at most capacity_points points (a prefix) and always reports the total in *n_out; either host pointer may be NULL */
int ws_store_surface_download(ws_store *st, void *records_host, float *marker_host, size_t capacity_points, size_t *n_out);
/* Measurement entry, as ws_debug_surface_timing: ms_out receives the device time of the count passes (the masks and their totals), the
 * scan and the emit pass of the last call */
int ws_debug_store_surface_timing(ws_store *st, int32_t enable, float ms_out[3]);

/* The mesh of the store: the surface nets of ws_map_mesh over the chunks of the global map, wherever they lie -- the mesh of the
 * whole run, not of the window -- on the device, without a chunk leaving HBM.
 *   field: a voxel of a present chunk holds that chunk's entry.  A voxel of an absent chunk is NOT VALID, whatever fill_entry is,
 *     and is not inside.  Everything else is word for word the rule set of ws_map_mesh applied to that field: valid / inside and
 *     WS_MESH_ANY_WEIGHT, cells, the crossing offset o, the vertex as the floor mean of its crossings, the weight word, the face
 *     orientation, the four-valid-cells condition of a quad, the 16-byte vertex record and the 12-byte face record.
 *   box: inclusive world voxels [lo, hi]; it need not lie in any window.  Both NULL: the bounding box of the present chunks,
 *     64 kmin .. 64 kmax + 63 per axis.  Exactly one NULL, or hi < lo: WS_ERR_INVALID.  Voxels outside the box are not valid; the
 *     cell range is lo .. hi - 1.  A box one voxel thick along an axis, an empty store and a box that meets no present chunk are
 *     WS_OK with zero vertices and zero faces.
 *   order: vertices by ascending cell (x, y, z), z fastest; faces by ascending owner voxel (x, y, z), z fastest, then axis 0, 1, 2,
 *     the two triangles of a quad adjacent -- over the whole box, across chunk borders.  Consequence: if a window holds the same
 *     voxels as the store inside a box, and fill_entry has weight 0 (so that what ws_store_load_box writes for an absent chunk is
 *     not valid either), ws_map_mesh on that window and box returns the same bytes.
 *   map_resolution: the store does not know the map's resolution, the caller passes it (mm per voxel); <= 0: WS_ERR_INVALID.
 *   WS_ERR_RANGE, as for ws_map_mesh: (|coordinate| + 1) res of a corner of the box does not fit int32 (with the default box this
 *     is decided on the bounding box), or more than 2^32 - 1 vertices; also a box that overlaps 2^19 present chunks or more (512 GB
 *     of voxels).  Nothing is launched then, and the last result stays.  Unknown flag bits: WS_ERR_INVALID.
 *   ordering: the work is stream-ordered behind every save, load and shift already enqueued on the store's context; the call
 *     synchronises (the two counts come back), is read-only on the chunks and is serialised with the other store calls by the
 *     store's mutex.
 *   result buffers: they belong to the store, grow on demand and are not allocated before the first call; they stay valid until
 *     the next ws_store_mesh on the store -- later saves, loads, shifts and drops leave them untouched -- and are destroyed with
 *     it.  Every output write is bounded by the buffers' capacities.
 *   cost: scratch and work follow the number of present chunks the box overlaps (4096 words of 64 voxels per chunk, 29 bytes of
 *     scratch per word: 119 KB per chunk, plus 140 bytes of tables), never the volume of the box: three chunks a million voxels
 *     apart cost three chunks, and nothing is refused because the bounding box is large. */
int ws_store_mesh(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t map_resolution, uint32_t flags, size_t *n_vertices, size_t *n_faces);
const void *ws_store_mesh_vertices_dev(const ws_store *st, size_t *n);  /* device memory, n x 16 bytes; NULL when n == 0 */
const uint32_t *ws_store_mesh_faces_dev(const ws_store *st, size_t *n); /* device memory, n x 3 uint32; NULL when n == 0 */
/* copies at most cap_vertices vertices and cap_faces faces (prefixes) and always reports the totals; either host pointer may be NULL */
int ws_store_mesh_download(ws_store *st, void *vertices_host, uint32_t *faces_host, size_t cap_vertices, size_t cap_faces, size_t *n_vertices, size_t *n_faces);
/* Measurement entry, as ws_debug_mesh_timing: ms_out receives the device time of the count passes, the scan and the emit passes */
int ws_debug_store_mesh_timing(ws_store *st, int32_t enable, float ms_out[3]);

/* The ray cast of the store: ws_map_raycast over the chunks of the global map, wherever they lie -- the predicted scan, or the residual
 * of a scan, from ANY pose of the run, not only from inside the window -- on the device, without a chunk leaving HBM.
 *   rules: word for word those of ws_map_raycast -- samples, L and step; T as the trilinear interpolant times res^3; the hit
 *     condition, the range t and the hit point; the 16-byte record and the gradient; WS_RAYCAST_ANY_WEIGHT, _GRADIENT and _TARGETS; the
 *     dead rays -- applied to the field of ws_store_mesh: a voxel of a present chunk holds that chunk's entry; a voxel of an absent
 *     chunk is NOT VALID, whatever fill_entry is.
 *   box: inclusive world voxels [lo, hi]; it need not lie in any window.  Both NULL: everything.  Exactly one NULL, or hi < lo:
 *     WS_ERR_INVALID.  Voxels outside the box are not valid; a cell is valid iff all 8 of its voxels are valid.
 *   map_resolution: the store does not know the map's resolution, the caller passes it (mm per voxel); <= 0: WS_ERR_INVALID,
 *     > 1024: WS_ERR_RANGE.
 *   errors, as for ws_map_raycast: max_range <= 0 and unknown flag bits are WS_ERR_INVALID; |o| + max_range + 2 res does not fit
 *     int32 on an axis, or n > 2^27: WS_ERR_RANGE; also WS_ERR_RANGE if the call lists 2^19 present chunks or more (those the box
 *     overlaps; all of them without a box).  On a refusal nothing is launched, and the last result stays.  n == 0: WS_OK, nothing
 *     written.  An empty store, or a box that meets no present chunk: WS_OK, every record a no-hit.
 *   consequence: if a window holds the same voxels as the store inside a box, the box is that window, and fill_entry has weight 0
 *     (so that what ws_store_load_box writes for an absent chunk is not valid either), ws_map_raycast on that window returns the
 *     same bytes, records and gradient.
 *   ordering: the work is stream-ordered behind every save, load and shift already enqueued on the store's context; the call
 *     synchronises (*n_hits, may be NULL, comes back), is read-only on the chunks and is serialised with the other store calls by the
 *     store's mutex.
 *   result buffers: they belong to the store, are not allocated before the first call and grow on demand; they stay valid until
 *     the next ws_store_raycast on the store -- later saves, loads, shifts and drops leave them untouched -- and are apart from
 *     those of ws_store_mesh.  Every output write is bounded by the buffers' capacities.
 *   cost: the host lists the present chunks the box overlaps and writes a lookup key -> slot of 32 to 64 bytes per listed chunk,
 *     never anything that follows the volume of the box.  A ray does not sample absent chunks or the space outside the box: it
 *     goes from the sample at which it enters one straight to the first sample behind it, which leaves the records as they are.
 * ws_store_raycast_dev takes an array that is already in device memory (it must stay untouched until the call returns). */
int ws_store_raycast(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin_mm[3], const int32_t *dirs_host, size_t n, int32_t max_range_mm,
                     int32_t map_resolution, uint32_t flags, size_t *n_hits);
int ws_store_raycast_dev(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t origin_mm[3], const int32_t *dirs_dev, size_t n, int32_t max_range_mm,
                         int32_t map_resolution, uint32_t flags, size_t *n_hits);
const void *ws_store_raycast_records_dev(const ws_store *st, size_t *n);     /* device memory, n x 16 bytes; NULL when n == 0 */
const int32_t *ws_store_raycast_gradient_dev(const ws_store *st, size_t *n); /* n x 3 int32; NULL unless the last call asked for it */
/* copies at most capacity_rays records (and gradients: a prefix) and always reports the number of rays; either host pointer may be NULL */
int ws_store_raycast_download(ws_store *st, void *records_host, int32_t *gradient_host, size_t capacity_rays, size_t *n_out);
/* The point sample of the store: ws_map_sample over the chunks of the global map, wherever they lie.
 *   rules: word for word those of ws_map_sample -- the cell, T, the 16-byte record, the classes, the gradient at g, the selection, the
 *     flags.  The field is that of ws_store_raycast: a voxel of an absent chunk is not valid whatever fill_entry is; voxels outside
 *     [lo, hi] are not valid; both lo and hi NULL means everything; exactly one of them NULL, or hi < lo, is WS_ERR_INVALID.  `raw` is
 *     given whenever g lies in a present chunk and inside the box, else 0.
 *   band_mm <= 0 is WS_ERR_INVALID (the store does not know a tau), and so is map_resolution <= 0.  WS_ERR_RANGE: res > 1024,
 *     n > 2^27, or the call lists 2^19 present chunks or more.  On a refusal nothing is launched and the last result stays.
 *   consequence, as for the ray cast: if a window holds the same voxels as the store inside a box, the box is that window, and
 *     fill_entry has weight 0, then ws_map_sample and ws_store_sample return the same bytes in all three arrays.  (One word is excepted,
 *     by the rule of `raw` above: where g lies in an absent chunk the store gives 0 and the window gives what ws_store_load_box wrote
 *     there, fill_entry.)
 *   The buffers belong to the store, grow on demand, stay valid until the next ws_store_sample on it -- later saves, loads, shifts and
 *     drops leave them untouched -- and are apart from those of the other queries; the store's lock serialises the calls. */
int ws_store_sample(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *points_host, size_t n, int32_t band_mm, int32_t map_resolution,
                    uint32_t flags, uint64_t counts[4]);
int ws_store_sample_dev(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *points_dev, size_t n, int32_t band_mm, int32_t map_resolution,
                        uint32_t flags, uint64_t counts[4]);
const void *ws_store_sample_records_dev(const ws_store *st, size_t *n);     /* device memory, n x 16 bytes; NULL when n == 0 */
const int32_t *ws_store_sample_gradient_dev(const ws_store *st, size_t *n); /* n x 3 int32; NULL unless the last call asked for it */
const int32_t *ws_store_sample_selected_dev(const ws_store *st, size_t *n); /* n_selected x 3 int32; NULL unless asked for, or empty */
int ws_store_sample_download(ws_store *st, void *records_host, int32_t *gradient_host, int32_t *selected_host, size_t capacity_points, size_t capacity_selected,
                             size_t *n_out, size_t *n_selected);
int ws_debug_store_sample_timing(ws_store *st, int32_t enable, float ms_out[3]);
/* Measurement entry, as ws_debug_raycast_timing: ms_out receives the device time of the upload (the chunk lookup and, for the host
 * form, the directions), of the march and of the gradient pass of the last call */
int ws_debug_store_raycast_timing(ws_store *st, int32_t enable, float ms_out[3]);
/* Host only, for tests: the chunk lookup the kernels of ws_store_raycast read.  keys_slots: n x {cx, cy, cz, slot} with distinct keys,
 * n < 2^19; *n_places receives the table's size in 16-byte places, the power of two >= max(2, 2 n); table (may be NULL) receives
 * them if capacity_places allows.  _find returns the slot of `key` by the kernels' own probe, 0xffffffff if the table does not list it. */
int ws_debug_store_raycast_table(const int32_t *keys_slots, size_t n, int32_t *table, size_t capacity_places, size_t *n_places);
uint32_t ws_debug_store_raycast_find(const int32_t *table, size_t n_places, const int32_t key[3]);

/* The distance field of the store: ws_map_distance applied to the field of ws_store_mesh -- the cost map of the whole run, not of the
 * window around the sensor: a goal, a frontier or a return path lies exactly where the window no longer is -- on the device, without
 * a chunk leaving HBM.
 *   field: a voxel of a present chunk holds that chunk's entry.  A voxel of an absent chunk is NOT VALID (class 0, UNKNOWN), whatever
 *     fill_entry is: under WS_DISTANCE_UNKNOWN_OCCUPIED such a voxel is therefore a site, and it counts in *n_sites.
 *   rules: everything else is word for word the rule set of ws_map_distance applied to that field -- the classes and
 *     WS_DISTANCE_ANY_WEIGHT; the sites, which lie inside the box only; 1 <= R <= 255, else WS_ERR_RANGE;
 *     d2 = min(R², min over sites |v - s|²); the record (bits 0..23 d2, bits 30..31 the class); the dense order, x major, z fastest;
 *     WS_DISTANCE_COLUMNS with its nx ny records, y fastest; the four flag values.  Under WS_DISTANCE_COLUMNS the precedence of a
 *     column is part of the rules: occupied wins, then unknown-as-site, then free; an absent chunk contributes unknown voxels.
 *   box: inclusive world voxels [lo, hi], anywhere in int32 voxel space; it need not lie in any window.  Extents are formed in 64 bits.
 *     Both NULL: the bounding box of the present chunks, as for ws_store_mesh; an empty store with a NULL box is WS_OK with zero
 *     records and zero sites.  Exactly one NULL, or hi < lo: WS_ERR_INVALID.
 *   limits: more than 2^32 - 1 records (nx ny nz, or nx ny under WS_DISTANCE_COLUMNS, whose z extent is bounded only by int32) is
 *     WS_ERR_RANGE, and so is a box that overlaps 2^19 present chunks or more.  Also WS_ERR_RANGE: more than 16 776 960 voxels along
 *     the fastest axis of the records (nz, or ny under WS_DISTANCE_COLUMNS): the row pass holds a line in 65 535 workgroups.  Unknown
 *     flag bits: WS_ERR_INVALID.  On a refusal nothing is launched and the last result stays.  An allocation that fails is
 *     WS_ERR_HIP and leaves the store usable.
 *   consequence: if a window holds the same voxels as the store inside a box, the box lies in that window, and fill_entry has weight 0
 *     (so that what ws_store_load_box writes for an absent chunk is not valid either), ws_map_distance on that window and box returns
 *     the same bytes and the same site count, under every flag combination.
 *   ordering: the work is stream-ordered behind every save, load and shift already enqueued on the store's context; the call
 *     synchronises (*n_sites, may be NULL, comes back), is read-only on the chunks and is serialised with the other store calls by the
 *     store's mutex.
 *   result buffer: it belongs to the store, is not allocated before the first call and grows on demand; it stays valid until the next
 *     ws_store_distance on the store -- later saves, loads, shifts and drops leave it untouched -- and is apart from the results of
 *     ws_store_mesh and ws_store_raycast.  Every output write is bounded by the buffers' capacities.
 *   cost: unlike the store's mesh and ray cast, this result is DENSE.  Scratch and result are 8 bytes per record of the box, and the
 *     line passes follow the box.  Only pass 0 follows the present chunks: absent chunks are never read, and under
 *     WS_DISTANCE_COLUMNS a column is walked only across the z range of the listed chunks.  The chunk table is 32 to 64 bytes per
 *     listed chunk and never follows the volume of the box. */
int ws_store_distance(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t max_dist_vox, uint32_t flags, size_t *n_sites);
const uint32_t *ws_store_distance_dev(const ws_store *st, size_t *n); /* device memory, n records; NULL before the first call (n == 0) */
/* copies at most `capacity` records (a prefix) and always reports the total in *n_out; host may be NULL */
int ws_store_distance_download(ws_store *st, uint32_t *host, size_t capacity, size_t *n_out);
/* Measurement entry, as ws_debug_distance_timing: ms_out receives the device time of pass 0 (the classification; the chunk table's
 * upload lies in front of it) and of the x, y and z line passes of the last call (under WS_DISTANCE_COLUMNS: pass 0, the x pass, the
 * y pass, 0) */
int ws_debug_store_distance_timing(ws_store *st, int32_t enable, float ms_out[4]);

/* The ground of the store: ws_map_ground applied to the field of ws_store_distance -- the elevation layer of the whole run -- on the
 * device, without a chunk leaving HBM.
 *   field: a voxel of a present chunk holds that chunk's entry; a voxel of an absent chunk is UNKNOWN, whatever fill_entry is.
 *   rules: everything else is word for word the rule set of ws_map_ground applied to that field: the classes and
 *     WS_GROUND_ANY_WEIGHT, 1 <= clear_vox <= 64 (else WS_ERR_RANGE), the level and WS_GROUND_UNKNOWN_HEADROOM (under which the unknown
 *     voxels of an absent chunk inside the box are headroom), the lowest level or WS_GROUND_TOP, height, column class, step, the
 *     8-byte record, the column order and counts[4].
 *   box: the box rules of ws_store_distance: inclusive world voxels [lo, hi] anywhere in int32 voxel space, extents formed in 64 bits;
 *     both NULL: the bounding box of the present chunks, and an empty store is WS_OK with zero records; exactly one NULL, or hi < lo:
 *     WS_ERR_INVALID.  A box over no present chunk: every column UNKNOWN.
 *   limits: more than 2^32 - 1 columns is WS_ERR_RANGE (the z extent is bounded only by int32), and so is a box that overlaps 2^19
 *     present chunks or more.  Unknown flag bits: WS_ERR_INVALID.  Every refusal comes before the first launch and leaves the last
 *     result in place.  An allocation that fails is WS_ERR_HIP and leaves the store usable.
 *   consequence: if a window holds the same voxels as the store inside a box, the box lies in that window, and fill_entry has weight
 *     0, ws_map_ground on that window and box returns the same bytes and the same counts, under every flag combination.
 *   ordering and result buffer: as for ws_store_distance; the result is apart from every other query's of the store.
 *   cost: 16 bytes per column of the box for the result and the scratch of pass 2.  Pass 1 follows the present chunks: absent chunks
 *     are never read and a column is walked only across the z range of the listed chunks. */
int ws_store_ground(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t clear_vox, uint32_t flags, uint64_t counts[4]);
const void *ws_store_ground_dev(const ws_store *st, size_t *n); /* device memory, n 8-byte records; NULL before the first call (n == 0) */
int ws_store_ground_download(ws_store *st, void *host, size_t capacity, size_t *n_out); /* as ws_map_ground_download */
int ws_store_ground_box(ws_store *st, int32_t lo[3], uint32_t ext[3]);                  /* as ws_map_ground_box */
/* Measurement entry, as ws_debug_ground_timing (the chunk table's upload lies in front of pass 1) */
int ws_debug_store_ground_timing(ws_store *st, int32_t enable, float ms_out[2]);
/* ws_map_ground_distance over the last ws_store_ground result of this store, word for word: it replaces the store's distance result,
 * which ws_store_reach then treats as a column map */
int ws_store_ground_distance(ws_store *st, int32_t max_step_q8, int32_t max_dist_vox, uint32_t flags, size_t *n_sites);

/* The frontier of the store: ws_map_frontier over the chunks of the global map, wherever they lie -- what the whole run has not
 * covered yet, not what the window has not -- on the device, without a chunk leaving HBM.
 *   field: a voxel of a present chunk holds that chunk's entry.  A voxel of an absent chunk inside the box is UNKNOWN whatever
 *     fill_entry is, as in ws_store_distance; it is never FREE.
 *   rules: everything else is word for word the rule set of ws_map_frontier applied to that field: the classes and
 *     WS_FRONTIER_ANY_WEIGHT, min_value (a raw value: the store needs neither tau nor the resolution), the frontier voxel with its
 *     neighbours inside the box only, the record, the order across chunk borders, WS_FRONTIER_CLUSTERS with labels, numbering, table
 *     and the 2^31 - 1 limit.
 *   box: the rules of ws_store_surface: inclusive world voxels [lo, hi] anywhere in int32, both NULL: the bounding box of the present
 *     chunks; exactly one NULL or hi < lo: WS_ERR_INVALID; 2^19 or more present chunks in the box: WS_ERR_RANGE.  The faces of the
 *     bounding box are the rim of the box and therefore no frontier: a caller who wants the outer faces of the mapped volume as
 *     frontier passes a box ONE VOXEL LARGER than the bounding box on every side (the voxels of that shell lie in absent chunks or
 *     hold whatever the chunks hold).  An empty store, or a box that meets no present chunk, is WS_OK with zero records.
 *   consequence: if a window holds the same voxels as the store inside a box, ws_map_frontier on that window and box returns the same
 *     bytes: records, labels and table.  What ws_store_load_box writes for an absent chunk must be UNKNOWN as well: a fill_entry of
 *     weight 0.
 *   errors, ordering, result buffers: those of ws_store_surface.  On a refusal nothing is launched and the last result stays; the
 *     call synchronises; the buffers belong to the store, stay valid until the next ws_store_frontier and are apart from those of
 *     every other query.  Every output write is bounded by the buffers' capacities.
 *   cost: scratch, tables and work of the extraction follow the number of present chunks the box overlaps (32 KB of scratch and 56
 *     bytes of tables per chunk), never the volume of the box; the clustering follows the records (8 bytes each). */
int ws_store_frontier(ws_store *st, const int32_t lo[3], const int32_t hi[3], int32_t min_value, uint32_t flags, size_t *n_out, size_t *n_clusters);
const void *ws_store_frontier_records_dev(const ws_store *st, size_t *n);    /* device memory, n x 16 bytes; NULL when n == 0 */
const uint32_t *ws_store_frontier_labels_dev(const ws_store *st, size_t *n); /* n uint32; NULL unless the last call asked for clusters */
const void *ws_store_frontier_clusters_dev(const ws_store *st, size_t *n);   /* n x 64 bytes; NULL unless the last call asked for them */
/* as ws_map_frontier_download */
int ws_store_frontier_download(ws_store *st, void *records_host, uint32_t *labels_host, void *clusters_host, size_t cap_records, size_t cap_clusters, size_t *n_out,
                               size_t *n_clusters);
/* Measurement entry, as ws_debug_frontier_timing (the chunk tables' upload lies in front of the count pass) */
int ws_debug_store_frontier_timing(ws_store *st, int32_t enable, float ms_out[4]);

/* The reach of the store: ws_map_reach over the last ws_store_distance result of this store, word for word -- the same rules, the same
 * kernels, the same limits and refusals.  A voxel of an absent chunk is UNKNOWN in that result: blocked by default, passable under
 * WS_REACH_UNKNOWN_FREE (unless the distance call ran under WS_DISTANCE_UNKNOWN_OCCUPIED and clear_d2 >= 1).  A distance result
 * without records (an empty store asked without a box) gives a reach result without records: WS_OK, every lookup 0xFFFFFFFF.
 *   consequence: if a window holds the same voxels as the store inside a box, ws_map_reach behind ws_map_distance on that window and
 *     box returns the same bytes -- costs, lookups and paths.
 * The result belongs to the store, carries its own box and is apart from every other query's; later saves, loads, shifts, drops and
 * distance calls leave it untouched. */
int ws_store_reach(ws_store *st, const int32_t *seeds_host, size_t n_seeds, int32_t clear_d2, uint32_t flags, uint32_t max_rounds, size_t *n_seeded, size_t *n_reached,
                   uint32_t *rounds);
const uint32_t *ws_store_reach_dev(const ws_store *st, size_t *n); /* device memory, n costs; NULL when n == 0 */
int ws_store_reach_download(ws_store *st, uint32_t *host, size_t capacity, size_t *n_out);
int ws_store_reach_box(ws_store *st, int32_t lo[3], uint32_t ext[3], int32_t *columns);
int ws_store_reach_lookup(ws_store *st, const int32_t *points_host, size_t n, int32_t stride, uint32_t *cost_host);
int ws_store_reach_lookup_dev(ws_store *st, const int32_t *points_dev, size_t n, int32_t stride, uint32_t *cost_dev);
int ws_store_reach_paths(ws_store *st, const int32_t *goals_host, size_t g, uint32_t cap_steps, void *headers_host, void *records_host);
int ws_debug_store_reach_timing(ws_store *st, int32_t enable, float ms_out[3]);

/* The view gain of the store: ws_map_view_gain over the chunks of the global map, wherever they lie.
 *   field: a voxel of the box in an absent chunk is UNKNOWN: it counts, and it blocks nothing.
 *   box: as for ws_store_frontier: inclusive world voxels; both NULL: the bounding box of the present chunks (an empty store: an empty
 *     box, every sample is outside it); exactly one NULL or hi < lo: WS_ERR_INVALID; 2^19 or more present chunks in the box:
 *     WS_ERR_RANGE.
 *   map_resolution: the store does not know the map's resolution, the caller passes it (mm per voxel); <= 0: WS_ERR_INVALID.
 *   rules: everything else is word for word the rule set of ws_map_view_gain: classes, views, fan, samples, walk, records, flags,
 *     limits and refusals.
 *   consequence: if a window holds the same voxels as the store inside a box, ws_map_view_gain on that window and box returns the
 *     same bytes.
 * The result belongs to the store and is apart from every other query's; the call synchronises, and the store's lock serialises it. */
int ws_store_view_gain(ws_store *st, const int32_t lo[3], const int32_t hi[3], const int32_t *origins_host, size_t m, const int32_t *dirs_host, size_t n,
                       int32_t max_range_mm, int32_t map_resolution, int32_t min_value, uint32_t flags, uint64_t *best_unknown_k2);
const void *ws_store_view_gain_records_dev(const ws_store *st, size_t *n); /* device memory, n x 32 bytes; NULL when n == 0 */
const void *ws_store_view_gain_rays_dev(const ws_store *st, size_t *n);    /* n = views x rays records of 8 bytes; NULL unless the last call asked for them */
/* as ws_map_view_gain_download */
int ws_store_view_gain_download(ws_store *st, void *records_host, void *rays_host, size_t cap_views, size_t cap_rays, size_t *n_views, size_t *n_rays);
int ws_debug_store_view_gain_timing(ws_store *st, int32_t enable, float ms_out[3]);

/* The clearance of the store: ws_map_clearance over the last distance result of the store (ws_store_distance or
 * ws_store_ground_distance) -- the one host flow and the one kernel file of the window's call.
 *   map_resolution: mm per voxel, 1 .. 1024 (the store keeps none, as for ws_store_sample); <= 0: WS_ERR_INVALID, > 1024: WS_ERR_RANGE.
 *   rules: everything else is word for word the rule set of ws_map_clearance: input, body, poses, samples, margin, records, flags, *best,
 *     limits and errors.  The records of an absent chunk inside the box of the distance call are UNKNOWN and show as such.
 *   consequence: if a window's distance result and the store's hold the same box and records, the two calls return the same bytes.
 * Synchronises.  The result belongs to the store and is apart from every other query's. */
int ws_store_clearance(ws_store *st, const int32_t *poses_host, size_t n_traj, size_t n_poses, const int32_t *body_host, size_t k, int32_t soft_mm,
                       int32_t map_resolution, uint32_t flags, int64_t *best);
int ws_store_clearance_dev(ws_store *st, const int32_t *poses_dev, size_t n_traj, size_t n_poses, const int32_t *body_host, size_t k, int32_t soft_mm,
                           int32_t map_resolution, uint32_t flags, int64_t *best);
const void *ws_store_clearance_records_dev(const ws_store *st, size_t *n); /* device memory, n x 32 bytes; NULL when n == 0 */
const void *ws_store_clearance_poses_dev(const ws_store *st, size_t *n);   /* n = T x P records of 8 bytes; NULL unless the last call asked for them */
/* as ws_map_clearance_download */
int ws_store_clearance_download(ws_store *st, void *records_host, void *poses_host, size_t cap_traj, size_t cap_poses, size_t *n_traj, size_t *n_poses);
int ws_debug_store_clearance_timing(ws_store *st, int32_t enable, float ms_out[3]);

/* One store fused into another under a rigid pose: SRC is resampled on the voxel lattice of DST and integrated into it with the
 * weighted average of the TSDF update, on the device, without a chunk leaving HBM.  Two runs of one site, a map loaded from a file
 * and the map of the current run, or a submap that a registration has moved, become one map that keeps its TSDF.  The rule uses
 * integers only: products and sums are int64, "floor" is floor division, and the result is the same bytes on every run.
 *   pull transform: the map from the frame of DST to the frame of SRC, 15 int32: rot_q30[9] row-major, every entry in
 *     [-2^30, 2^30] (else WS_ERR_INVALID); pivot_dst_mm[3]; pivot_src_mm[3].
 *   voxel mapping: for the centre p = v res + h (h = res / 2 truncated) of the world voxel v of DST, axis k gets
 *     q_k = floor((sum_j rot[k][j] (p_j - pivot_dst_j) + 2^29) / 2^30) + pivot_src_k.  Orthonormality is not required of rot: the
 *     bytes follow from the matrix as given.  Every voxel with a component of |p - pivot_dst| >= 2^24 mm is outside the call and is
 *     never touched; with that limit no sum exceeds 2^56.  The voxels the call looks at are those of the candidate chunks of its plan
 *     (below), which for a rotation are all that can receive anything.
 *   sample: the cell of ws_store_sample at q in the field of SRC (base voxel floor((q - h) / res), fractions f, T): a voxel of an
 *     absent chunk is not valid, and a voxel is valid iff weight > 0 (there is no ANY_WEIGHT variant).  One change makes
 *     lattice-aligned poses exact: a corner whose trilinear coefficient is zero takes part neither in validity nor in the weight
 *     (with f_k = 0 on an axis only the low plane of that axis counts).  nv = floor(T / res^3); nw = the smallest weight among the
 *     corners that take part.  A point the sample calls dead (a component of q of magnitude >= 2^30) is not valid.
 *   integrate: wso_update_avg's rule (cu_avg_tsdf_krnl of the reference) on the entry (ev, ew) of DST; a voxel of an absent chunk of
 *     DST holds fill_entry.  Sample not valid: the voxel is untouched.  ew > 0: value (ev ew + nv nw) / (ew + nw) with C's truncating
 *     division, weight min(max_weight, ew + nw), both cast to int16.  Otherwise the entry becomes (nv, nw).
 *   chunks: a chunk of DST exists after the call iff it existed before or at least one of its voxels received a valid sample.  A
 *     chunk the call creates holds fill_entry wherever nothing was fused.
 *   stats[6]: candidate chunks of DST examined; chunks created; voxels averaged (ew > 0); voxels set (ew <= 0); over the averaged
 *     voxels the sum of |nv - ev|; over the averaged voxels the sum of min(nw, ew).  Integer adds, exact whatever the order.  The
 *     fifth divided by the third is the disagreement of the two maps under this pose, in mm.
 *   flags: WS_FUSE_DEFAULT; WS_FUSE_COUNT_ONLY: every statistic as the real call would report it, "chunks created" included, and no
 *     byte of DST and no entry of its directory changes (the chunk limit of DST is not looked at).  Unknown bits: WS_ERR_INVALID.
 *   refusals, nothing changed and nothing launched: WS_ERR_INVALID: a NULL argument, dst == src, stores of different contexts,
 *     max_weight outside 1 .. 32767, a fill_entry of DST with weight > 0, a rot_q30 entry out of range.  WS_ERR_RANGE: map_resolution
 *     < 1 or > 1024; 2^23 candidate chunks or more, or 2^19 chunks of SRC or more.  WS_ERR_CAPACITY: the chunks to create do not fit
 *     under max_chunks of DST; this is decided after the count pass and before any write.  WS_ERR_HIP: a segment cannot be allocated.
 *     An empty SRC is WS_OK with zero statistics.
 *   plan: the host maps the eight corners of every chunk of SRC, grown by two voxels, forward with the transpose of rot in double
 *     precision; the candidates are the chunks of DST those boxes (2 mm more per side) overlap, clipped to the 2^24 mm limit,
 *     ascending.  The rounding of q is below 1 mm, so for a rotation this is a superset of what can receive anything, and the result
 *     does not depend on how generous it is.  A count pass over the candidates leaves the per-chunk counts and the statistics; the
 *     host reads them (the one synchronisation besides the end of the call), gives the absent candidates with a non-zero count their
 *     slots, which are filled with fill_entry on the device, and a write pass over the candidates with a non-zero count samples again
 *     and integrates in place.
 *   ordering: both stores' locks are taken in address order; the work is stream-ordered behind everything enqueued on either store;
 *     the call synchronises before it returns.  SRC is only read.  The result buffers of DST's queries stay untouched. */
typedef struct ws_fuse_pose
{
  int32_t rot_q30[9];
  int32_t pivot_dst_mm[3];
  int32_t pivot_src_mm[3];
} ws_fuse_pose;
#define WS_FUSE_DEFAULT 0u
#define WS_FUSE_COUNT_ONLY 1u
int ws_store_fuse(ws_store *dst, ws_store *src, const ws_fuse_pose *pull, int32_t map_resolution, int32_t max_weight, uint32_t flags, uint64_t stats[6]);
/* Measurement entry, as ws_debug_store_view_gain_timing: ms_out receives the device time of the plan's upload, of the count pass and of
 * the write pass (with the fill of the created chunks) of the last call with this store as DST */
int ws_debug_store_fuse_timing(ws_store *dst, int32_t enable, float ms_out[3]);

/* A store at half the resolution of another: every voxel of DST is 2 x 2 x 2 voxels of SRC, computed on the device without a chunk
 * leaving HBM.  Every ws_store_* query takes the resolution as an argument, so the coarse store is queried, meshed, loaded into a
 * window and registered against like any other, with twice the map_resolution.  The rule uses integers only and the result is the
 * same bytes on every run.
 *   children: the coarse world voxel V has the eight children 2 V + (i, j, k), i, j, k in {0, 1}, for negative coordinates too.  The
 *     parent of the chunk key k is k >> 1 per axis (arithmetic shift, floor(k / 2)); a chunk of DST is fed by the up to eight chunks
 *     2 K + {0, 1}^3 of SRC.  A child in an absent chunk of SRC is unobserved.
 *   rule: a child is observed iff its weight is > 0 (there is no ANY_WEIGHT variant).  n = the number of observed children, S = the
 *     sum of their values, W = the smallest of their weights.  With n >= min_observed the coarse entry is (floor(S / n), W), the
 *     floor toward minus infinity; otherwise it is the fill_entry of DST.  |S| <= 2^18: everything is int32.
 *   min_observed: 1 .. 8.  With 8 and an even resolution r the coarse entry is what ws_store_sample reports at the centre
 *     (2 V + 1) r of the coarse voxel, where every trilinear fraction is r / 2: x = floor(S / 8), y = W, the cell valid.
 *   listed chunks: with dst_keys == NULL the parents of every chunk of SRC; otherwise the n_keys given keys, in any order, duplicates
 *     allowed.  A listed chunk with at least one child chunk in SRC exists in DST afterwards (created if need be) and all 262 144 of
 *     its words are written, each with the coarse entry or fill_entry.  A listed chunk without a child chunk is not created; if it
 *     exists, it is filled with fill_entry.  A chunk of DST that is not listed keeps every byte.
 *   plan: which chunks are created follows from the two directories alone, so there is no count pass and no host read.  The new
 *     chunks are counted before the launch (WS_ERR_CAPACITY, nothing changed, if they do not fit under max_chunks of DST), one row
 *     per chunk {dst slot, eight child slots} travels through a slot table of DST's ring, and one launch writes the chunks.
 *   stats: NULL: the call returns after enqueueing, stream-ordered on the context's stream behind everything enqueued on either
 *     store.  Otherwise the call synchronises and reports: chunks processed; chunks created; coarse voxels that received a value;
 *     coarse voxels with 1 <= n < min_observed.  Integer adds, exact whatever the order.
 *   refusals, nothing changed and nothing launched: WS_ERR_INVALID: a NULL store, dst == src, stores of different contexts,
 *     min_observed outside 1 .. 8, unknown flag bits, n_keys > 0 with NULL keys, a fill_entry of DST with weight > 0.  WS_ERR_RANGE:
 *     2^23 chunks to write or more.  WS_ERR_CAPACITY: see above.  WS_ERR_HIP: a segment cannot be allocated.  A HIP error while
 *     enqueueing takes the chunks the call created out of the directory again.  An empty SRC with dst_keys == NULL is WS_OK.
 *   ordering: both stores' locks are taken in address order.  SRC is only read.  The result buffers of DST's queries stay untouched.
 *   ws_store_parents_of: host only, no device: the parents of n keys, unique and ascending (cx, cy, cz); copies at most `capacity`
 *     keys and always reports the count. */
#define WS_COARSEN_DEFAULT 0u
int ws_store_coarsen(ws_store *dst, ws_store *src, const int32_t *dst_keys /* n_keys x 3 or NULL */, size_t n_keys, int32_t min_observed, uint32_t flags,
                     uint64_t stats[4] /* may be NULL */);
int ws_store_parents_of(const int32_t *keys /* n x 3 */, size_t n, int32_t *parents /* capacity x 3 */, size_t capacity, size_t *n_out);
/* Measurement entry, as ws_debug_store_fuse_timing: ms_out receives the device time of the plan's upload and of the pass of the last
 * call with this store as DST */
int ws_debug_store_coarsen_timing(ws_store *dst, int32_t enable, float ms_out[2]);

/* Change detection between two stores: WHERE the store CUR ("now") differs from the store REF ("before") under a rigid pose -- what
 * has appeared, what has been taken away -- as ordered records with clusters and exact statistics, on the device, without a chunk
 * leaving HBM.  The rule uses integers only and the result is the same bytes on every run.
 *   lattice and transform: the comparison runs on the voxel lattice of CUR.  The map from the frame of CUR to the frame of REF is the
 *     pull transform of ws_store_fuse with CUR in the place of DST and REF in the place of SRC: the same ws_fuse_pose, the same voxel
 *     mapping q(p) for the centre p = v res + h, the same reach (a voxel with a component of |p - pivot_dst| >= 2^24 mm is outside
 *     the call) and the same dead rule (a component of q of magnitude >= 2^30: the sample is not valid).
 *   voxels examined: the voxels of the PRESENT chunks of CUR that lie in the inclusive world-voxel box [lo, hi] and within the reach.
 *     The box rules are those of ws_store_frontier: both NULL: the bounding box of the present chunks; exactly one NULL or hi < lo:
 *     WS_ERR_INVALID; a box that meets no present chunk: WS_OK with zero records and zero statistics; 2^19 or more present chunks in
 *     the box: WS_ERR_RANGE.  A voxel of an absent chunk of CUR is unknown and is never examined.
 *   CUR side: the entry (ev, ew); KNOWN iff ew >= min_weight.
 *   REF side: the sample of ws_store_fuse at q, exactly as the fuse takes it, gives (nv, nw) or "not valid": corners with a zero
 *     coefficient take no part, a corner is valid iff its weight is > 0, a voxel of an absent chunk is not valid.  KNOWN iff the
 *     sample is valid and nw >= min_weight.
 *   classes of a known side with value d (ev, or nv): OCCUPIED iff |d| < band; FREE iff d >= free_value; otherwise neither.  Raw
 *     values, as in the frontier: the store knows no tau.
 *   kinds: APPEARED (1) iff CUR is OCCUPIED and REF is FREE; VANISHED (2) iff CUR is FREE and REF is OCCUPIED.  Nothing else is a
 *     record; unknown on either side is never a change.
 *   record: 16 bytes: x, y, z in world voxels of CUR, then the word (uint16)nv | kind << 16.  The records come in the output order of
 *     ws_store_frontier: ascending world (x, y, z), z fastest, across chunk borders.
 *   stats[6]: chunks of CUR listed; voxels known on both sides; voxels appeared; voxels vanished; voxels known in CUR and not in REF
 *     (new ground); over the voxels known on both sides the sum of |nv - ev|.  Integer adds, exact whatever the order; they always
 *     cover both kinds, whatever the flags select.
 *   flags: WS_CHANGES_APPEARED, WS_CHANGES_VANISHED: the kinds that become records (WS_CHANGES_DEFAULT: both).  WS_CHANGES_CLUSTERS:
 *     the labels and the 64-byte cluster table of ws_map_frontier over the selected records, with its numbering and its 2^31 - 1
 *     limit; with both kinds selected a moved object whose old and new place touch is one cluster.  Unknown bits, or no kind bit:
 *     WS_ERR_INVALID.
 *   refusals, nothing launched and the last result stays: WS_ERR_INVALID: a NULL store, pose or stats; cur == ref; stores of
 *     different contexts; a rot_q30 entry out of range; the box (above).  WS_ERR_RANGE: map_resolution < 1 or > 1024; band < 1;
 *     free_value < band or > 32767; min_weight < 1 or > 32767; 2^19 or more chunks of REF, or of CUR in the box.
 *   consequences: under the identity pose (rot = 2^30 I, equal pivots) every fraction is 0 and the rule is a plain voxel-by-voxel
 *     comparison of the two entries (the REF entry counts with weight > 0 and >= min_weight).  A store compared with a byte copy of
 *     itself gives zero records, and stats[1] equals its voxels with weight >= min_weight.
 *   ordering and ownership: both stores' locks are taken in address order; the work is stream-ordered behind everything enqueued on
 *     either store; the call synchronises.  Both stores are only read.  The result belongs to CUR, is apart from every other query's
 *     result (the frontier's included) and stays valid until the next ws_store_changes with this store as CUR.  Every output write is
 *     bounded by the buffers' capacities.
 *   cost: a count pass over the listed chunks of CUR (one coalesced read of CUR; REF is gathered only by the lanes whose CUR entry is
 *     known), the scan, and an emit pass that samples again on the voxels of the records: no buffer follows the number of voxels
 *     (32 KB of scratch and 32 bytes of tables per listed chunk, 16 bytes per chunk place of REF's lookup). */
#define WS_CHANGES_APPEARED 1u
#define WS_CHANGES_VANISHED 2u
#define WS_CHANGES_CLUSTERS 4u
#define WS_CHANGES_DEFAULT 3u
int ws_store_changes(ws_store *cur, ws_store *ref, const ws_fuse_pose *pull, int32_t map_resolution, const int32_t lo[3], const int32_t hi[3], int32_t band,
                     int32_t free_value, int32_t min_weight, uint32_t flags, size_t *n_out, size_t *n_clusters, uint64_t stats[6]);
const void *ws_store_changes_records_dev(const ws_store *cur, size_t *n);    /* device memory, n x 16 bytes; NULL when n == 0 */
const uint32_t *ws_store_changes_labels_dev(const ws_store *cur, size_t *n); /* n uint32; NULL unless the last call asked for clusters */
const void *ws_store_changes_clusters_dev(const ws_store *cur, size_t *n);   /* n x 64 bytes; NULL unless the last call asked for them */
/* as ws_map_frontier_download */
int ws_store_changes_download(ws_store *cur, void *records_host, uint32_t *labels_host, void *clusters_host, size_t cap_records, size_t cap_clusters, size_t *n_out,
                              size_t *n_clusters);
/* Measurement entry, as ws_debug_store_frontier_timing: ms_out receives the device time of the tables' upload with the count pass, of
 * the scan, of the emit pass and of the clustering of the last call with this store as CUR */
int ws_debug_store_changes_timing(ws_store *cur, int32_t enable, float ms_out[4]);

/* ------------------------------------------------------------------ packed snapshots of the global map ---- */
/* The chunks of a store in a packed form that removes the redundancy of a TSDF chunk (space never seen holds the default entry, free
 * space one repeated word), made and expanded on the device, the same bytes on every run.  The chunk set stays the host
 * directory's: the device classifies the bricks inside the chunks the host names and writes them in a fixed order.
 *   bricks: a chunk is 64^3 words, index x*4096 + y*64 + z; it is 8 x 8 x 8 bricks of 8^3 words.  The word at (x, y, z) is word
 *     (x&7)*64 + (y&7)*8 + (z&7) of brick b = ((x>>3)*8 + (y>>3))*8 + (z>>3).
 *   class of a brick, on raw uint32 words against a `fill` word: 0 default: every word == fill, no payload; 1 uniform: every word
 *     equals the brick's word 0 and that word != fill, 1 payload word; 2 dense: anything else, 512 payload words.  Code 3 is invalid.
 *   header: WS_PACK_HEADER_WORDS = 40 uint32 per chunk: [0..2] the key (int32); [3] the number of class-1 bricks; [4] the number of
 *     class-2 bricks; [5], [6] low and high word of the index of the chunk's first payload word (64-bit, counted in words); [7] 0;
 *     [8..39] the class codes, 2 bits per brick: brick b sits in word 8 + b/16, bits 2*(b%16).
 *   payload: one uint32 stream.  Chunks come in header order, and headers in strictly ascending key order (cx, then cy, then cz).
 *     Inside a chunk the bricks ascend; class 1 gives its word, class 2 its 512 words in brick word order.  A chunk contributes
 *     [3] + 512*[4] words, and its first word index is the sum of the contributions of the chunks before it.
 *
 * ws_store_pack packs the chunks `keys` names (n_keys x 3; NULL: every chunk of the store), in ascending key order whatever the order
 *   given, against the store's own fill_entry.  A named key the store does not hold, a key named twice, NULL keys with n_keys > 0,
 *   unknown flag bits: WS_ERR_INVALID, nothing launched, the last result stays.  The result (headers, payload) stays in buffers the
 *   store owns, apart from every other query's result, valid until the next ws_store_pack on this store.  The store is only read.
 *   stats[4] (may be NULL): default, uniform and dense bricks, and the bytes of headers + payload.  The call synchronises (the payload
 *   is sized from the scanned total); an allocation that fails is WS_ERR_HIP and leaves an empty result.  Counts and offsets are 64-bit.
 *   flags: WS_PACK_DEFAULT; WS_PACK_EMIT_DIRECT (measurement): the emit pass writes the payload straight from the lanes that read
 *   the chunk, in 32-byte runs, not through LDS; the bytes are the same.
 * ws_store_unpack / ws_store_unpack_dev: every listed chunk is created or overwritten WHOLE: class 0 bricks get `fill` (the
 *   argument, so a clone is byte-exact even into a store with another default), class 1 bricks their word, class 2 bricks their 512
 *   words.  Chunks not listed keep their bytes.  The headers are always the host's (the directory is the host's) and are validated
 *   first (ws_pack_check): every failure of the stream is WS_ERR_INVALID; more chunks than max_chunks allows: WS_ERR_CAPACITY; no
 *   memory for a segment or the staging: WS_ERR_HIP.  All refusals come before the first launch and leave the store unchanged.  Slots
 *   are handed out on the host before the launch.  ws_store_unpack_dev (payload in device memory: payload_words uint32 the caller
 *   keeps unchanged until the launch has run) is stream-ordered and does not wait for the device unless a segment is allocated;
 *   ws_store_unpack (payload in host memory) returns when the caller's buffers may be reused.  flags: 0.
 * ws_pack_check, ws_pack_expand_chunk, ws_pack_chunk: host only, no GPU and no context -- the CPU statement of the rule, for tools
 *   that read and write packed files.  ws_pack_check accepts a header list iff the keys ascend strictly, no class code is 3, the
 *   counts equal the class map, the first-word indices equal the running sum (64 bits), the total equals payload_words and word 7 is
 *   zero; else WS_ERR_INVALID with the reason in ws_last_error.  ws_pack_expand_chunk expands one chunk from its header and ITS OWN
 *   payload words (the stream at the header's first-word index) into out[262144].  ws_pack_chunk packs one chunk into a header
 *   (first-word index 0: whoever assembles a stream writes the running sum) and its own payload words; *words receives their number,
 *   and WS_ERR_CAPACITY is returned, with nothing written to payload_out, if cap_words is smaller. */
#define WS_PACK_HEADER_WORDS 40
#define WS_PACK_DEFAULT 0u
#define WS_PACK_EMIT_DIRECT 1u
int ws_store_pack(ws_store *st, const int32_t *keys /* n_keys x 3 or NULL: every chunk */, size_t n_keys, uint32_t flags, size_t *n_chunks, uint64_t *payload_words,
                  uint64_t stats[4] /* may be NULL */);
const uint32_t *ws_store_pack_headers_dev(const ws_store *st, size_t *n_chunks);        /* device memory, n_chunks x 40 uint32; NULL when 0 */
const uint32_t *ws_store_pack_payload_dev(const ws_store *st, uint64_t *payload_words); /* device memory; NULL when 0 */
/* Copies the last result to the host.  *n_chunks and *payload_words always receive the sizes; a capacity too small for a part that is
 * asked for: WS_ERR_CAPACITY, nothing copied.  headers_host or payload_host may be NULL: that part is not copied and its capacity
 * not looked at. */
int ws_store_pack_download(ws_store *st, uint32_t *headers_host, uint32_t *payload_host, size_t cap_chunks, uint64_t cap_words, size_t *n_chunks,
                           uint64_t *payload_words);
int ws_store_unpack(ws_store *st, const uint32_t *headers_host, const uint32_t *payload_host, size_t n_chunks, uint64_t payload_words, uint32_t fill, uint32_t flags);
int ws_store_unpack_dev(ws_store *st, const uint32_t *headers_host, const uint32_t *payload_dev, size_t n_chunks, uint64_t payload_words, uint32_t fill,
                        uint32_t flags);
int ws_pack_check(const uint32_t *headers, size_t n_chunks, uint64_t payload_words);
int ws_pack_expand_chunk(const uint32_t *header, const uint32_t *payload, uint32_t fill, uint32_t *out /* 262144 */);
int ws_pack_chunk(const uint32_t *chunk /* 262144 */, const int32_t key[3], uint32_t fill, uint32_t *header_out, uint32_t *payload_out, uint64_t cap_words,
                  uint64_t *words);
/* Measurement entry, as ws_debug_store_surface_timing: ms_out receives the device time of the classify pass, of the scan and of the
 * emit pass of the last ws_store_pack on this store -- or, if a ws_store_unpack came after it, that call's launch in ms_out[0] and
 * zeros */
int ws_debug_store_pack_timing(ws_store *st, int32_t enable, float ms_out[3]);

/* ------------------------------------------------------------------ TSDF update ---- */
/* TSDFCuda::update_tsdf(scan_points, scanner_pos, up) — update_tsdf.cu:143-166.
 * xyz_host: n x 3 int32 (rmagine::Pointi AoS); scanner_pos in voxel units, up scaled by 32768.
 * Returns after enqueueing, like the reference (no device sync). */
int ws_tsdf_update(ws_map *map, const int32_t *xyz_host, size_t n, const int32_t scanner_pos[3], const int32_t up[3]);
/* same with the scan already resident in HBM (no H2D copy).  Asynchronous like a stream copy: xyz_dev must stay unchanged until
 * the kernels enqueued by this call have read it (stream order: anything enqueued later on the context's stream is safe, e.g.
 * ws_scan_preprocess of the next frame).  The next call that takes this map -- ws_register_cloud, ws_reg_iterate, ws_sync, a
 * download, the next update -- looks at the scan's verdict first and repeats the scan with a larger record pool in the rare case
 * that it did not fit (never an inexact map); the repeat reads a copy of the scan that the first attempt left in a buffer of the
 * map, not xyz_dev. */
int ws_tsdf_update_dev(ws_map *map, const int32_t *xyz_dev, size_t n, const int32_t scanner_pos[3], const int32_t up[3]);
/* only the scatter (cu_min_tsdf_krnl, update_tsdf.cu:45-128): fills new_map, no integrate. For parity tests. */
int ws_tsdf_scatter_dev(ws_map *map, const int32_t *xyz_dev, size_t n, const int32_t scanner_pos[3], const int32_t up[3]);
/* only the integrate pass (cu_avg_tsdf_krnl, update_tsdf.cu:13-43) */
int ws_tsdf_integrate(ws_map *map);
int ws_tsdf_set_integrate(ws_map *map, int mode);
/* Candidate-record capacity of the scatter: records of 8 bytes in sub-chunks of 32 that belong to one 4x4x64-voxel tile each,
 * taken from a pool.  The pool is sized from the scan's own record bound (its set-up pass counts every ray step as a candidate,
 * ~2.7 x what a scan makes) plus a fixed share per work item -- an estimate: how many partly filled sub-chunks a scan leaves
 * has no useful bound.  A scan that does exhaust the pool is ABORTED -- the maps stay untouched -- and repeated with a larger
 * pool inside the same ws_tsdf_update* call, which therefore returns once the marches are over (~0.35 ms into the update, the
 * resolve still running).  Reserving up front only avoids such a re-run. */
int ws_tsdf_set_capacity(ws_map *map, uint64_t records);
/* Test entry: the pool's share for the records is (record bound / 32) >> (est_shift - 1) (0: the default, the whole bound) -- a
 * large shift forces the abort-and-repeat route on a small map.  budget_bytes is unused (rounds 1-4 had a second policy). */
int ws_debug_tsdf_chunk_policy(ws_map *map, uint64_t budget_bytes, uint32_t est_shift);

typedef struct
{
  int64_t contested_voxels; /* voxels of the last update decided by the exact ordered rounds (a negative-weight
                               candidate could have blocked the earliest positive one)                         */
  int64_t records;          /* scatter targets that became records (ray tails + free-space candidates on keyed voxels) */
  int64_t tiles;            /* touched 4x4x64-voxel tiles (resolved and integrated)                             */
  int32_t error_flags;      /* device error bits since the last call: 2 record-field range, 4 free-space bound, 8 internal */
  int32_t hash_entries;     /* entries beyond a tile's 128th that went through the (tile, number) hash since it was last emptied */
  int64_t runs;             /* (wave, tile) groups of records: one reservation in the tile's entry table each           */
  int64_t free_space_hits;  /* free-space candidates that met ordered candidates (and joined that tile's records)   */
  int64_t record_slots;     /* the scan's record bound (from its set-up pass) ...                                 */
  int64_t record_capacity;  /* ... and the record places of the pool (sub-chunks x 32)                             */
} ws_tsdf_stats_t;
int ws_tsdf_stats(ws_map *map, ws_tsdf_stats_t *out); /* synchronises */

/* ------------------------------------------------------------------ registration ---- */
/* RegistrationCuda::RegistrationCuda — registration.cu:259-281 (buffers grow on demand beyond max_points) */
int ws_reg_create(ws_context *ctx, size_t max_points, ws_reg **out);
int ws_reg_destroy(ws_reg *reg);
/* RegistrationCuda::prepare_registration — registration.cu:303-308 */
int ws_reg_prepare(ws_reg *reg, const int32_t *xyz_host, size_t n);
/* the same for a cloud in HBM: an asynchronous device-to-device copy on the context's stream (xyz_dev must stay unchanged until that
 * copy has run: anything enqueued later on the context's stream is safe; a caller with streams of its own -- torch's allocator --
 * keeps the buffer until the next ws_reg_prepare* or a ws_sync, as warpsense_amd/api.py does) */
int ws_reg_prepare_dev(ws_reg *reg, const int32_t *xyz_dev, size_t n);
/* the registration's own copy of the prepared cloud (device memory, n x 3 int32) and its point count; the pointer
 * changes when a larger cloud makes the buffer grow (callers that capture kernels into HIP graphs key on it) */
const int32_t *ws_reg_points_dev(const ws_reg *reg, size_t *n);
/* RegistrationCuda::perform_registration — registration.cu:347-368. T, h column-major. Synchronises. */
int ws_reg_iterate(ws_reg *reg, const ws_map *map, const float T[16], int32_t map_resolution, uint32_t flags,
                   int64_t h[36], int64_t g[6], int32_t *e, int32_t *c);
/* cuda::TSDFRegistration::register_cloud — src/warpsense/tsdf_registration.cpp:28-96 with the whole
 * Gauss-Newton loop on the device (points must have been given to ws_reg_prepare*). Synchronises. */
int ws_register_cloud(ws_reg *reg, const ws_map *map, const float T_in[16], int32_t max_iterations,
                      float it_weight_gradient, float epsilon, int32_t map_resolution, uint32_t flags,
                      float T_out[16], int32_t *iterations);
int ws_reg_set_loop(ws_reg *reg, int mode /* WS_REG_LOOP_* */);

/* K registrations of the prepared cloud against one map, each from its own start pose, in one launch.
 * T_in, T_out: k x 16 floats, column-major; iterations, e_out, c_out: k each (the last three may be NULL).
 * Result k is bit for bit what ws_register_cloud(reg, map, T_in + 16 k, ...) returns alone;
 * e_out[k], c_out[k] are e and c of ws_reg_iterate at T_out + 16 k.  k == 0 is WS_OK.  Synchronises.
 * One workgroup runs the whole Gauss-Newton loop of one start pose: no exchange between workgroups, nothing that must be
 * resident together, so k may exceed the number of compute units.  `flags` select the points exactly as for ws_register_cloud.
 * WS_ERR_INVALID: NULL reg / map, NULL T_in / T_out with k > 0, map_resolution < 1.  A living resident server of ws_reg_iterate
 * is asked to leave first.  The call leaves the single route alone: the handle's loop mode, the sums ws_debug_reg_sums
 * reports and the state ws_reg_poll reads are those of the last ws_register_cloud.  The per-pose device records live in `reg`
 * and grow on demand. */
int ws_register_cloud_batch(ws_reg *reg, const ws_map *map, const float *T_in, size_t k, int32_t max_iterations,
                            float it_weight_gradient, float epsilon, int32_t map_resolution, uint32_t flags,
                            float *T_out, int32_t *iterations, int32_t *e_out, int32_t *c_out);
/* Host only: the best hypothesis of a batch.  Among those with c[i] >= min_count the one with the smallest e[i] / c[i],
 * compared exactly as e[a] * c[b] < e[b] * c[a] in int64; ties: larger c, then lower index.  *best = -1 if none.
 * (e is a sum of |value|, so e >= 0; a hypothesis with c[i] <= 0 has no mean and is never chosen.) */
int ws_reg_batch_best(const int32_t *e, const int32_t *c, size_t k, int32_t min_count, int64_t *best);

/* Building blocks of the same loop for point-sharded multi-GPU runs: every rank owns the
 * points [first, first+count) of the prepared cloud, accumulates its 44 int64 partial sums
 * (h[36] column-major, g[6], e, c) into sums_dev, the caller all-reduces sums_dev (RCCL), then every
 * rank runs the identical solve. All stream-ordered, no host synchronisation. */
int ws_reg_begin(ws_reg *reg, const float T_in[16], int32_t max_iterations, float it_weight_gradient, float epsilon);
int ws_reg_accumulate_dev(ws_reg *reg, const ws_map *map, int32_t map_resolution, uint32_t flags, size_t first,
                          size_t count, int64_t *sums_dev /* 44 */);
int ws_reg_solve_dev(ws_reg *reg, const int64_t *sums_dev /* 44 */);
/* The same two steps as ONE launch per iteration: if apply_previous != 0, first the Gauss-Newton update from the 44
 * (all-reduced) sums in sums_dev -- exactly what ws_reg_solve_dev does --, then the accumulation of [first, first+count)
 * into sums_dev.  A sharded loop is: ws_reg_begin; { ws_reg_iterate_shard_dev(apply_previous = not the first); all-reduce
 * sums_dev } x n; ws_reg_solve_dev(sums_dev); ws_reg_poll.  Do not touch sums_dev between the all-reduce and the next call. */
int ws_reg_iterate_shard_dev(ws_reg *reg, const ws_map *map, int32_t map_resolution, uint32_t flags, size_t first, size_t count,
                             int64_t *sums_dev /* 44 */, int32_t apply_previous);
int ws_reg_poll(ws_reg *reg, int32_t *finished, int32_t *iterations, float T_out[16]); /* synchronises */

/* The same sharded loop WITHOUT the host in it (north_star: point-sharded registration across GPUs): every rank runs the
 * resident loop of ws_register_cloud on its points [first, first + count) and the ranks' 44 sums meet in MAILBOXES in each
 * other's HBM -- fine-grained device memory, peer-mapped through hipIpc, system-scope atomic adds over xGMI whose top byte
 * counts the ranks (exact for any rank order) -- so an iteration costs one device-side exchange instead of a launch, an RCCL
 * call and two host calls.  Set-up, once per process group:
 *   ws_reg_peer_mailbox(reg, handle)            -> this rank's mailbox as a 64-byte IPC handle (hipIpcMemHandle_t)
 *   [all-gather the handles, any transport]
 *   ws_reg_peer_connect(reg, rank, world, handles (world x 64 bytes), blocks)
 * then all ranks call ws_register_cloud_peers together for every cloud (every rank has prepared the WHOLE cloud; the map is
 * replicated).  `blocks`: workgroups of the loop on this rank, 0 = 256 (one per CU); ranks that share one GPU (tests) pass
 * 256 / ranks-per-GPU so that all of them are resident at once.  WS_ERR_TIMEOUT: a peer did not deliver within 20 ms
 * (WS_REG_PEER_TIMEOUT_MS in the environment at connect time changes the limit) -- all ranks see it; call ws_reg_peer_reset
 * on every rank (between two barriers of the caller's) and fall back to the RCCL route.  Until then every further
 * ws_register_cloud_peers on this handle is refused (WS_ERR_INVALID): the mailboxes hold the partial additions of the
 * exchange that was given up.
 * ws_reg_peer_connect_local connects ws_reg handles of ONE process (several contexts / streams on one GPU) without IPC. */
#define WS_IPC_HANDLE_BYTES 64
int ws_reg_peer_mailbox(ws_reg *reg, void *ipc_handle_out /* WS_IPC_HANDLE_BYTES, may be NULL */);
int ws_reg_peer_connect(ws_reg *reg, int32_t rank, int32_t world, const void *ipc_handles, int32_t blocks);
int ws_reg_peer_connect_local(ws_reg *reg, int32_t rank, int32_t world, ws_reg *const *regs, int32_t blocks);
int ws_reg_peer_disconnect(ws_reg *reg);
int ws_reg_peer_reset(ws_reg *reg);
int ws_register_cloud_peers(ws_reg *reg, const ws_map *map, size_t first, size_t count, const float T_in[16], int32_t max_iterations,
                            float it_weight_gradient, float epsilon, int32_t map_resolution, uint32_t flags, float T_out[16],
                            int32_t *iterations);

/* Test entry: the 6x6 solve of the Gauss-Newton update alone (LU with partial pivoting in double, one wavefront per
 * system; stands for Eigen's hf.inverse() * g, tsdf_registration.cpp:69). n systems: A row-major n x 36, b n x 6 ->
 * x n x 6, status n (0, or -1 for a singular matrix). Host pointers; synchronises. */
int ws_debug_solve6(ws_context *ctx, const double *A, const double *b, size_t n, double *x, int32_t *status);

/* Diagnostics: the per-workgroup statistics slots of the last TSDF update (records per tail workgroup, then at +65536 its
 * flush groups, then at +131072 the contested voxels per resolve workgroup).  Synchronises. */
int ws_debug_block_stats(ws_map *map, uint32_t *out, size_t words);

/* Test entry: make the NEXT resident registration of `reg` lose one workgroup's contribution to the first exchange, as if
 * another kernel kept that workgroup off the chip: the exchange times out (5 ms) and ws_register_cloud repeats the
 * registration with one launch per iteration. *fallbacks (may be NULL) receives how often that has happened on `reg`. */
int ws_debug_reg_stall(ws_reg *reg, int32_t stall_next, int32_t *fallbacks);
/* test / tuning entry: the resident server behind ws_reg_iterate (enable: 1 / 0, -1 = leave as it is; idle_us > 0: how long it
 * stays without a request, default 50); *launches = servers started so far on this handle */
int ws_debug_reg_server(ws_reg *reg, int32_t enable, int32_t idle_us, int32_t *launches);
/* Test entry, no GPU needed: the host half of the server's mail protocol (request line with checksum, the answer's seven tagged lines:
 * stale, incomplete and torn answers must not be taken).  0: as expected, else a bit per failed case. */
int ws_debug_reg_mail_selftest(void);

/* Test entry: the 44 sums (h[36] column-major, g[6], e, c -- the out-parameters of perform_registration, registration.cu:347-368)
 * the LAST Gauss-Newton update of the last ws_register_cloud / ws_register_cloud_peers on `reg` was made from.  Synchronises. */
int ws_debug_reg_sums(ws_reg *reg, int64_t sums_out[44]);

/* ------------------------------------------------------------------ scan pre-processing ---- */
/* App::preprocess — src/warpsense/app.cpp:119-148, on the device: sensor points in float metres
 * (x y z first, `stride_floats` floats per point, e.g. 3, or 4 for PointXYZI) are dropped if x, y and z are all
 * < 0.3, scaled to mm, snapped to the centre of their `map_resolution` voxel, transformed by to_int_mat(pose)
 * (pose: 4x4 column-major, translation in mm) and de-duplicated.  Output: int32 mm points in the order of their
 * first occurrence in the input (the reference's unordered_set order is unspecified), resident on the device
 * until the next call: feed ws_scan_points_dev() to ws_tsdf_update_dev / ws_reg_prepare_dev.  Synchronises
 * (the count comes back to the host).  WS_ERR_RANGE: a transformed coordinate beyond +-2^20 mm. */
int ws_scan_create(ws_context *ctx, size_t max_points, ws_scan **out);
int ws_scan_destroy(ws_scan *scan);
int ws_scan_preprocess(ws_scan *scan, const float *xyz_host, size_t n, size_t stride_floats, const float pose[16],
                       int32_t map_resolution, size_t *n_out);
int ws_scan_preprocess_dev(ws_scan *scan, const float *xyz_dev, size_t n, size_t stride_floats, const float pose[16],
                           int32_t map_resolution, size_t *n_out);
const int32_t *ws_scan_points_dev(const ws_scan *scan); /* n_out x 3 int32, device memory */
int ws_scan_download(ws_scan *scan, int32_t *xyz_host, size_t capacity_points, size_t *n_out);

/* Motion-compensated pre-processing: one sensor pose per time bin of a sweep (a spinning lidar moves while it turns).
 * A sweep is described by k poses (1 <= k <= WS_SWEEP_MAX_BINS; each 4x4 column-major float, translation in mm, as `pose` above;
 * poses_host: k x 16 floats) and a rule that gives every input point a bin b in 0 .. k-1.  Point i is treated exactly as the
 * plain call treats it with to_int_mat(poses[b]) in place of to_int_mat(pose): the same drop rule (x, y, z all < 0.3;
 * non-finite dropped), the same float snapping to the voxel centre in the sensor frame, the same wrapping int32 products and
 * truncating division by 32768, the same +-2^20 mm range check (WS_ERR_RANGE).  De-duplication runs over the whole sweep, not per
 * bin: two points of different bins that land on the same integer point are kept once, at the first one's input position.  The
 * output is the input order with later duplicates removed; it is read with ws_scan_points_dev / ws_scan_download as above.
 * With k = 1 the result is that of the plain call with poses[0].
 *
 * The rule (ws_sweep_t) is one of two:
 *   by index (time_field = -1): the cloud is organised, `columns` >= 1 firing columns with n % columns == 0.
 *       col = ring_major ? i % columns : i / (n / columns);   b = (uint64)col * k / columns
 *     (ring_major != 0: index = ring * columns + column, the order of an image row per ring; 0: column after column.)
 *   by a per-point time (3 <= time_field < stride_floats): t is the float at that index of the point's record,
 *       s = (t - t_begin) / (t_end - t_begin);   v = s * (float)k         (each operation in float32, not contracted)
 *       b = v >= (float)k ? k - 1 : (v > 0 ? (uint32)v : 0)
 *     so a time before t_begin goes to bin 0, one after t_end to bin k-1, and s * k exactly integral to the upper bin.  A NaN s
 *     drops the point.  t_begin == t_end or a non-finite bound is refused; columns and ring_major are not read.
 * WS_ERR_INVALID, before anything is launched (the next valid call works as usual): k out of range, n % columns != 0 or
 * columns == 0, a time_field of 0..2, below -1 or >= stride_floats, bad time bounds, NULL arguments, stride_floats < 3,
 * map_resolution < 1, n above what ws_scan_create reserved.
 * The poses are converted on the host with the plain call's to_int_mat, one 64-byte row of 16 int32 per bin, and uploaded in stream
 * order from pinned memory; the table and its staging belong to `scan` and are allocated by the first sweep call.  Synchronises. */
#define WS_SWEEP_MAX_BINS 4096
typedef struct
{
  uint32_t columns;   /* by index: firing columns of the organised cloud             */
  int32_t ring_major; /* by index: != 0 if index = ring * columns + column          */
  int32_t time_field; /* -1: by index; else the index of the time in a point record */
  float t_begin, t_end; /* by time: the times of the sweep's begin and end           */
} ws_sweep_t;
int ws_scan_preprocess_sweep(ws_scan *scan, const float *xyz_host, size_t n, size_t stride_floats, const float *poses_host, uint32_t k,
                             const ws_sweep_t *rule, int32_t map_resolution, size_t *n_out);
int ws_scan_preprocess_sweep_dev(ws_scan *scan, const float *xyz_dev, size_t n, size_t stride_floats, const float *poses_host, uint32_t k,
                                 const ws_sweep_t *rule, int32_t map_resolution, size_t *n_out);
/* The k poses of a sweep from the pose at its end and the motion during it.  Pure host code in double; needs no device.
 * motion: the sensor's pose at the end of the sweep expressed in its frame at the beginning, T_begin^-1 * T_end (column-major, mm).
 * poses_out[b] (k x 16, column-major) is the pose at s_b = (b + 0.5) / k:  pose_end * rel(s_b), where
 *   rotation of rel(s)    = exp((1 - s) * log(R_motion^T))
 *   translation of rel(s) = (1 - s) * (-R_motion^T * t_motion)
 * -- slerp and lerp towards the end frame: rel(1) = I, rel(0) = motion^-1 -- rounded to float32 once, at the end.  The logarithm
 * is taken as axis and angle: axis from the skew part of R_motion^T, angle = atan2(|skew part|, (trace - 1) / 2).  A motion that is
 * exactly the identity returns pose_end bit for bit in every bin.  WS_ERR_INVALID: k out of range, NULL or non-finite input, a
 * rotation of more than 90 degrees within the sweep. */
int ws_sweep_poses(const float pose_end[16], const float motion[16], uint32_t k, float *poses_out);

/* ------------------------------------------------------------------ measurement ---- */
/* Kernel classes for hipEvent timing (bench.py's roofline leg). */
#define WS_K_SETUP 0         /* per-ray set-up + direction sort                                    */
#define WS_K_MARCH_TAILS 1   /* ray tails -> records, handed to the chunks of their tiles            */
#define WS_K_MARCH_FREE 2    /* free-space steps -> one byte per voxel                             */
#define WS_K_TILE_BIN 3      /* rounds 1-3 only (no kernel of this class since round 4: always 0)   */
#define WS_K_TILE_RESOLVE 4  /* exact per-tile fold in LDS (+ fused integrate)                     */
#define WS_K_INTEGRATE 5     /* separate sparse or dense weighted-average pass (cu_avg_tsdf_krnl)  */
#define WS_K_REG 6           /* Gauss-Newton iterations (accumulate + solve)                       */
#define WS_K_UPDATE 7        /* one span over ALL kernels of a ws_tsdf_update* call (two events per scan)  */
#define WS_K_COUNT 8
int ws_prof_enable(ws_context *ctx, uint32_t class_mask); /* 0 disables */
/* sum of event-measured durations and number of launches per class since the last reset (synchronises) */
int ws_prof_read(ws_context *ctx, int kernel_class, double *total_ms, int64_t *launches);
int ws_prof_reset(ws_context *ctx);

#ifdef __cplusplus
}
#endif
#endif /* WARPSENSE_HIP_H */
