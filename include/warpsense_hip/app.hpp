// app.hpp — ROS-free C++ twins of the code AROUND the hot path, on top of compat.hpp / mapping.hpp:
//
//   GlobalMap      HDF5GlobalMap            src/map/hdf5_global_map.cpp:4-221   64^3-voxel chunks, 64-chunk LRU, .h5 file
//   LocalMap       HDF5LocalMap             src/map/hdf5_local_map.cpp:5-217    host ring buffer, shift(), write_back()
//   MappingNode    cuda::TSDFMapping::map_shift  tsdf_mapping.cpp:97-136        + device-side shift_map / write_back
//   App            warpsense::App           src/warpsense/app.cpp:30-224        cloud_callback sequencing without ROS
//
// The .h5 file needs libwarpsense_h5.so (include/warpsense_h5.h); define WARPSENSE_HIP_WITH_H5 before including this
// header to compile the file backing in, otherwise GlobalMap keeps every chunk in memory.
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>

#include "warpsense_hip/mapping.hpp"
#include "warpsense_hip/visualization.hpp"
#ifdef WARPSENSE_HIP_WITH_H5
#include "warpsense_h5.h"
#endif

namespace warpsense
{
namespace rm = rmagine;

inline int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// ---------------------------------------------------------------------------------------------------- GlobalMap
class GlobalMap
{
public:
  static constexpr int CHUNK_SIZE = 64;  // hdf5_global_map.h:75
  static constexpr int NUM_CHUNKS = 64;  // hdf5_global_map.h:78
  using Key = std::array<int, 3>;

  GlobalMap(int16_t default_value, int16_t default_weight, const std::string &filename = std::string())
      : default_entry_(default_value, default_weight), filename_(filename)
  {
#ifdef WARPSENSE_HIP_WITH_H5
    if (!filename_.empty() && ws_h5_create(filename_.c_str(), &file_) != 0) throw std::runtime_error(ws_h5_last_error());
#else
    if (!filename_.empty()) throw std::runtime_error("GlobalMap: built without WARPSENSE_HIP_WITH_H5");
#endif
  }
  ~GlobalMap()
  {
#ifdef WARPSENSE_HIP_WITH_H5
    if (file_)
    {
      write_back();
      ws_h5_close(file_);
    }
#endif
  }
  GlobalMap(const GlobalMap &) = delete;
  GlobalMap &operator=(const GlobalMap &) = delete;

  const std::string &filename() const { return filename_; }
  bool has_file() const { return file_backed(); }
  TSDFEntry get_default_tsdf_entry() const { return default_entry_; }

  // activate_chunk — hdf5_global_map.cpp:59-135: cached, else read from the file, else default-filled; the least
  // recently used chunk is written to the file when a 65th is needed (memory-only maps keep everything)
  std::vector<TSDFEntry::RawType> &activate_chunk(const Key &c)
  {
    auto it = chunks_.find(c);
    if (it != chunks_.end())
    {
      if (file_backed()) touch(c);
      return it->second;
    }
    std::vector<TSDFEntry::RawType> data((size_t)CHUNK_SIZE * CHUNK_SIZE * CHUNK_SIZE);
    bool found = false;
#ifdef WARPSENSE_HIP_WITH_H5
    if (file_)
    {
      int32_t ex = 0;
      if (ws_h5_read_chunk(file_, c[0], c[1], c[2], data.data(), &ex) != 0) throw std::runtime_error(ws_h5_last_error());
      found = ex != 0;
    }
#endif
    if (!found) std::fill(data.begin(), data.end(), default_entry_.raw());
    if (file_backed() && (int)chunks_.size() >= NUM_CHUNKS)
    {
      const Key old = lru_.back();
      write_chunk(old, chunks_[old]);
      chunks_.erase(old);
      lru_.pop_back();
    }
    auto &ref = chunks_[c];
    ref = std::move(data);
    if (file_backed()) lru_.push_front(c);
    return ref;
  }
  static int index_from_pos(int x, int y, int z, const Key &c) // :53-57
  {
    return (x - c[0] * CHUNK_SIZE) * CHUNK_SIZE * CHUNK_SIZE + (y - c[1] * CHUNK_SIZE) * CHUNK_SIZE + (z - c[2] * CHUNK_SIZE);
  }
  TSDFEntry get_value(int x, int y, int z)
  {
    const Key c{floor_div(x, CHUNK_SIZE), floor_div(y, CHUNK_SIZE), floor_div(z, CHUNK_SIZE)};
    return TSDFEntry(activate_chunk(c)[index_from_pos(x, y, z, c)]);
  }
  void set_value(int x, int y, int z, const TSDFEntry &v)
  {
    const Key c{floor_div(x, CHUNK_SIZE), floor_div(y, CHUNK_SIZE), floor_div(z, CHUNK_SIZE)};
    activate_chunk(c)[index_from_pos(x, y, z, c)] = v.raw();
  }
  // true if the map holds data for this chunk (in memory or in the file): a chunk never seen is all default
  bool has_chunk(const Key &c)
  {
    std::lock_guard<std::recursive_mutex> g(mutex_);
    return chunks_.count(c) != 0 || in_file_.count(c) != 0;
  }
  // dense world-voxel box [lo, hi] (inclusive, x major / z fastest) <-> chunks.  Thread safe per chunk: the map-shift
  // worker files slabs while the scan thread writes poses (the HDF5 library is used by one thread at a time).
  void save_box(const rm::Pointi &lo, const rm::Pointi &hi, const std::vector<TSDFEntry> &box) { move_box(lo, hi, const_cast<TSDFEntry *>(box.data()), true); }
  void save_box(const rm::Pointi &lo, const rm::Pointi &hi, const TSDFEntry *box) { move_box(lo, hi, const_cast<TSDFEntry *>(box), true); }
  void load_box(const rm::Pointi &lo, const rm::Pointi &hi, std::vector<TSDFEntry> &box)
  {
    box.resize((size_t)(hi.x - lo.x + 1) * (size_t)(hi.y - lo.y + 1) * (size_t)(hi.z - lo.z + 1));
    move_box(lo, hi, box.data(), false);
  }
  // a whole chunk from elsewhere (DeviceGlobalMap::flush_to): over the cached copy if the chunk is active; else straight into the
  // file of a file-backed map (no read, no default fill, no turn of the LRU), or into the cache of a memory-only one
  void put_chunk(const Key &c, const std::vector<TSDFEntry::RawType> &data)
  {
    std::lock_guard<std::recursive_mutex> g(mutex_);
    auto it = chunks_.find(c);
    if (it != chunks_.end())
      it->second = data;
    else if (file_backed())
      write_chunk(c, data);
    else
      chunks_[c] = data;
  }
  void write_back() // :160-176
  {
#ifdef WARPSENSE_HIP_WITH_H5
    std::lock_guard<std::recursive_mutex> g(mutex_);
    if (!file_) return;
    for (auto &kv : chunks_) write_chunk(kv.first, kv.second);
    ws_h5_flush(file_);
#endif
  }
  // write_pose — :178-199 (rotation as Eigen would turn it into a quaternion, every value rounded to 3 decimals)
  std::array<float, 7> write_pose(const rm::Matrix4x4f &pose, float scale)
  {
    std::array<float, 7> v = pose_values(pose, scale);
#ifdef WARPSENSE_HIP_WITH_H5
    std::lock_guard<std::recursive_mutex> g(mutex_);
    if (file_ && ws_h5_write_pose(file_, v.data()) != 0) throw std::runtime_error(ws_h5_last_error());
#endif
    return v;
  }
  void write_meta(int tau, const rm::Pointi &size, float max_distance, int resolution, int max_weight) // :207-221
  {
#ifdef WARPSENSE_HIP_WITH_H5
    if (file_ && ws_h5_write_meta(file_, tau, &size.x, max_distance, resolution, max_weight) != 0) throw std::runtime_error(ws_h5_last_error());
#else
    (void)tau; (void)size; (void)max_distance; (void)resolution; (void)max_weight;
#endif
  }
  static std::array<float, 7> pose_values(const rm::Matrix4x4f &pose, float scale)
  {
    std::array<float, 7> v{};
    for (int k = 0; k < 3; ++k) v[k] = (float)(std::round(((double)pose.at(k, 3) / scale) * 1000.0f) / 1000.0f);
    float q[4]; // x y z w, Eigen::Quaternionf(Matrix3f)
    const auto m = [&](int i, int j) { return pose.at(i, j); };
    float t = m(0, 0) + m(1, 1) + m(2, 2);
    if (t > 0.f)
    {
      t = std::sqrt(t + 1.0f);
      q[3] = 0.5f * t;
      t = 0.5f / t;
      q[0] = (m(2, 1) - m(1, 2)) * t;
      q[1] = (m(0, 2) - m(2, 0)) * t;
      q[2] = (m(1, 0) - m(0, 1)) * t;
    }
    else
    {
      int i = 0;
      if (m(1, 1) > m(0, 0)) i = 1;
      if (m(2, 2) > m(i, i)) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0f);
      q[i] = 0.5f * t;
      t = 0.5f / t;
      q[3] = (m(k, j) - m(j, k)) * t;
      q[j] = (m(j, i) + m(i, j)) * t;
      q[k] = (m(k, i) + m(i, k)) * t;
    }
    for (int n = 0; n < 4; ++n) v[3 + n] = std::round(q[n] * 1000.0f) / 1000.0f;
    return v;
  }
  size_t active_chunks() const { return chunks_.size(); }

private:
  bool file_backed() const
  {
#ifdef WARPSENSE_HIP_WITH_H5
    return file_ != nullptr;
#else
    return false;
#endif
  }
  void touch(const Key &c)
  {
    lru_.remove(c);
    lru_.push_front(c);
  }
  void write_chunk(const Key &c, const std::vector<TSDFEntry::RawType> &data)
  {
#ifdef WARPSENSE_HIP_WITH_H5
    if (ws_h5_write_chunk(file_, c[0], c[1], c[2], data.data()) != 0) throw std::runtime_error(ws_h5_last_error());
    in_file_.insert(c);
#else
    (void)c; (void)data;
#endif
  }
  void move_box(const rm::Pointi &lo, const rm::Pointi &hi, TSDFEntry *box, bool save)
  {
    const int cs = CHUNK_SIZE;
    const size_t ey = (size_t)(hi.y - lo.y + 1), ez = (size_t)(hi.z - lo.z + 1);
    for (int cx = floor_div(lo.x, cs); cx <= floor_div(hi.x, cs); ++cx)
      for (int cy = floor_div(lo.y, cs); cy <= floor_div(hi.y, cs); ++cy)
        for (int cz = floor_div(lo.z, cs); cz <= floor_div(hi.z, cs); ++cz)
        {
          const Key c{cx, cy, cz};
          std::lock_guard<std::recursive_mutex> g(mutex_);
          auto &chunk = activate_chunk(c);
          const int ax = std::max(lo.x, cx * cs), bx = std::min(hi.x, cx * cs + cs - 1);
          const int ay = std::max(lo.y, cy * cs), by = std::min(hi.y, cy * cs + cs - 1);
          const int az = std::max(lo.z, cz * cs), bz = std::min(hi.z, cz * cs + cs - 1);
          for (int x = ax; x <= bx; ++x)
            for (int y = ay; y <= by; ++y)
            {
              TSDFEntry::RawType *cp = &chunk[index_from_pos(x, y, az, c)];
              TSDFEntry *bp = &box[((size_t)(x - lo.x) * ey + (size_t)(y - lo.y)) * ez + (size_t)(az - lo.z)];
              for (int z = az; z <= bz; ++z, ++cp, ++bp)
              {
                if (save)
                  *cp = bp->raw();
                else
                  bp->raw(*cp);
              }
            }
        }
  }

  TSDFEntry default_entry_;
  std::string filename_;
  std::map<Key, std::vector<TSDFEntry::RawType>> chunks_;
  std::list<Key> lru_;
  std::set<Key> in_file_; // chunks written to the file by this object
  std::recursive_mutex mutex_;
#ifdef WARPSENSE_HIP_WITH_H5
  ws_h5 *file_ = nullptr;
#else
  void *file_ = nullptr;
#endif
};

// what DeviceGlobalMap::changes returns (ws_store_changes)
struct Changes
{
  std::vector<ChangeRecord> records;     // ascending world (x, y, z), z fastest
  std::vector<uint32_t> labels;          // the cluster number of every record; empty unless asked for
  std::vector<FrontierCluster> clusters; // numbered by their first record; empty unless asked for
  ChangeStats stats;
};

// ---------------------------------------------------------------------------------------------------- DeviceGlobalMap
// The global map in device memory (ws_store, warpsense_hip.h): 64^3 chunks in HBM, the key -> slot directory on the host.  A
// MappingNode that has one attached shifts with device-to-device copies (shift_map_device) and writes back through it.
class DeviceGlobalMap
{
public:
  using Key = GlobalMap::Key;
  static constexpr size_t CHUNK_WORDS = (size_t)GlobalMap::CHUNK_SIZE * GlobalMap::CHUNK_SIZE * GlobalMap::CHUNK_SIZE;
  explicit DeviceGlobalMap(const TSDFEntry &default_entry, uint64_t max_chunks = 0, uint32_t segment_chunks = 0)
  {
    WS_CHECK(ws_store_create(cuda::detail::context(), default_entry.raw(), max_chunks, segment_chunks, &store_));
    fill_ = default_entry.raw();
  }
  ~DeviceGlobalMap() { ws_store_destroy(store_); }
  DeviceGlobalMap(const DeviceGlobalMap &) = delete;
  DeviceGlobalMap &operator=(const DeviceGlobalMap &) = delete;
  ws_store *handle() { return store_; }
  void reserve(uint64_t chunks) { WS_CHECK(ws_store_reserve(store_, chunks)); }
  size_t count() const
  {
    uint64_t n = 0;
    WS_CHECK(ws_store_count(store_, &n, nullptr));
    return (size_t)n;
  }
  std::vector<Key> keys() const // ascending (cx, cy, cz)
  {
    size_t n = 0;
    WS_CHECK(ws_store_keys(store_, nullptr, 0, &n));
    std::vector<int32_t> flat(3 * n);
    WS_CHECK(ws_store_keys(store_, flat.data(), n, &n));
    std::vector<Key> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = Key{flat[3 * i], flat[3 * i + 1], flat[3 * i + 2]};
    return out;
  }
  bool has_chunk(const Key &c) const { return ws_store_has(store_, c.data()) != 0; }
  bool chunk(const Key &c, std::vector<TSDFEntry::RawType> &out) // false: the store does not hold it
  {
    out.resize(CHUNK_WORDS);
    int32_t found = 0;
    WS_CHECK(ws_store_get_chunk(store_, c.data(), out.data(), &found));
    return found != 0;
  }
  void put_chunk(const Key &c, const std::vector<TSDFEntry::RawType> &data)
  {
    if (data.size() != CHUNK_WORDS) throw std::invalid_argument("DeviceGlobalMap::put_chunk: a chunk is 64^3 entries");
    WS_CHECK(ws_store_put_chunk(store_, c.data(), data.data()));
  }
  void drop_chunk(const Key &c) { WS_CHECK(ws_store_drop_chunk(store_, c.data())); }
  // the distance field of the chunks (visualization.hpp, ws_store_distance)
  DistanceField distance(int32_t max_dist_vox, bool unknown_occupied = false, bool columns = false, bool any_weight = false, const rm::Pointi *lo = nullptr,
                         const rm::Pointi *hi = nullptr)
  {
    return global_map_distance(store_, max_dist_vox, unknown_occupied, columns, any_weight, lo, hi);
  }
  // the ground layer of the chunks, and the column distance field over it (visualization.hpp, ws_store_ground, ws_store_ground_distance)
  GroundLayer ground(int32_t clear_vox, bool any_weight = false, bool unknown_headroom = false, bool top = false, const rm::Pointi *lo = nullptr,
                     const rm::Pointi *hi = nullptr)
  {
    return global_map_ground(store_, clear_vox, any_weight, unknown_headroom, top, lo, hi);
  }
  DistanceField ground_distance(int32_t max_step_q8, int32_t max_dist_vox, bool unknown_occupied = false)
  {
    return global_map_ground_distance(store_, max_step_q8, max_dist_vox, unknown_occupied);
  }
  // where the chunks' known world ends (visualization.hpp, ws_store_frontier)
  Frontier frontier(bool clusters = true, int32_t min_value = 0, bool any_weight = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    return global_map_frontier(store_, clusters, min_value, any_weight, lo, hi);
  }
  // what the sensor would see from candidate poses, through the chunks (visualization.hpp, ws_store_view_gain)
  ViewGain view_gain(int resolution, const std::vector<rm::Pointi> &origins, const std::vector<rm::Pointi> &dirs, int32_t max_range_mm, int32_t min_value = 0,
                     bool any_weight = false, bool with_rays = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    return global_map_view_gain(store_, resolution, origins, dirs, max_range_mm, min_value, any_weight, with_rays, lo, hi);
  }
  // candidate trajectories against the last distance() or ground_distance() of the chunks (visualization.hpp, ws_store_clearance)
  Clearance clearance(int resolution, const std::vector<ClearanceInput> &poses, size_t n_poses, const std::vector<ClearanceSphere> &body, int32_t soft_mm = 0,
                      bool per_pose = false, bool outside_ok = false)
  {
    return global_map_clearance(store_, resolution, poses, n_poses, body, soft_mm, per_pose, outside_ok);
  }
  // path costs over the last distance() of the chunks, and the paths back from goals (visualization.hpp, ws_store_reach)
  ReachField reach(const std::vector<rm::Pointi> &seeds, int32_t clear_d2 = 0, bool unknown_free = false, uint32_t max_rounds = 0)
  {
    return global_map_reach(store_, seeds, clear_d2, unknown_free, max_rounds);
  }
  ReachPaths reach_paths(const std::vector<rm::Pointi> &goals, uint32_t cap_steps) { return global_map_reach_paths(store_, goals, cap_steps); }
  // what the chunks say at given points (visualization.hpp, ws_store_sample)
  PointSample sample(int resolution, const std::vector<rm::Pointi> &points, int32_t band_mm, bool any_weight = false, bool with_gradient = false, uint32_t select = 0,
                     const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    return global_map_sample(store_, resolution, points, band_mm, any_weight, with_gradient, select, lo, hi);
  }
  // `other` resampled on this map's lattice under the pull transform and integrated into it (ws_store_fuse); resolution: the
  // maps', in mm per voxel, which a store does not know -- the contract of the Python DeviceGlobalMap.fuse
  FuseStats fuse(DeviceGlobalMap &other, const FusePose &pose, int max_weight, bool count_only, int resolution)
  {
    uint64_t s[6] = {0, 0, 0, 0, 0, 0};
    WS_CHECK(ws_store_fuse(store_, other.store_, &pose, resolution, max_weight, count_only ? WS_FUSE_COUNT_ONLY : WS_FUSE_DEFAULT, s));
    FuseStats out;
    out.candidates = s[0], out.created = s[1], out.averaged = s[2], out.set = s[3], out.sum_abs_diff = s[4], out.sum_min_weight = s[5];
    return out;
  }
  // Where this map ("now") differs from `ref` ("before") under the pull transform (ws_store_changes): band and free_value are raw
  // values, kinds WS_CHANGES_APPEARED | WS_CHANGES_VANISHED; resolution: the maps', in mm per voxel -- the contract of the Python
  // DeviceGlobalMap.changes.  Both maps are only read
  Changes changes(DeviceGlobalMap &ref, const FusePose &pose, int resolution, int band, int free_value, int min_weight = 1, uint32_t kinds = WS_CHANGES_DEFAULT,
                  bool clusters = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    Changes out;
    size_t n = 0, k = 0;
    uint64_t s[6] = {0, 0, 0, 0, 0, 0};
    const uint32_t flags = (kinds & WS_CHANGES_DEFAULT) | (clusters ? WS_CHANGES_CLUSTERS : 0u);
    WS_CHECK(ws_store_changes(store_, ref.store_, &pose, resolution, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, band, free_value, min_weight, flags, &n, &k, s));
    out.records.resize(n);
    if (clusters) out.labels.resize(n), out.clusters.resize(k);
    size_t got = 0, got_k = 0;
    WS_CHECK(ws_store_changes_download(store_, n ? out.records.data() : nullptr, n && clusters ? out.labels.data() : nullptr,
                                       k && clusters ? out.clusters.data() : nullptr, n, clusters ? k : 0, &got, &got_k));
    if (got != n || (clusters && got_k != k)) throw std::runtime_error("DeviceGlobalMap::changes: another call replaced the result before it was downloaded");
    out.stats.chunks = s[0], out.stats.known_both = s[1], out.stats.appeared = s[2], out.stats.vanished = s[3], out.stats.new_ground = s[4], out.stats.sum_abs_diff = s[5];
    return out;
  }
  // this map at half the resolution into `dst` (ws_store_coarsen): the chunks `keys` of dst rebuilt whole, nullptr: the parents of
  // every chunk of this map; with_stats = false returns after enqueueing with zero statistics -- the contract of the Python
  // DeviceGlobalMap.coarsen
  CoarsenStats coarsen(DeviceGlobalMap &dst, const std::vector<Key> *keys = nullptr, int min_observed = 8, bool with_stats = true)
  {
    uint64_t s[4] = {0, 0, 0, 0};
    const int32_t *k = keys && !keys->empty() ? (*keys)[0].data() : nullptr;
    const int32_t none[3] = {0, 0, 0}; // (an empty list is not "every parent")
    WS_CHECK(ws_store_coarsen(dst.store_, store_, keys ? (k ? k : none) : nullptr, keys ? keys->size() : 0, min_observed, WS_COARSEN_DEFAULT, with_stats ? s : nullptr));
    CoarsenStats out;
    out.chunks = s[0], out.created = s[1], out.valued = s[2], out.short_of = s[3];
    return out;
  }
  // Chunks of this map in packed form, made on the device (ws_store_pack): the chunks `keys` names (nullptr: every chunk) in
  // ascending key order; download = false leaves the payload on the device (ws_store_pack_payload_dev, valid until the next pack) --
  // the contract of the Python DeviceGlobalMap.pack.  This map is only read
  PackedMap pack(const std::vector<Key> *keys = nullptr, bool download = true)
  {
    PackedMap out;
    out.fill = fill();
    if (keys && keys->empty()) return out; // (an empty list is not "every chunk")
    size_t n = 0;
    uint64_t s[4] = {0, 0, 0, 0};
    WS_CHECK(ws_store_pack(store_, keys ? (*keys)[0].data() : nullptr, keys ? keys->size() : 0, WS_PACK_DEFAULT, &n, &out.payload_words, s));
    out.headers.resize(n * WS_PACK_HEADER_WORDS);
    if (download) out.payload.resize((size_t)out.payload_words);
    size_t got = 0;
    uint64_t got_w = 0;
    WS_CHECK(ws_store_pack_download(store_, n ? out.headers.data() : nullptr, download && out.payload_words ? out.payload.data() : nullptr, n,
                                    download ? out.payload_words : 0, &got, &got_w));
    if (got != n || got_w != out.payload_words) throw std::runtime_error("DeviceGlobalMap::pack: another call replaced the result before it was downloaded");
    out.default_bricks = s[0], out.uniform_bricks = s[1], out.dense_bricks = s[2], out.bytes = s[3];
    return out;
  }
  // the chunks of `p` created or overwritten whole, default bricks with p.fill (ws_store_unpack); the others keep their bytes
  void unpack(const PackedMap &p)
  {
    if (p.payload.size() != p.payload_words) throw std::invalid_argument("DeviceGlobalMap::unpack: the payload is not on the host");
    WS_CHECK(ws_store_unpack(store_, p.headers.data(), p.payload.data(), p.n_chunks(), p.payload_words, p.fill, 0));
  }
  // ... from a payload in device memory (ws_store_unpack_dev): stream-ordered, no wait
  void unpack_dev(const PackedMap &p, const uint32_t *payload_dev)
  {
    WS_CHECK(ws_store_unpack_dev(store_, p.headers.data(), payload_dev, p.n_chunks(), p.payload_words, p.fill, 0));
  }
  // a byte-exact copy of this map into `other` (its listed chunks are overwritten): pack, then unpack from the payload where it lies
  // on the device; only the headers visit the host.  Returns after the copy has run
  void clone_into(DeviceGlobalMap &other)
  {
    const PackedMap p = pack(nullptr, false);
    other.unpack_dev(p, ws_store_pack_payload_dev(store_, nullptr));
    WS_CHECK(ws_sync(cuda::detail::context()));
  }
  std::unique_ptr<DeviceGlobalMap> clone()
  {
    std::unique_ptr<DeviceGlobalMap> other(new DeviceGlobalMap(TSDFEntry(fill()), 0, 0));
    clone_into(*other);
    return other;
  }
  uint32_t fill() const { return fill_; }
  // every chunk merged into the host global map (and through it into its file)
  void flush_to(GlobalMap &g)
  {
    std::vector<TSDFEntry::RawType> data;
    for (const Key &c : keys())
      if (chunk(c, data)) g.put_chunk(c, data);
  }

private:
  ws_store *store_ = nullptr;
  uint32_t fill_ = 0;
};
// the surface cloud of the device global map (visualization.hpp, ws_store_surface)
inline SurfaceCloud global_map_cloud(DeviceGlobalMap &g, int tau, int resolution, bool marker = true, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr,
                                     int band = 0)
{
  return global_map_cloud(g.handle(), tau, resolution, marker, lo, hi, band);
}

// the frontier of the device global map (visualization.hpp, ws_store_frontier)
inline Frontier global_map_frontier(DeviceGlobalMap &g, bool clusters = true, int32_t min_value = 0, bool any_weight = false, const rm::Pointi *lo = nullptr,
                                    const rm::Pointi *hi = nullptr)
{
  return global_map_frontier(g.handle(), clusters, min_value, any_weight, lo, hi);
}

// the view gain of the device global map (visualization.hpp, ws_store_view_gain)
inline ViewGain global_map_view_gain(DeviceGlobalMap &g, int resolution, const std::vector<rm::Pointi> &origins, const std::vector<rm::Pointi> &dirs, int32_t max_range_mm,
                                     int32_t min_value = 0, bool any_weight = false, bool with_rays = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
{
  return global_map_view_gain(g.handle(), resolution, origins, dirs, max_range_mm, min_value, any_weight, with_rays, lo, hi);
}

// the clearance of the device global map (visualization.hpp, ws_store_clearance)
inline Clearance global_map_clearance(DeviceGlobalMap &g, int resolution, const std::vector<ClearanceInput> &poses, size_t n_poses, const std::vector<ClearanceSphere> &body,
                                      int32_t soft_mm = 0, bool per_pose = false, bool outside_ok = false)
{
  return global_map_clearance(g.handle(), resolution, poses, n_poses, body, soft_mm, per_pose, outside_ok);
}

// the reach of the device global map and its paths (visualization.hpp, ws_store_reach)
inline ReachField global_map_reach(DeviceGlobalMap &g, const std::vector<rm::Pointi> &seeds, int32_t clear_d2 = 0, bool unknown_free = false, uint32_t max_rounds = 0)
{
  return global_map_reach(g.handle(), seeds, clear_d2, unknown_free, max_rounds);
}
inline ReachPaths global_map_reach_paths(DeviceGlobalMap &g, const std::vector<rm::Pointi> &goals, uint32_t cap_steps)
{
  return global_map_reach_paths(g.handle(), goals, cap_steps);
}

// the mesh of the device global map (visualization.hpp, ws_store_mesh)
inline SurfaceMesh global_map_mesh(DeviceGlobalMap &g, int resolution, bool any_weight = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
{
  return global_map_mesh(g.handle(), resolution, any_weight, lo, hi);
}

// the ray cast of the device global map (visualization.hpp, ws_store_raycast)
inline RayCast global_map_raycast(DeviceGlobalMap &g, int resolution, const rm::Pointi &origin_mm, const std::vector<rm::Pointi> &dirs, int32_t max_range_mm,
                                  bool any_weight = false, bool with_gradient = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr, bool targets = false)
{
  return global_map_raycast(g.handle(), resolution, origin_mm, dirs, max_range_mm, any_weight, with_gradient, lo, hi, targets);
}

// the point sample of the device global map (visualization.hpp, ws_store_sample)
inline PointSample global_map_sample(DeviceGlobalMap &g, int resolution, const std::vector<rm::Pointi> &points, int32_t band_mm, bool any_weight = false,
                                     bool with_gradient = false, uint32_t select = 0, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
{
  return global_map_sample(g.handle(), resolution, points, band_mm, any_weight, with_gradient, select, lo, hi);
}

// ---------------------------------------------------------------------------------------------------- MapPyramid
// `levels` coarser copies of a DeviceGlobalMap, each with twice the voxel edge of the one below (DeviceGlobalMap::coarsen) -- the
// contract of the Python MapPyramid.  store(0) is the base, which the pyramid does not own; store(l) is queried like any
// DeviceGlobalMap with resolution(l) = resolution << l.  The levels follow the base only when rebuild() or refresh() is called.
class MapPyramid
{
public:
  using Key = DeviceGlobalMap::Key;
  MapPyramid(DeviceGlobalMap &base, int levels, int resolution, const TSDFEntry &default_entry, int min_observed = 8, uint32_t segment_chunks = 0)
      : base_(base), resolution_(resolution), min_observed_(min_observed)
  {
    if (levels < 1) throw std::invalid_argument("MapPyramid: levels must be at least 1");
    for (int l = 0; l < levels; ++l) stores_.emplace_back(new DeviceGlobalMap(default_entry, 0, segment_chunks));
  }
  int levels() const { return (int)stores_.size(); }
  int min_observed() const { return min_observed_; }
  DeviceGlobalMap &store(int level) { return level == 0 ? base_ : *stores_.at((size_t)level - 1); }
  int resolution(int level) const { return resolution_ << level; }
  // every level from the one below, over the parents of all its chunks
  std::vector<CoarsenStats> rebuild(bool with_stats = true)
  {
    std::vector<CoarsenStats> out;
    for (int l = 1; l <= levels(); ++l) out.push_back(store(l - 1).coarsen(store(l), nullptr, min_observed_, with_stats));
    return out;
  }
  // after a change of the base inside the inclusive box [lo, hi] of base voxels: level 1 recomputes the parents of the chunks the box
  // overlaps, every level above the parents of those; nothing else is touched
  std::vector<CoarsenStats> refresh(const rm::Pointi &lo, const rm::Pointi &hi, bool with_stats = true)
  {
    size_t n = 0;
    WS_CHECK(ws_store_chunks_of_box(&lo.x, &hi.x, nullptr, 0, &n));
    std::vector<Key> keys(n);
    WS_CHECK(ws_store_chunks_of_box(&lo.x, &hi.x, keys[0].data(), n, &n));
    std::vector<CoarsenStats> out;
    for (int l = 1; l <= levels(); ++l)
    {
      keys = parents_of(keys);
      out.push_back(store(l - 1).coarsen(store(l), &keys, min_observed_, with_stats));
    }
    return out;
  }

private:
  DeviceGlobalMap &base_;
  int resolution_, min_observed_;
  std::vector<std::unique_ptr<DeviceGlobalMap>> stores_;
};

// ---------------------------------------------------------------------------------------------------- LocalMap
// The in-memory state of HDF5LocalMap (hdf5_local_map.cpp:5-20): odd sizes, offset = size / 2, default-filled.
class LocalMap
{
public:
  LocalMap(int sx, int sy, int sz, GlobalMap &map)
      : size_(sx % 2 ? sx : sx + 1, sy % 2 ? sy : sy + 1, sz % 2 ? sz : sz + 1), pos_(0, 0, 0), offset_(size_.x / 2, size_.y / 2, size_.z / 2),
        map_(map), data_((size_t)size_.x * size_.y * size_.z, map.get_default_tsdf_entry())
  {
  }
  rm::Pointi &get_size() { return size_; }
  rm::Pointi &get_pos() { return pos_; }
  rm::Pointi &get_offset() { return offset_; }
  std::vector<TSDFEntry> &data() { return data_; }
  GlobalMap &global_map() { return map_; }
  bool in_bounds(int x, int y, int z) const
  {
    return std::abs(x - pos_.x) <= size_.x / 2 && std::abs(y - pos_.y) <= size_.y / 2 && std::abs(z - pos_.z) <= size_.z / 2;
  }
  TSDFEntry &value(int x, int y, int z)
  {
    if (!in_bounds(x, y, z)) throw std::out_of_range("Index out of bounds"); // hdf5_local_map.h:172-181
    const size_t xi = (size_t)((x - pos_.x + offset_.x + size_.x) % size_.x), yi = (size_t)((y - pos_.y + offset_.y + size_.y) % size_.y),
                 zi = (size_t)((z - pos_.z + offset_.z + size_.z) % size_.z);
    return data_[(xi * size_.y + yi) * size_.z + zi];
  }
  // the window in world voxels, every ring cell once: pos - size/2 .. pos - size/2 + size - 1 (ws_shift_plan's window)
  void window(rm::Pointi &lo, rm::Pointi &hi) const
  {
    lo = rm::Pointi(pos_.x - size_.x / 2, pos_.y - size_.y / 2, pos_.z - size_.z / 2);
    hi = rm::Pointi(lo.x + size_.x - 1, lo.y + size_.y - 1, lo.z + size_.z - 1);
  }
  // pos / offset after a shift the device has made (the data is not touched)
  void follow(const rm::Pointi &new_pos)
  {
    const int *sz = &size_.x, *np = &new_pos.x;
    int *ps = &pos_.x, *of = &offset_.x;
    for (int k = 0; k < 3; ++k)
    {
      of[k] = (int)((((int64_t)of[k] + np[k] - ps[k]) % sz[k] + sz[k]) % sz[k]);
      ps[k] = np[k];
    }
  }

private:
  rm::Pointi size_, pos_, offset_;
  GlobalMap &map_;
  std::vector<TSDFEntry> data_;
};

// ---------------------------------------------------------------------------------------------------- MappingNode
// cuda::TSDFRegistration plus the map-shift / export side of cuda::TSDFMapping, with the window moved ON THE DEVICE.
class MappingNode
{
public:
  MappingNode(const cuda::HotPathParams &params, LocalMap &local_map)
      : params_(params), local_map_(local_map), view_(&local_map.get_size(), &local_map.get_offset(), local_map.data().data(), &local_map.get_pos()),
        gpu_(params, view_)
  {
  }
  cuda::TSDFRegistration &gpu() { return gpu_; }
  // the global map in device memory: shift_map_device and write_back go through it from now on (nullptr: detach)
  void attach(DeviceGlobalMap *device_global_map) { device_global_map_ = device_global_map; }

  // The shift with the global map in device memory (ws_shift_device): per axis the leaving slab goes into the store's chunks,
  // pos / offset of both maps move, the entering slab comes out of them -- revisits and corners included -- in stream order.
  // No transfer, no staging, no worker; returns after enqueueing.
  void shift_map_device(const rm::Pointi &new_pos)
  {
    if (!device_global_map_) throw std::logic_error("shift_map_device: no DeviceGlobalMap attached");
    wait_shift();
    pyramid_touch(); // (the leaving slabs go into chunks that global_pyramid has to refresh)
    WS_CHECK(ws_shift_device(gpu_.tsdf().handle(), device_global_map_->handle(), &new_pos.x));
    local_map_.follow(new_pos);
  }

  // TSDFMapping::map_shift body (tsdf_mapping.cpp:109-126) == HDF5LocalMap::shift (hdf5_local_map.cpp:53-118) per axis:
  // save the slab that leaves, move pos/offset, load the slab that enters -- each slab packed / unpacked by the GPU.
  void shift_map(const rm::Pointi &new_pos)
  {
    wait_shift();
    auto &avg = gpu_.tsdf().avg_map();
    auto &fresh = gpu_.tsdf().new_map();
    GlobalMap &gm = local_map_.global_map();
    ws_shift_plan_t plan;
    if (ws_shift_plan(&local_map_.get_size().x, &local_map_.get_pos().x, &local_map_.get_offset().x, &new_pos.x, &plan) != WS_OK)
      throw std::out_of_range("shift_map: further than one window");
    const auto point = [](const int32_t v[3]) { return rm::Pointi(v[0], v[1], v[2]); };
    std::vector<TSDFEntry> slab;
    for (int i = 0; i < plan.n; ++i)
    {
      avg.extract_box(point(plan.leave_lo[i]), point(plan.leave_hi[i]), slab);
      gm.save_box(point(plan.leave_lo[i]), point(plan.leave_hi[i]), slab);
      rm::Pointi step = local_map_.get_pos();
      (&step.x)[plan.axis[i]] += plan.d[i];
      local_map_.follow(step);
      avg.update_params(view_);
      fresh.update_params(view_); // new_map is (tau, 0) everywhere: only its window moves
      gm.load_box(point(plan.enter_lo[i]), point(plan.enter_hi[i]), slab);
      avg.insert_box(point(plan.enter_lo[i]), point(plan.enter_hi[i]), slab);
    }
  }

  // The same shift the way the reference runs it — off the scan path (its own thread, tsdf_mapping.cpp:97-136): the
  // window moves by device kernels inside this call (ws_shift_begin: pack the leaving slabs, move pos/offset, fill the
  // entering slabs with the default entry; nothing waits), chunks the global map already holds for the entering slabs are
  // uploaded (revisits only), and a worker thread files the leaving slabs into the global map once their copy to pinned
  // memory has landed.  Same maps as shift_map().
  // staging for asynchronous shifts of up to `shift_voxels` per axis (plus slack), allocated now instead of inside the first
  // shift: a pinned allocation of that size takes tens of milliseconds (56 ms of the first shifting scan of the 1025^3 stream)
  void reserve_shift(int shift_voxels)
  {
    const rm::Pointi &size = local_map_.get_size();
    const uint64_t d = (uint64_t)(shift_voxels > 0 ? shift_voxels : 0) + 8u;
    WS_CHECK(ws_shift_reserve(gpu_.tsdf().handle(), d * ((uint64_t)size.x * size.y + (uint64_t)size.y * size.z + (uint64_t)size.x * size.z)));
  }
  void shift_map_async(const rm::Pointi &new_pos)
  {
    wait_shift();
    auto &avg = gpu_.tsdf().avg_map();
    ws_shift *ticket = nullptr;
    WS_CHECK(ws_shift_begin(gpu_.tsdf().handle(), &new_pos.x, local_map_.global_map().get_default_tsdf_entry().raw(), &ticket));
    // Between ws_shift_begin and the start of the worker, loading the entering boxes can throw: the window has moved on the
    // device by then, so the leaving slabs are still filed (synchronously, by this guard) and the ticket is closed -- an
    // open ticket would make every later ws_shift_begin fail.
    GlobalMap *gm = &local_map_.global_map();
    std::string *err = &shift_error_;
    struct Owner
    {
      ws_shift *t;
      int n;
      GlobalMap *gm;
      std::string *err;
      bool armed;
      ~Owner()
      {
        if (armed) file_leaving_slabs(t, n, gm, err);
      }
    } owner{ticket, ws_shift_count(ticket), gm, err, true};
    local_map_.follow(new_pos);
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    const int n = ws_shift_count(ticket), cs = GlobalMap::CHUNK_SIZE;
    std::vector<TSDFEntry> part;
    for (int i = 0; i < n; ++i)
    {
      int lo[3], hi[3];
      WS_CHECK(ws_shift_entering(ticket, i, lo, hi));
      for (int k = 0; k < 3; ++k) // only what is still inside the final window
      {
        lo[k] = std::max(lo[k], (&wlo.x)[k]);
        hi[k] = std::min(hi[k], (&whi.x)[k]);
      }
      if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) continue;
      for (int cx = floor_div(lo[0], cs); cx <= floor_div(hi[0], cs); ++cx)
        for (int cy = floor_div(lo[1], cs); cy <= floor_div(hi[1], cs); ++cy)
          for (int cz = floor_div(lo[2], cs); cz <= floor_div(hi[2], cs); ++cz)
          {
            if (!local_map_.global_map().has_chunk(GlobalMap::Key{cx, cy, cz})) continue;
            const rm::Pointi a(std::max(lo[0], cx * cs), std::max(lo[1], cy * cs), std::max(lo[2], cz * cs)),
                b(std::min(hi[0], cx * cs + cs - 1), std::min(hi[1], cy * cs + cs - 1), std::min(hi[2], cz * cs + cs - 1));
            local_map_.global_map().load_box(a, b, part);
            avg.insert_box(a, b, part);
          }
    }
    shift_error_.clear();
    owner.armed = false; // from here on the worker owns the ticket
    shift_worker_ = std::thread(file_leaving_slabs, ticket, n, gm, err);
  }
  // The leaving slabs of an asynchronous shift -> the global map; closes the ticket whatever happens (an open ticket makes
  // the next ws_shift_begin fail), and a failure -- a HIP error while waiting for the slabs, an exception out of the global
  // map -- is kept for wait_shift() instead of being swallowed or ending the process through std::terminate.
  static void file_leaving_slabs(ws_shift *ticket, int n, GlobalMap *gm, std::string *err)
  {
    struct Closer
    {
      ws_shift *t;
      ~Closer() { ws_shift_end(t); }
    } closer{ticket};
    try
    {
      if (ws_shift_wait(ticket) != WS_OK)
      {
        *err = std::string("ws_shift_wait: ") + ws_last_error();
        return;
      }
      std::vector<TSDFEntry> own;
      for (int i = 0; i < n; ++i)
      {
        int lo[3], hi[3];
        const uint32_t *data = nullptr;
        if (ws_shift_slab(ticket, i, lo, hi, &data) != WS_OK) continue;
        TSDFEntry *box = reinterpret_cast<TSDFEntry *>(const_cast<uint32_t *>(data));
        const size_t ey = (size_t)(hi[1] - lo[1] + 1), ez = (size_t)(hi[2] - lo[2] + 1);
        // a corner that entered with an earlier axis of this shift and leaves with this one was packed as default fill:
        // put the global map's own data there, so that saving the slab changes nothing for it
        for (int j = 0; j < i; ++j)
        {
          int elo[3], ehi[3];
          if (ws_shift_entering(ticket, j, elo, ehi) != WS_OK) continue;
          int a[3], b[3];
          bool any = true;
          for (int k = 0; k < 3; ++k)
          {
            a[k] = std::max(lo[k], elo[k]);
            b[k] = std::min(hi[k], ehi[k]);
            any = any && a[k] <= b[k];
          }
          if (!any) continue;
          gm->load_box(rm::Pointi(a[0], a[1], a[2]), rm::Pointi(b[0], b[1], b[2]), own);
          const size_t oy = (size_t)(b[1] - a[1] + 1), oz = (size_t)(b[2] - a[2] + 1);
          for (int x = a[0]; x <= b[0]; ++x)
            for (int y = a[1]; y <= b[1]; ++y)
              for (int z = a[2]; z <= b[2]; ++z)
                box[((size_t)(x - lo[0]) * ey + (size_t)(y - lo[1])) * ez + (size_t)(z - lo[2])] =
                    own[((size_t)(x - a[0]) * oy + (size_t)(y - a[1])) * oz + (size_t)(z - a[2])];
        }
        gm->save_box(rm::Pointi(lo[0], lo[1], lo[2]), rm::Pointi(hi[0], hi[1], hi[2]), box);
      }
    }
    catch (const std::exception &e)
    {
      *err = std::string("filing the leaving slabs: ") + e.what();
    }
    catch (...)
    {
      *err = "filing the leaving slabs: unknown exception";
    }
  }
  // joins the worker of the last asynchronous shift; throws if its slabs did not reach the global map
  void wait_shift()
  {
    if (shift_worker_.joinable()) shift_worker_.join();
    if (!shift_error_.empty())
    {
      const std::string msg = "asynchronous map shift failed: " + shift_error_;
      shift_error_.clear();
      throw std::runtime_error(msg);
    }
  }
  ~MappingNode()
  {
    if (shift_worker_.joinable()) shift_worker_.join(); // (a destructor does not throw; the error was the caller's to collect)
  }

  // HDF5LocalMap::write_back + HDF5GlobalMap::write_back (hdf5_local_map.cpp:210-217, app.cpp:215-221) from the device map
  // box_lo / box_hi (inclusive world voxels, either may be null) restrict the export to a part of the window
  void write_back(const rm::Pointi *box_lo = nullptr, const rm::Pointi *box_hi = nullptr)
  {
    wait_shift();
    auto &avg = gpu_.tsdf().avg_map();
    const int cs = GlobalMap::CHUNK_SIZE;
    rm::Pointi lo, hi;
    local_map_.window(lo, hi);
    if (box_lo) lo = rm::Pointi(std::max(lo.x, box_lo->x), std::max(lo.y, box_lo->y), std::max(lo.z, box_lo->z));
    if (box_hi) hi = rm::Pointi(std::min(hi.x, box_hi->x), std::min(hi.y, box_hi->y), std::min(hi.z, box_hi->z));
    if (lo.x > hi.x || lo.y > hi.y || lo.z > hi.z) return; // the box misses the window
    if (device_global_map_)
    {
      // the window into the device chunks in one launch, the chunks into the host map, the host map into its file
      WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &lo.x, &hi.x));
      device_global_map_->flush_to(local_map_.global_map());
      local_map_.global_map().write_back();
      return;
    }
    std::vector<TSDFEntry> slab;
    for (int cx = floor_div(lo.x, cs); cx <= floor_div(hi.x, cs); ++cx)
    {
      const rm::Pointi a(std::max(lo.x, cx * cs), lo.y, lo.z), b(std::min(hi.x, cx * cs + cs - 1), hi.y, hi.z);
      avg.extract_box(a, b, slab);
      local_map_.global_map().save_box(a, b, slab);
    }
    local_map_.global_map().write_back();
  }
  // The mesh of everything the run has seen: the window into the device chunks (the first step of write_back, with its capacity
  // refusals), then the mesh of the store -- nothing leaves the device but the mesh
  SurfaceMesh global_mesh(bool any_weight = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    if (!device_global_map_) throw std::logic_error("global_mesh: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return global_map_mesh(*device_global_map_, params_.map_resolution, any_weight, lo, hi);
  }
  // The surface cloud of everything the run has seen: the window into the device chunks, as global_mesh does, then the cloud of the
  // store -- nothing leaves the device but the records
  SurfaceCloud global_surface(bool marker = true, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr, int band = 0)
  {
    if (!device_global_map_) throw std::logic_error("global_surface: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return global_map_cloud(*device_global_map_, params_.tau, params_.map_resolution, marker, lo, hi, band);
  }
  // The predicted scan from anywhere the run has been: the window into the device chunks, as global_mesh does, then the ray cast of
  // the store -- nothing leaves the device but the records
  RayCast global_raycast(const rm::Pointi &origin_mm, const std::vector<rm::Pointi> &dirs, int32_t max_range_mm, bool any_weight = false, bool with_gradient = false,
                         const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr, bool targets = false)
  {
    if (!device_global_map_) throw std::logic_error("global_raycast: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return global_map_raycast(*device_global_map_, params_.map_resolution, origin_mm, dirs, max_range_mm, any_weight, with_gradient, lo, hi, targets);
  }
  // What the averaged map says at map-frame points in millimetres (local_map_sample); band_mm <= 0: tau
  PointSample sample(const std::vector<rm::Pointi> &points, int32_t band_mm = 0, bool any_weight = false, bool with_gradient = false, uint32_t select = 0)
  {
    return local_map_sample(gpu_.tsdf(), points, band_mm, any_weight, with_gradient, select);
  }
  // The same of everything the run has seen: the window into the device chunks, as global_mesh does, then the sample of the store.
  // band_mm <= 0: tau
  PointSample global_sample(const std::vector<rm::Pointi> &points, int32_t band_mm = 0, bool any_weight = false, bool with_gradient = false, uint32_t select = 0,
                            const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    if (!device_global_map_) throw std::logic_error("global_sample: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return global_map_sample(*device_global_map_, params_.map_resolution, points, band_mm > 0 ? band_mm : params_.tau, any_weight, with_gradient, select, lo, hi);
  }
  // The cost map of everything the run has seen: the window into the device chunks, as global_mesh does, then the distance field of
  // the store -- nothing leaves the device but the records
  DistanceField global_distance(int32_t max_dist_vox, bool unknown_occupied = false, bool columns = false, bool any_weight = false, const rm::Pointi *lo = nullptr,
                                const rm::Pointi *hi = nullptr)
  {
    if (!device_global_map_) throw std::logic_error("global_distance: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return device_global_map_->distance(max_dist_vox, unknown_occupied, columns, any_weight, lo, hi);
  }
  // The ground layer of the averaged map (local_map_ground): one level per column under clear_vox voxels of headroom
  GroundLayer ground(int32_t clear_vox, bool any_weight = false, bool unknown_headroom = false, bool top = false, const rm::Pointi *lo = nullptr,
                     const rm::Pointi *hi = nullptr)
  {
    return local_map_ground(gpu_.tsdf(), clear_vox, any_weight, unknown_headroom, top, lo, hi);
  }
  // The same of everything the run has seen: the window into the device chunks, as global_mesh does, then the ground of the store
  GroundLayer global_ground(int32_t clear_vox, bool any_weight = false, bool unknown_headroom = false, bool top = false, const rm::Pointi *lo = nullptr,
                            const rm::Pointi *hi = nullptr)
  {
    if (!device_global_map_) throw std::logic_error("global_ground: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return device_global_map_->ground(clear_vox, any_weight, unknown_headroom, top, lo, hi);
  }
  // Where the window's known free space ends (local_map_frontier on the averaged map)
  Frontier frontier(bool clusters = true, int32_t min_value = 0, bool any_weight = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    return local_map_frontier(gpu_.tsdf(), WS_MAP_AVG, clusters, min_value, any_weight, lo, hi);
  }
  // The frontier of everything the run has seen: the window into the device chunks, as global_mesh does, then the frontier of the
  // store.  Without a box: the bounding box of the chunks grown by one voxel on every side (cut to int32), so that the outer faces of
  // the mapped volume are frontier too
  Frontier global_frontier(bool clusters = true, int32_t min_value = 0, bool any_weight = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    if (!device_global_map_) throw std::logic_error("global_frontier: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    if (lo || hi) return device_global_map_->frontier(clusters, min_value, any_weight, lo, hi);
    const std::vector<DeviceGlobalMap::Key> keys = device_global_map_->keys();
    if (keys.empty()) return device_global_map_->frontier(clusters, min_value, any_weight);
    int64_t a[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, b[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    for (const DeviceGlobalMap::Key &c : keys)
      for (int k = 0; k < 3; ++k) a[k] = std::min<int64_t>(a[k], c[k]), b[k] = std::max<int64_t>(b[k], c[k]);
    const int64_t cs = GlobalMap::CHUNK_SIZE;
    const auto cut = [](int64_t v) { return (int32_t)std::min<int64_t>(std::max<int64_t>(v, INT32_MIN), INT32_MAX); };
    const rm::Pointi glo(cut(a[0] * cs - 1), cut(a[1] * cs - 1), cut(a[2] * cs - 1)), ghi(cut((b[0] + 1) * cs), cut((b[1] + 1) * cs), cut((b[2] + 1) * cs));
    return device_global_map_->frontier(clusters, min_value, any_weight, &glo, &ghi);
  }
  // What the sensor would see from `origins` (map frame, mm) along the fan `dirs` in the averaged map (local_map_view_gain)
  ViewGain view_gain(const std::vector<rm::Pointi> &origins, const std::vector<rm::Pointi> &dirs, int32_t max_range_mm, int32_t min_value = 0, bool any_weight = false,
                     bool with_rays = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    return local_map_view_gain(gpu_.tsdf(), origins, dirs, max_range_mm, WS_MAP_AVG, min_value, any_weight, with_rays, lo, hi);
  }
  // Another map fused into everything the run has seen: the window into the device chunks, as global_mesh does, the fuse of the
  // store at the map's resolution (max_weight < 0: the map's), and, unless count_only, the window loaded back from the chunks, so
  // that it holds the merged voxels and a later save does not undo the merge
  FuseStats merge_map(DeviceGlobalMap &other, const FusePose &pose, int max_weight = -1, bool count_only = false)
  {
    if (!device_global_map_) throw std::logic_error("merge_map: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    const FuseStats st = device_global_map_->fuse(other, pose, max_weight < 0 ? params_.max_weight : max_weight, count_only, params_.map_resolution);
    if (!count_only) WS_CHECK(ws_store_load_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    if (!count_only) pyramid_all_ = true; // (the fuse wrote chunks anywhere: global_pyramid rebuilds)
    return st;
  }
  // Where everything the run has seen differs from an earlier map: the window into the device chunks, as global_mesh does, then
  // DeviceGlobalMap::changes at the map's resolution (band < 0: the resolution; free_value < 0: tau)
  Changes map_changes(DeviceGlobalMap &ref, const FusePose &pose, int band = -1, int free_value = -1, int min_weight = 1, uint32_t kinds = WS_CHANGES_DEFAULT,
                      bool clusters = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    if (!device_global_map_) throw std::logic_error("map_changes: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return device_global_map_->changes(ref, pose, params_.map_resolution, band < 0 ? params_.map_resolution : band, free_value < 0 ? params_.tau : free_value,
                                       min_weight, kinds, clusters, lo, hi);
  }
  // Everything the run has seen in packed form: the window into the device chunks, as global_mesh does, then DeviceGlobalMap::pack
  // (the `.wspk` file of such a stream is written by the Python PackedMap.save)
  PackedMap global_packed()
  {
    if (!device_global_map_) throw std::logic_error("global_packed: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return device_global_map_->pack();
  }
  // Coarser levels of everything the run has seen: the window into the device chunks, as global_mesh does, then a MapPyramid over the
  // store, rebuilt (the first call, other levels or min_observed, after merge_map) or refreshed over the windows the node has held
  // since the last call.  The node keeps the pyramid; chunks written into the store behind its back want MapPyramid::rebuild().
  MapPyramid &global_pyramid(int levels, int min_observed = 8, uint32_t segment_chunks = 0)
  {
    if (!device_global_map_) throw std::logic_error("global_pyramid: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    if (!pyramid_ || &pyramid_->store(0) != device_global_map_ || pyramid_->levels() != levels || pyramid_->min_observed() != min_observed)
    {
      pyramid_.reset(new MapPyramid(*device_global_map_, levels, params_.map_resolution, local_map_.global_map().get_default_tsdf_entry(), min_observed, segment_chunks));
      pyramid_all_ = true, pyramid_dirty_ = false;
    }
    pyramid_touch();
    if (pyramid_all_)
      pyramid_->rebuild(false);
    else
      pyramid_->refresh(dirty_lo_, dirty_hi_, false);
    pyramid_all_ = pyramid_dirty_ = false;
    return *pyramid_;
  }
  // The same through everything the run has seen: the window into the device chunks, as global_mesh does, then the view gain of the
  // store (without a box: the bounding box of the chunks)
  ViewGain global_view_gain(const std::vector<rm::Pointi> &origins, const std::vector<rm::Pointi> &dirs, int32_t max_range_mm, int32_t min_value = 0,
                            bool any_weight = false, bool with_rays = false, const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    if (!device_global_map_) throw std::logic_error("global_view_gain: no DeviceGlobalMap attached");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    return device_global_map_->view_gain(params_.map_resolution, origins, dirs, max_range_mm, min_value, any_weight, with_rays, lo, hi);
  }
  // How far every voxel of the window (or of [lo, hi]) is from `seeds` (world voxels) along free space that keeps clear_vox voxels
  // from the obstacles: the distance field with a range one voxel beyond the clearance, then local_map_reach on it
  ReachField reach(const std::vector<rm::Pointi> &seeds, int32_t clear_vox = 0, bool unknown_free = false, const rm::Pointi *lo = nullptr,
                   const rm::Pointi *hi = nullptr, bool columns = false, uint32_t max_rounds = 0)
  {
    if (clear_vox < 0 || clear_vox > 254) throw std::invalid_argument("reach: the clearance is 0 .. 254 voxels");
    WS_CHECK(ws_map_distance(gpu_.tsdf().handle(), WS_MAP_AVG, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, clear_vox + 1,
                             columns ? WS_DISTANCE_COLUMNS : WS_DISTANCE_DEFAULT, nullptr));
    return local_map_reach(gpu_.tsdf(), seeds, clear_vox * clear_vox, unknown_free, max_rounds);
  }
  // the same over everything the run has seen: the window into the device chunks, as global_mesh does, then distance and reach of the store
  ReachField global_reach(const std::vector<rm::Pointi> &seeds, int32_t clear_vox = 0, bool unknown_free = false, const rm::Pointi *lo = nullptr,
                          const rm::Pointi *hi = nullptr, bool columns = false, uint32_t max_rounds = 0)
  {
    if (!device_global_map_) throw std::logic_error("global_reach: no DeviceGlobalMap attached");
    if (clear_vox < 0 || clear_vox > 254) throw std::invalid_argument("reach: the clearance is 0 .. 254 voxels");
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    WS_CHECK(ws_store_distance(device_global_map_->handle(), lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, clear_vox + 1,
                               columns ? WS_DISTANCE_COLUMNS : WS_DISTANCE_DEFAULT, nullptr));
    return device_global_map_->reach(seeds, clear_vox * clear_vox, unknown_free, max_rounds);
  }
  // Candidate trajectories scored against the averaged map: the distance field of the window (or of [lo, hi]; columns: the 2-D field of
  // a ground robot) with a range of max_dist_vox voxels (0: the largest radius + soft_mm, rounded up, plus one), then local_map_clearance
  Clearance score_trajectories(const std::vector<ClearanceInput> &poses, size_t n_poses, const std::vector<ClearanceSphere> &body, int32_t soft_mm = 0,
                               bool columns = true, bool per_pose = false, bool outside_ok = false, int32_t max_dist_vox = 0, bool unknown_occupied = false,
                               const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    const uint32_t flags = (columns ? WS_DISTANCE_COLUMNS : 0u) | (unknown_occupied ? WS_DISTANCE_UNKNOWN_OCCUPIED : 0u);
    WS_CHECK(ws_map_distance(gpu_.tsdf().handle(), WS_MAP_AVG, lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, score_range(body, soft_mm, max_dist_vox), flags, nullptr));
    return local_map_clearance(gpu_.tsdf(), poses, n_poses, body, soft_mm, per_pose, outside_ok);
  }
  // the same over everything the run has seen: the window into the device chunks, as global_mesh does, then distance and clearance of the store
  Clearance global_score_trajectories(const std::vector<ClearanceInput> &poses, size_t n_poses, const std::vector<ClearanceSphere> &body, int32_t soft_mm = 0,
                                      bool columns = true, bool per_pose = false, bool outside_ok = false, int32_t max_dist_vox = 0, bool unknown_occupied = false,
                                      const rm::Pointi *lo = nullptr, const rm::Pointi *hi = nullptr)
  {
    if (!device_global_map_) throw std::logic_error("global_score_trajectories: no DeviceGlobalMap attached");
    const int32_t range = score_range(body, soft_mm, max_dist_vox);
    wait_shift();
    rm::Pointi wlo, whi;
    local_map_.window(wlo, whi);
    WS_CHECK(ws_store_save_box(device_global_map_->handle(), gpu_.tsdf().handle(), WS_MAP_AVG, &wlo.x, &whi.x));
    const uint32_t flags = (columns ? WS_DISTANCE_COLUMNS : 0u) | (unknown_occupied ? WS_DISTANCE_UNKNOWN_OCCUPIED : 0u);
    WS_CHECK(ws_store_distance(device_global_map_->handle(), lo ? &lo->x : nullptr, hi ? &hi->x : nullptr, range, flags, nullptr));
    return device_global_map_->clearance(params_.map_resolution, poses, n_poses, body, soft_mm, per_pose, outside_ok);
  }
  // the range of the distance call behind score_trajectories, in voxels
  int32_t score_range(const std::vector<ClearanceSphere> &body, int32_t soft_mm, int32_t max_dist_vox) const
  {
    int64_t need = 0;
    for (const ClearanceSphere &s : body) need = std::max<int64_t>(need, s.radius_mm);
    const int64_t res = params_.map_resolution, vox = max_dist_vox > 0 ? max_dist_vox : (need + soft_mm + res - 1) / res + 1;
    if (vox < 1 || vox > 255) throw std::invalid_argument("score_trajectories: the distance range must be 1 .. 255 voxels");
    return (int32_t)vox;
  }
  // the reference's route, kept for comparison: whole window to the host array of the local map
  void download() { gpu_.tsdf().avg_map().to_host(view_); }
  // publish_local_map's cloud of the averaged map (visualization/map.h:14-121), selected on the device: no whole-map download
  SurfaceCloud surface(bool marker = true) { return local_map_cloud(gpu_.tsdf(), WS_MAP_AVG, marker); }

private:
  // the present window joins the box that global_pyramid has to refresh
  void pyramid_touch()
  {
    if (!pyramid_) return;
    rm::Pointi lo, hi;
    local_map_.window(lo, hi);
    if (pyramid_dirty_)
    {
      lo = rm::Pointi(std::min(lo.x, dirty_lo_.x), std::min(lo.y, dirty_lo_.y), std::min(lo.z, dirty_lo_.z));
      hi = rm::Pointi(std::max(hi.x, dirty_hi_.x), std::max(hi.y, dirty_hi_.y), std::max(hi.z, dirty_hi_.z));
    }
    dirty_lo_ = lo, dirty_hi_ = hi, pyramid_dirty_ = true;
  }
  cuda::HotPathParams params_;
  LocalMap &local_map_;
  cuda::DeviceMap view_;
  cuda::TSDFRegistration gpu_;
  DeviceGlobalMap *device_global_map_ = nullptr;
  std::unique_ptr<MapPyramid> pyramid_; // global_pyramid's, with the box of base voxels that changed since it last ran
  bool pyramid_all_ = false, pyramid_dirty_ = false;
  rm::Pointi dirty_lo_, dirty_hi_;
  std::thread shift_worker_;
  std::string shift_error_; // written by the worker, read after join()
};

// ---------------------------------------------------------------------------------------------------- App
struct AppParams
{
  cuda::HotPathParams hot;
  float max_distance = 1.0f; // map/max_distance (m)
  float shift = 10.0f;       // map/shift (m)
  int map_size[3] = {513, 513, 513}; // voxels
  int initial_weight = 0;
  bool async_shift = false; // MappingNode::shift_map_async: the map shift off the scan path
  bool device_shift = false; // MappingNode::shift_map_device: the global map in device memory (takes precedence over async_shift)
  // de-skewing: false -- every point of a scan is transformed with the one pose of the scan (the reference); true -- "constant
  // velocity": one pose per time bin of the sweep (ScanPreprocessor::preprocess_sweep), the motion during the sweep taken to be
  // the pose change between the last two scans (the identity for the first two)
  bool deskew_constant_velocity = false;
  uint32_t sweep_bins = 1024; // poses per sweep; also the columns of the default rule (by index, ring-major)
  // true: the points of a scan that the averaged map holds as FREE at the scan's pose (ws_map_sample, band tau: observed free space, the
  // sign of a moving object) are dropped on the device before the update and the registration; App::last_rejected() counts them.  An
  // empty map is UNKNOWN everywhere: the first scan drops nothing
  bool reject_dynamic = false;
};

// wall-clock microseconds of the stages of one cloud_callback -- the reference's RuntimeEvaluator forms "preprocess", "tsdf",
// "registration", "total" (app.cpp:68-111), plus the map shift's turn
struct StageTimes
{
  double preprocess_us = 0, tsdf_us = 0, registration_us = 0, shift_us = 0, total_us = 0;
};

class App
{
public:
  App(const AppParams &p, const std::string &h5_filename = std::string(), size_t max_points = 128 * 1024)
      : params_(p), global_map_((int16_t)p.hot.tau, (int16_t)p.initial_weight, h5_filename),
        local_map_(p.map_size[0], p.map_size[1], p.map_size[2], global_map_), node_(p.hot, local_map_), pre_(max_points)
  {
    pose_.setIdentity();
    last_tsdf_pose_.setIdentity();
    last_shift_pose_.setIdentity();
    if (p.device_shift)
    {
      device_global_map_.reset(new DeviceGlobalMap(global_map_.get_default_tsdf_entry()));
      node_.attach(device_global_map_.get());
    }
    else if (p.async_shift) node_.reserve_shift((int)std::ceil(p.shift * 1000.f / (float)p.hot.map_resolution));
    if (global_map_.has_file()) global_map_.write_meta(p.hot.tau, local_map_.get_size(), p.max_distance, p.hot.map_resolution, p.hot.max_weight);
  }

  // App::cloud_callback — app.cpp:65-117; `pretransform` stands for imu_acc_.acc_transform(stamp) (identity: no IMU).
  // The map-shift thread's turn (tsdf_mapping.cpp:104-127) runs synchronously at the end.
  // sweep_motion: the sensor's pose at the end of the sweep in its frame at the beginning (mm); with it, or with
  // AppParams::deskew_constant_velocity, the scan is pre-processed with one pose per time bin, the sweep ending at the current
  // pose.  sweep: the bin rule (default: by index, ring-major, sweep_bins columns).
  const rm::Matrix4x4f &cloud_callback(const float *cloud_xyz, size_t n, size_t stride_floats, const rm::Matrix4x4f *pretransform = nullptr,
                                       const rm::Matrix4x4f *sweep_motion = nullptr, const ws_sweep_t *sweep = nullptr)
  {
    using clk = std::chrono::steady_clock;
    auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    const clk::time_point t0 = clk::now();
    rm::Matrix4x4f guessed;
    if (!sweep_motion && params_.deskew_constant_velocity)
    {
      guessed = last_motion();
      sweep_motion = &guessed;
    }
    size_t n_pts;
    if (sweep_motion)
    {
      const ws_sweep_t rule = sweep ? *sweep : cuda::ScanPreprocessor::by_index(params_.sweep_bins);
      n_pts = pre_.preprocess_sweep(cloud_xyz, n, stride_floats, sweep_poses(pose_, *sweep_motion, params_.sweep_bins), rule, params_.hot.map_resolution);
    }
    else
      n_pts = pre_.preprocess(cloud_xyz, n, stride_floats, pose_, params_.hot.map_resolution); // App::preprocess :119-148
    const int32_t *pts_dev = pre_.points_dev();
    last_rejected_ = 0;
    if (params_.reject_dynamic)
    {
      // The kept points are the sample's selection: they live in the map's sample buffer until the next sample call on this map, so
      // nothing else may sample the map before this callback's update and registration have taken them
      uint64_t counts[4] = {0, 0, 0, 0};
      WS_CHECK(ws_map_sample_dev(node_.gpu().tsdf().handle(), WS_MAP_AVG, pts_dev, n_pts, 0,
                                 WS_SAMPLE_SELECT_UNKNOWN | WS_SAMPLE_SELECT_SURFACE | WS_SAMPLE_SELECT_INSIDE, counts));
      pts_dev = ws_map_sample_selected_dev(node_.gpu().tsdf().handle(), &n_pts);
      last_rejected_ = (size_t)counts[WS_SAMPLE_FREE];
    }
    const clk::time_point t1 = clk::now();
    if (!initialized_ || distance_m(last_tsdf_pose_, pose_) > 0.3f || shifted_)
    {
      initialized_ = true;
      last_tsdf_pose_ = pose_;
      rm::Pointi pos_rm, up_rm;
      node_.gpu().convert_pose_to_gpu(pose_, pos_rm, up_rm);
      node_.gpu().tsdf().update_tsdf_dev(pts_dev, n_pts, pos_rm, up_rm);
      shifted_ = false;
      ++n_updates_;
    }
    const clk::time_point t2 = clk::now();
    rm::Matrix4x4f pre;
    if (pretransform)
      pre = *pretransform;
    else
      pre.setIdentity();
    node_.gpu().registration().prepare_registration_dev(pts_dev, n_pts);
    const rm::Matrix4x4f transform =
        node_.gpu().registration().register_cloud(node_.gpu().tsdf().device_map(), pre, params_.hot.max_iterations, params_.hot.it_weight_gradient,
                                                  params_.hot.epsilon, params_.hot.map_resolution, &last_iterations_);
    update_pose_estimate(transform);
    before_last_pose_ = last_pose_;
    last_pose_ = pose_;
    ++n_scans_;
    if (global_map_.has_file()) global_map_.write_pose(pose_, 1000.f);
    const clk::time_point t3 = clk::now();
    map_shift();
    const clk::time_point t4 = clk::now();
    last_points_ = n_pts;
    times_.preprocess_us = us(t0, t1);
    times_.tsdf_us = us(t1, t2);
    times_.registration_us = us(t2, t3);
    times_.shift_us = us(t3, t4);
    times_.total_us = us(t0, t4);
    return pose_;
  }
  void update_pose_estimate(const rm::Matrix4x4f &t) // app.cpp:172-176
  {
    float R[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
      {
        float acc = 0.f;
        for (int k = 0; k < 3; ++k) acc += t.at(i, k) * pose_.at(k, j);
        R[i][j] = acc;
      }
    for (int i = 0; i < 3; ++i)
    {
      for (int j = 0; j < 3; ++j) pose_.at(i, j) = R[i][j];
      pose_.at(i, 3) += t.at(i, 3);
    }
  }
  // the pose change between the last two scans, inv(pose[-2]) * pose[-1] of rigid poses, in double (the identity for the first two)
  rm::Matrix4x4f last_motion() const
  {
    rm::Matrix4x4f m;
    m.setIdentity();
    if (n_scans_ < 2) return m;
    const rm::Matrix4x4f &a = before_last_pose_, &b = last_pose_;
    for (int i = 0; i < 3; ++i)
    {
      for (int j = 0; j < 3; ++j)
      {
        double acc = 0.0;
        for (int k = 0; k < 3; ++k) acc += (double)a.at(k, i) * (double)b.at(k, j);
        m.at(i, j) = (float)acc;
      }
      double t = 0.0;
      for (int k = 0; k < 3; ++k) t += (double)a.at(k, i) * ((double)b.at(k, 3) - (double)a.at(k, 3));
      m.at(i, 3) = (float)t;
    }
    return m;
  }
  void map_shift()
  {
    if (distance_m(last_shift_pose_, pose_) >= params_.shift)
    {
      last_shift_pose_ = pose_;
      const int res = params_.hot.map_resolution;
      const rm::Pointi target((int)std::floor(pose_.at(0, 3) / (float)res), (int)std::floor(pose_.at(1, 3) / (float)res),
                              (int)std::floor(pose_.at(2, 3) / (float)res)); // to_map, util/util.h:52-56
      if (params_.device_shift)
        node_.shift_map_device(target);
      else if (params_.async_shift)
        node_.shift_map_async(target);
      else
        node_.shift_map(target);
      shifted_ = true;
      ++n_shifts_;
    }
  }
  void terminate() // app.cpp:192-224
  {
    if (initialized_) node_.write_back();
  }

  const rm::Matrix4x4f &pose() const { return pose_; }
  int last_iterations() const { return last_iterations_; }
  const StageTimes &last_times() const { return times_; }
  size_t last_points() const { return last_points_; }
  size_t last_rejected() const { return last_rejected_; } // AppParams::reject_dynamic: points of the last scan dropped as FREE
  int n_updates() const { return n_updates_; }
  int n_shifts() const { return n_shifts_; }
  MappingNode &node() { return node_; }
  SurfaceCloud surface(bool marker = true) { return node_.surface(marker); }
  LocalMap &local_map() { return local_map_; }
  GlobalMap &global_map() { return global_map_; }

private:
  static float distance_m(const rm::Matrix4x4f &a, const rm::Matrix4x4f &b)
  {
    float s = 0.f;
    for (int k = 0; k < 3; ++k)
    {
      const float d = a.at(k, 3) / 1000.f - b.at(k, 3) / 1000.f;
      s += d * d;
    }
    return std::sqrt(s);
  }

  AppParams params_;
  GlobalMap global_map_;
  LocalMap local_map_;
  MappingNode node_;
  std::unique_ptr<DeviceGlobalMap> device_global_map_; // AppParams::device_shift
  cuda::ScanPreprocessor pre_;
  rm::Matrix4x4f pose_, last_tsdf_pose_, last_shift_pose_;
  rm::Matrix4x4f last_pose_, before_last_pose_; // pose_ after the last two scans (last_motion)
  bool initialized_ = false, shifted_ = false;
  int last_iterations_ = 0, n_updates_ = 0, n_shifts_ = 0, n_scans_ = 0;
  size_t last_points_ = 0, last_rejected_ = 0;
  StageTimes times_;
};

} // namespace warpsense
