"""Host-side mirror of the reference's device API over the C ABI (include/warpsense_hip.h).

Same names, argument meaning and error behaviour as the reference classes, so tests read like the
reference's own (test/cuda.cpp, test/pcd_registration.cpp):

    DeviceMap            include/warpsense/cuda/device_map.h:32-164     (non-owning host view)
    DeviceMapMemWrapper  include/warpsense/cuda/device_map_wrapper.h:10-36
    TSDFCuda             include/warpsense/cuda/update_tsdf.h:9-34
    RegistrationCuda     include/warpsense/cuda/registration.h:10-45
    TSDFMapping          src/warpsense/tsdf_mapping.cpp:30-95            (ROS-free constructor path)
    TSDFRegistration     src/warpsense/tsdf_registration.cpp:22-96
    pause / cleanup      src/warpsense/cuda/cleanup.cu

Matrices handed to these classes are ordinary numpy 4x4 arrays (math layout, M[i, j]); the column-major
flattening the C ABI wants (rmagine::Matrix4x4f / Eigen) happens here.  All compute runs in the HIP
library; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import (WS_INTEGRATE_DENSE, WS_INTEGRATE_SPARSE, WS_MAP_AVG, WS_MAP_NEW, WS_REG_ALL_POINTS,
                   WS_REG_COMPAT_REFERENCE_LAUNCH, WsError, check)

MATRIX_RESOLUTION = 32768  # include/warpsense/consts.h:12-13
WEIGHT_RESOLUTION = 64     # include/warpsense/consts.h:9-10


def _ptr(a):
    """void* of a numpy array, a ctypes array or a torch tensor (host or device)."""
    if a is None:
        return None
    if isinstance(a, C.Array):
        return a
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _is_device(a) -> bool:
    return hasattr(a, "is_cuda") and bool(a.is_cuda)


_I3 = C.c_int32 * 3


def _i3(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(3))


def _i3c(v):
    """three int32 for the C ABI only; tuples and lists skip numpy (this sits between two scans of a stream)"""
    if isinstance(v, (tuple, list)) and len(v) == 3:
        return _I3(int(v[0]), int(v[1]), int(v[2]))
    return _i3(v)


def _colmajor(T) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(4, 4).T).reshape(16)


def pack_entry(value, weight):
    """TSDFEntry raw word: low 16 bits value, high 16 bits weight (include/map/tsdf.h:16-23)."""
    v = np.asarray(value).astype(np.int16).astype(np.uint16).astype(np.uint32)
    w = np.asarray(weight).astype(np.int16).astype(np.uint16).astype(np.uint32)
    return v | (w << np.uint32(16))


def unpack_entry(raw):
    raw = np.asarray(raw, dtype=np.uint32)
    return (raw & 0xFFFF).astype(np.uint16).astype(np.int16), (raw >> 16).astype(np.uint16).astype(np.int16)


# one record of ws_map_surface: world voxel coordinates and the packed entry (16 bytes)
SURFACE_RECORD = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("raw", "<u4")])


# one vertex of ws_map_mesh: world position in millimetres and the smallest corner weight of its cell (16 bytes)
VERT = np.dtype([("x_mm", "<i4"), ("y_mm", "<i4"), ("z_mm", "<i4"), ("weight", "<u4")])


# one record of ws_map_raycast: the hit point and the range along the ray in millimetres; no hit: 0, 0, 0, -1 (16 bytes)
RAY = np.dtype([("x_mm", "<i4"), ("y_mm", "<i4"), ("z_mm", "<i4"), ("range_mm", "<i4")])


# one record of ws_map_sample: the interpolated signed distance in mm, the smallest corner weight of the cell, the class (0 unknown,
# 1 free, 2 surface, 3 inside) and the packed entry of the nearest voxel (16 bytes)
SAMPLE = np.dtype([("d_mm", "<i4"), ("weight", "<i4"), ("cls", "<u4"), ("raw", "<u4")])
SAMPLE_CLASSES = _lib.SAMPLE_CLASSES


def distance_class(rec):
    """The class bits of ws_map_distance records: 2 occupied, 1 free, 0 unknown (uint8)."""
    return (np.asarray(rec, dtype=np.uint32) >> np.uint32(30)).astype(np.uint8)


def distance_d2(rec):
    """The squared distance in voxels of ws_map_distance records (bits 0..23, uint32), clamped at max_dist_vox squared."""
    return np.asarray(rec, dtype=np.uint32) & np.uint32(0xFFFFFF)


def distance_mm(rec, res):
    """The distance of ws_map_distance records in millimetres, res * sqrt(d2) as float32 -- the only float of the route, and it
    is made on the host."""
    return (np.float32(res) * np.sqrt(distance_d2(rec).astype(np.float32))).astype(np.float32)


class _DeviceArray:
    """a library-owned device buffer as torch sees it (__cuda_array_interface__); `owner` keeps the handle alive"""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        self._owner = owner


def _device_tensor(ptr, shape, typestr: str, owner):
    import torch
    if not ptr or shape[0] == 0:
        return torch.empty(shape, dtype=torch.int32 if typestr == "<i4" else torch.float32, device="cuda")
    return torch.as_tensor(_DeviceArray(ptr, shape, typestr, owner), device="cuda")


def write_surface_ply(path, marker):
    """The marker cloud of DeviceMapMemWrapper.surface(marker=True) as a binary little-endian PLY: float x y z (metres) and
    uchar red green blue (the reference's r / g / b in [0, 1) scaled by 255 and truncated)."""
    marker = np.asarray(marker, dtype=np.float32).reshape(-1, 7)
    out = np.empty(len(marker), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    out["x"], out["y"], out["z"] = marker[:, 0], marker[:, 1], marker[:, 2]
    for name, col in (("red", 3), ("green", 4), ("blue", 5)):
        out[name] = np.clip(marker[:, col] * np.float32(255.0), 0.0, 255.0).astype(np.uint8)
    header = ("ply\nformat binary_little_endian 1.0\ncomment warpsense_amd surface cloud\n"
              f"element vertex {len(out)}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(out.tobytes())
    return len(out)


def write_mesh_ply(path, vertices, faces):
    """The mesh of DeviceMapMemWrapper.mesh() as a binary little-endian PLY: float x y z in metres (mm / 1000.f in single
    precision), faces as a uchar count (3) and int vertex indices.  Returns (vertices, faces) written."""
    vertices = np.asarray(vertices, dtype=VERT).reshape(-1)
    faces = np.asarray(faces, dtype=np.uint32).reshape(-1, 3)
    v = np.empty(len(vertices), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    for name in "xyz":
        v[name] = vertices[name + "_mm"].astype(np.float32) / np.float32(1000.0)
    f = np.empty(len(faces), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    f["n"] = 3
    f["i"] = faces.astype(np.int32)
    header = ("ply\nformat binary_little_endian 1.0\ncomment warpsense_amd surface-nets mesh\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())
    return len(v), len(f)


def write_raycast_ply(path, records, gradient=None):
    """The hits of DeviceMapMemWrapper.raycast() (records with range_mm >= 0) as a binary little-endian PLY point cloud: float x y z
    in metres (mm / 1000.f in single precision, as write_mesh_ply) and, when `gradient` is given, float nx ny nz: the gradient
    normalised in float64, then cast (a zero gradient stays zero).  Returns the number of points written."""
    records = np.asarray(records, dtype=RAY).reshape(-1)
    hit = records["range_mm"] >= 0
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if gradient is not None else [])
    v = np.empty(int(np.count_nonzero(hit)), dtype=np.dtype([(n, "<f4") for n in names]))
    for name in "xyz":
        v[name] = records[name + "_mm"][hit].astype(np.float32) / np.float32(1000.0)
    if gradient is not None:
        g = np.asarray(gradient, dtype=np.int32).reshape(-1, 3)[hit].astype(np.float64)
        length = np.sqrt(np.sum(g * g, axis=1))
        g = g / np.where(length > 0, length, 1.0)[:, None]
        for k, name in enumerate(("nx", "ny", "nz")):
            v[name] = g[:, k].astype(np.float32)
    header = ("ply\nformat binary_little_endian 1.0\ncomment warpsense_amd ray cast\n"
              f"element vertex {len(v)}\n" + "".join(f"property float {n}\n" for n in names) + "end_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
    return len(v)


class Context:
    """One per process and GPU: device + HIP stream (the reference uses the implicit CUDA context)."""

    _default = None
    _lock = threading.Lock()

    def __init__(self, device_id: int = -1):
        self._L = _lib.load()
        h = C.c_void_p()
        check(self._L.ws_ctx_create(int(device_id), C.byref(h)), "ws_ctx_create")
        self.handle = h

    @classmethod
    def default(cls) -> "Context":
        with cls._lock:
            if cls._default is None:
                cls._default = cls()
            return cls._default

    def set_stream(self, hip_stream_ptr):
        check(self._L.ws_ctx_set_stream(self.handle, C.c_void_p(hip_stream_ptr) if hip_stream_ptr else None),
              "ws_ctx_set_stream")

    def use_torch_stream(self):
        """Run the library's work on torch's CURRENT stream, so that torch operations (copies of the 44 sums, RCCL
        collectives) and the library's kernels are ordered by the stream alone.  The C ABI takes a hipStream_t and reads
        NULL as "the context's own stream", so torch's legacy default stream (handle 0) cannot be named there: in that case
        a new stream is created and made torch's current stream (for this thread) first."""
        import torch
        cur = torch.cuda.current_stream()
        if cur.cuda_stream == 0:
            # SIDE EFFECT, for the calling thread: torch's current stream becomes a new stream (restored by
            # restore_torch_stream() / close()).  The new stream first waits for everything already queued on the default
            # stream -- uploads or preprocessing the caller enqueued there -- so nothing queued earlier can race with later work.
            self._torch_prev_stream = cur
            new = torch.cuda.Stream()
            new.wait_stream(cur)
            torch.cuda.set_stream(new)
            cur = new
        self._torch_stream = cur  # keep it alive
        self.set_stream(cur.cuda_stream)

    def restore_torch_stream(self):
        """Undo use_torch_stream()'s stream switch: the library goes back to its own stream (after the work queued so far)
        and torch's current stream for this thread is the one it was before."""
        prev = getattr(self, "_torch_prev_stream", None)
        if prev is None:
            return
        import torch
        cur = getattr(self, "_torch_stream", None)
        if self.handle:
            self.set_stream(None)  # synchronises the stream it leaves
        if cur is not None:
            prev.wait_stream(cur)
        torch.cuda.set_stream(prev)
        self._torch_prev_stream = None
        self._torch_stream = None

    def sync(self):
        check(self._L.ws_sync(self.handle), "ws_sync")

    # hipEvent timing of kernel classes (bench.py)
    def prof_enable(self, mask: int):
        check(self._L.ws_prof_enable(self.handle, int(mask)), "ws_prof_enable")

    def prof_reset(self):
        check(self._L.ws_prof_reset(self.handle), "ws_prof_reset")

    def prof_read(self, cls: int):
        ms, n = C.c_double(0), C.c_int64(0)
        check(self._L.ws_prof_read(self.handle, int(cls), C.byref(ms), C.byref(n)), "ws_prof_read")
        return ms.value, n.value

    def close(self):
        if self.handle:
            try:
                self.restore_torch_stream()
            except Exception:  # noqa: BLE001 - closing must not fail on a torch that is already shutting down
                pass
            self._L.ws_ctx_destroy(self.handle)
            self.handle = None


def pause(ctx: Context | None = None):
    """cuda::pause() — cleanup.cu:3-6."""
    (ctx or Context.default()).sync()


def cleanup():
    """cuda::cleanup() — cleanup.cu:8-11.  Resets the device: every handle becomes invalid."""
    check(_lib.load().ws_device_reset(), "ws_device_reset")
    Context._default = None


class DeviceMap:
    """Non-owning view of a ring-buffer local map in HOST memory: size, offset, data, pos
    (include/warpsense/cuda/device_map.h:32-48).  The arrays are shared with whoever owns the map."""

    def __init__(self, size, offset, data, pos):
        self.size_ = np.asarray(size, dtype=np.int32).reshape(3)
        self.offset_ = np.asarray(offset, dtype=np.int32).reshape(3)
        self.pos_ = np.asarray(pos, dtype=np.int32).reshape(3)
        self.data_ = data
        if data is not None:
            assert data.dtype == np.uint32 and data.flags["C_CONTIGUOUS"]
            assert data.size == int(np.prod(self.size_.astype(np.int64)))

    def n_voxels(self) -> int:
        return int(np.prod(self.size_.astype(np.int64)))


def pose_to_values(pose, scale: float) -> np.ndarray:
    """The 7 floats HDF5GlobalMap::write_pose stores (hdf5_global_map.cpp:187-197): translation / scale and the
    rotation as a quaternion (x, y, z, w), each rounded to 3 decimals.  The quaternion follows Eigen's
    Quaternionf(Matrix3f) (trace branch / largest diagonal branch) in float32."""
    P = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    out = np.zeros(7, dtype=np.float32)
    for k in range(3):
        # (double / float) * 1000.0f, std::round (half away from zero), / 1000.0f, stored as float
        v = P[k, 3] / float(np.float32(scale)) * 1000.0
        out[k] = np.float32(np.trunc(v + np.copysign(0.5, v)) / 1000.0)
    m = P[:3, :3].astype(np.float32)
    f = np.float32
    q = np.zeros(4, dtype=np.float32)  # x y z w
    t = f(m[0, 0] + m[1, 1] + m[2, 2])
    if t > 0:
        t = f(np.sqrt(f(t + f(1))))
        q[3] = f(f(0.5) * t)
        t = f(f(0.5) / t)
        q[0] = f(f(m[2, 1] - m[1, 2]) * t)
        q[1] = f(f(m[0, 2] - m[2, 0]) * t)
        q[2] = f(f(m[1, 0] - m[0, 1]) * t)
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = f(np.sqrt(f(f(f(m[i, i] - m[j, j]) - m[k, k]) + f(1))))
        q[i] = f(f(0.5) * t)
        t = f(f(0.5) / t)
        q[3] = f(f(m[k, j] - m[j, k]) * t)
        q[j] = f(f(m[j, i] + m[i, j]) * t)
        q[k] = f(f(m[k, i] + m[i, k]) * t)
    for n in range(4):
        v = f(q[n] * f(1000.0))
        out[3 + n] = f(f(np.trunc(v + np.copysign(f(0.5), v))) / f(1000.0))
    return out


class GlobalMap:
    """HDF5GlobalMap (src/map/hdf5_global_map.cpp): the world is cut into 64^3-voxel chunks of raw uint32
    entries, index x*4096 + y*64 + z inside a chunk (:53-57); chunks never seen hold the default entry.

    Without `filename` every chunk stays in memory.  With `filename` the map is the reference's .h5 file
    (layout in include/warpsense_h5.h, written through libwarpsense_h5.so): at most NUM_CHUNKS = 64 chunks are
    active, the least recently used one is written to the file when a 65th is needed (:59-135), write_back()
    flushes the active ones (:160-176), write_pose()/write_meta() as :178-221."""

    CHUNK_SIZE = 64
    NUM_CHUNKS = 64  # hdf5_global_map.h:78

    def __init__(self, default_value, default_weight=0, filename: str | None = None, map_params=None, open_existing: bool = False):
        from collections import OrderedDict
        self.default_raw = int(pack_entry(default_value, default_weight))
        self.lock = threading.RLock()  # the map-shift worker saves slabs while the scan thread writes poses / loads boxes
        self.chunks: "OrderedDict[tuple[int, int, int], np.ndarray]" = OrderedDict()
        self._file = None
        self._filename = filename
        if filename is not None:
            self._H = _lib.load_h5()
            h = C.c_void_p()
            if open_existing:
                _lib.check_h5(self._H.ws_h5_open(filename.encode(), 1, C.byref(h)), "ws_h5_open")
            else:
                _lib.check_h5(self._H.ws_h5_create(filename.encode(), C.byref(h)), "ws_h5_create")
            self._file = h
            # which chunks the file holds, without asking HDF5 again (the map shift looks this up per entering chunk)
            self._in_file: set[tuple[int, int, int]] = set()
            if open_existing:
                n = C.c_int64(0)
                _lib.check_h5(self._H.ws_h5_num_chunks(h, C.byref(n)), "ws_h5_num_chunks")
                if n.value:
                    pos = np.zeros((n.value, 3), dtype=np.int32)
                    _lib.check_h5(self._H.ws_h5_list_chunks(h, _ptr(pos), n.value, C.byref(n)), "ws_h5_list_chunks")
                    self._in_file = {tuple(int(v) for v in p) for p in pos[:n.value]}
            if map_params is not None and not open_existing:
                self.write_meta(map_params)

    def filename(self):
        return self._filename

    # -- chunk cache --------------------------------------------------------------------------------
    def _write_chunk(self, key, data):
        _lib.check_h5(self._H.ws_h5_write_chunk(self._file, key[0], key[1], key[2], _ptr(data)), "ws_h5_write_chunk")
        self._in_file.add(key)

    def has_chunk(self, cx, cy, cz) -> bool:
        """True if the map holds data for this chunk (in memory or in the file) — a chunk never seen is all default."""
        key = (int(cx), int(cy), int(cz))
        with self.lock:
            return key in self.chunks or (self._file is not None and key in self._in_file)

    def activate_chunk(self, cx, cy, cz) -> np.ndarray:
        key = (int(cx), int(cy), int(cz))
        c = self.chunks.get(key)
        if c is not None:
            if self._file is not None:
                self.chunks.move_to_end(key)  # age 0
            return c
        c = np.empty(self.CHUNK_SIZE ** 3, dtype=np.uint32)
        found = C.c_int32(0)
        if self._file is not None:
            _lib.check_h5(self._H.ws_h5_read_chunk(self._file, key[0], key[1], key[2], _ptr(c), C.byref(found)), "ws_h5_read_chunk")
        if not found.value:
            c.fill(self.default_raw)
        if self._file is not None and len(self.chunks) >= self.NUM_CHUNKS:
            old_key, old = self.chunks.popitem(last=False)  # the oldest chunk goes to the file
            self._write_chunk(old_key, old)
        self.chunks[key] = c
        return c

    def get_value(self, x, y, z):
        cs = self.CHUNK_SIZE
        cx, cy, cz = int(x) // cs, int(y) // cs, int(z) // cs  # floor_divide, also for negative coordinates
        c = self.activate_chunk(cx, cy, cz)
        v, w = unpack_entry(c[(int(x) - cx * cs) * cs * cs + (int(y) - cy * cs) * cs + (int(z) - cz * cs)])
        return int(v), int(w)

    def set_value(self, x, y, z, value, weight):
        cs = self.CHUNK_SIZE
        cx, cy, cz = int(x) // cs, int(y) // cs, int(z) // cs
        c = self.activate_chunk(cx, cy, cz)
        c[(int(x) - cx * cs) * cs * cs + (int(y) - cy * cs) * cs + (int(z) - cz * cs)] = pack_entry(value, weight)

    def write_back(self):
        if self._file is None:
            return
        with self.lock:
            for key, data in self.chunks.items():
                self._write_chunk(key, data)
            _lib.check_h5(self._H.ws_h5_flush(self._file), "ws_h5_flush")

    def write_pose(self, pose, scale: float):
        if self._file is None:
            raise WsError("write_pose: this GlobalMap has no file")
        vals = pose_to_values(pose, scale)
        with self.lock:  # the map-shift worker may be writing chunks: the HDF5 library is used by one thread at a time
            _lib.check_h5(self._H.ws_h5_write_pose(self._file, _ptr(vals)), "ws_h5_write_pose")
        return vals

    def write_meta(self, p):
        """p: MapParams (tau, size in voxels, max_distance, resolution, max_weight scaled like map_params.h:88-90)."""
        size = np.asarray(p.size_voxels(), dtype=np.int32)
        _lib.check_h5(self._H.ws_h5_write_meta(self._file, int(p.tau), _ptr(size), C.c_float(p.max_distance), int(p.resolution),
                                               int(p.max_weight)), "ws_h5_write_meta")

    def close(self):
        if self._file is not None:
            self.write_back()
            self._H.ws_h5_close(self._file)
            self._file = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _box(self, lo, hi, buf, save: bool):
        """Move a dense world-voxel box (inclusive, x major / z fastest) between `buf` and the chunks."""
        cs = self.CHUNK_SIZE
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        ext = hi - lo + 1
        box = buf.reshape(int(ext[0]), int(ext[1]), int(ext[2]))
        c0, c1 = np.floor_divide(lo, cs), np.floor_divide(hi, cs)
        for cx in range(c0[0], c1[0] + 1):
            for cy in range(c0[1], c1[1] + 1):
                for cz in range(c0[2], c1[2] + 1):
                    base = np.array([cx, cy, cz], dtype=np.int64) * cs
                    a = np.maximum(lo, base)
                    b = np.minimum(hi, base + cs - 1)
                    sl_c = tuple(slice(int(a[k] - base[k]), int(b[k] - base[k]) + 1) for k in range(3))
                    sl_b = tuple(slice(int(a[k] - lo[k]), int(b[k] - lo[k]) + 1) for k in range(3))
                    with self.lock:  # per chunk: a pose written by the scan thread never waits for a whole slab
                        chunk = self.activate_chunk(cx, cy, cz).reshape(cs, cs, cs)
                        if save:
                            chunk[sl_c] = box[sl_b]
                        else:
                            box[sl_b] = chunk[sl_c]

    def save_box(self, lo, hi, buf):
        self._box(lo, hi, buf, True)

    def load_box(self, lo, hi) -> np.ndarray:
        ext = np.asarray(hi, dtype=np.int64) - np.asarray(lo, dtype=np.int64) + 1
        buf = np.empty(int(np.prod(ext)), dtype=np.uint32)
        self._box(lo, hi, buf, False)
        return buf


def _surface_call(L, name, owner, lead, lo, hi, band, tail, marker, device):
    """The surface call `name` (ws_map_surface, ws_store_surface) on owner.handle and its result: `lead` are the arguments of the entry
    point before the box, `tail` those between the band and the flags.  owner keeps the device tensors' memory alive."""
    if (lo is None) != (hi is None):
        raise WsError("surface: give both lo and hi, or neither")
    n = C.c_size_t(0)
    flags = _lib.WS_SURFACE_MARKER if marker else _lib.WS_SURFACE_RECORDS
    check(getattr(L, name)(owner.handle, *lead, _ptr(_i3(lo)) if lo is not None else None, _ptr(_i3(hi)) if hi is not None else None,
                           int(band) if band is not None else 0, *tail, flags, C.byref(n)), name)
    n = int(n.value)
    if device:
        cnt = C.c_size_t(0)
        rec = _device_tensor(getattr(L, name + "_records_dev")(owner.handle, C.byref(cnt)), (n, 4), "<i4", owner)
        if not marker:
            return rec
        return rec, _device_tensor(getattr(L, name + "_marker_dev")(owner.handle, C.byref(cnt)), (n, 7), "<f4", owner)
    rec = np.empty(n, dtype=SURFACE_RECORD)
    mk = np.empty((n, 7), dtype=np.float32) if marker else None
    got = C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), _ptr(mk), n, C.byref(got)), name + "_download")
    if int(got.value) != n:
        raise WsError("surface: another call replaced the result before it was downloaded")
    return (rec, mk) if marker else rec


def _mesh_call(L, name, owner, lead, lo, hi, tail, any_weight, device):
    """The mesh call `name` (ws_map_mesh, ws_store_mesh) on owner.handle and its result: `lead` and `tail` are the arguments of the
    entry point before and behind the box.  owner keeps the device tensors' memory alive."""
    if (lo is None) != (hi is None):
        raise WsError("mesh: give both lo and hi, or neither")
    nv, nf = C.c_size_t(0), C.c_size_t(0)
    flags = _lib.WS_MESH_ANY_WEIGHT if any_weight else _lib.WS_MESH_DEFAULT
    check(getattr(L, name)(owner.handle, *lead, _ptr(_i3(lo)) if lo is not None else None, _ptr(_i3(hi)) if hi is not None else None, *tail,
                           flags, C.byref(nv), C.byref(nf)), name)
    nv, nf = int(nv.value), int(nf.value)
    if device:
        cnt = C.c_size_t(0)
        return (_device_tensor(getattr(L, name + "_vertices_dev")(owner.handle, C.byref(cnt)), (nv, 4), "<i4", owner),
                _device_tensor(getattr(L, name + "_faces_dev")(owner.handle, C.byref(cnt)), (nf, 3), "<i4", owner))
    vert, face = np.empty(nv, dtype=VERT), np.empty((nf, 3), dtype=np.uint32)
    gv, gf = C.c_size_t(0), C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(vert), _ptr(face), nv, nf, C.byref(gv), C.byref(gf)), name + "_download")
    if (int(gv.value), int(gf.value)) != (nv, nf):
        raise WsError("mesh: another call replaced the result before it was downloaded")
    return vert, face


def _raycast_call(L, name, handle, lead, origin_mm, dirs, max_range_mm, tail, any_weight, gradient, targets):
    """The ray cast `name` (ws_map_raycast, ws_store_raycast; name + "_dev" for directions on the device) and its download: `lead` are
    the arguments of the entry point before the origin, `tail` those between the range and the flags.  Returns (records, gradient |
    None, hits)."""
    n = int(dirs.shape[0])
    flags = ((_lib.WS_RAYCAST_ANY_WEIGHT if any_weight else 0) | (_lib.WS_RAYCAST_GRADIENT if gradient else 0)
             | (_lib.WS_RAYCAST_TARGETS if targets else 0))
    hits = C.c_size_t(0)
    if _is_device(dirs):
        name_call, d = name + "_dev", dirs
    else:
        name_call, d = name, np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 3)
    check(getattr(L, name_call)(handle, *lead, _ptr(_i3(origin_mm)), _ptr(d), n, int(max_range_mm), *tail, flags, C.byref(hits)), name_call)
    rec = np.empty(n, dtype=RAY)
    grad = np.empty((n, 3), dtype=np.int32) if gradient else None
    got = C.c_size_t(0)
    check(getattr(L, name + "_download")(handle, _ptr(rec), _ptr(grad), n, C.byref(got)), name + "_download")
    if int(got.value) != n:
        raise WsError("raycast: another call replaced the result before it was downloaded")
    return rec, grad, int(hits.value)


class _SampleSelection:
    """what keeps the selection of a sample call reachable as DevicePoints: the owner of the buffers, and the way back to the host"""

    def __init__(self, L, name, owner, n_sel):
        self._L, self._name, self._owner, self._n = L, name, owner, int(n_sel)

    def download(self) -> np.ndarray:
        out = np.empty((self._n, 3), dtype=np.int32)
        n, ns = C.c_size_t(0), C.c_size_t(0)
        check(getattr(self._L, self._name + "_download")(self._owner.handle, None, None, _ptr(out), 0, self._n, C.byref(n), C.byref(ns)), self._name + "_download")
        if int(ns.value) != self._n:
            raise WsError("sample: another call replaced the selection before it was downloaded")
        return out


def _sample_flags(any_weight, gradient, select):
    flags = (_lib.WS_SAMPLE_ANY_WEIGHT if any_weight else 0) | (_lib.WS_SAMPLE_GRADIENT if gradient else 0)
    for name in ([select] if isinstance(select, str) else (select or ())):
        if name not in SAMPLE_CLASSES:
            raise WsError(f"sample: select names classes out of {SAMPLE_CLASSES}, not {name!r}")
        flags |= _lib.WS_SAMPLE_SELECT_UNKNOWN << SAMPLE_CLASSES.index(name)
    return flags


def _sample_call(L, name, owner, lead, points, band_mm, tail, any_weight, gradient, select, device):
    """The point sample `name` (ws_map_sample, ws_store_sample; name + "_dev" for points on the device) on owner.handle and its
    result: `lead` are the arguments of the entry point before the points, `tail` those between the band and the flags.  Returns
    (records, counts, gradient | None, selection | None); owner keeps device results' memory alive."""
    n = int(points.shape[0])
    flags = _sample_flags(any_weight, gradient, select)
    selecting = (flags >> 2) != 0
    counts = np.zeros(4, dtype=np.uint64)
    if _is_device(points):
        name_call, pts = name + "_dev", points
    else:
        name_call, pts = name, np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 3)
    check(getattr(L, name_call)(owner.handle, *lead, _ptr(pts), n, int(band_mm), *tail, flags, _ptr(counts)), name_call)
    n_sel = int(sum(int(counts[c]) for c in range(4) if (flags >> (2 + c)) & 1))
    cnt = C.c_size_t(0)
    if device:
        rec = _device_tensor(getattr(L, name + "_records_dev")(owner.handle, C.byref(cnt)), (n, 4), "<i4", owner)
        if int(cnt.value) != n:
            raise WsError("sample: another call replaced the result")
        grad = _device_tensor(getattr(L, name + "_gradient_dev")(owner.handle, C.byref(cnt)), (n, 3), "<i4", owner) if gradient else None
        sel = DevicePoints(getattr(L, name + "_selected_dev")(owner.handle, C.byref(cnt)) or 0, n_sel, _SampleSelection(L, name, owner, n_sel)) if selecting else None
        return rec, counts, grad, sel
    rec = np.empty(n, dtype=SAMPLE)
    grad = np.empty((n, 3), dtype=np.int32) if gradient else None
    sel = np.empty((n_sel, 3), dtype=np.int32) if selecting else None
    got, got_sel = C.c_size_t(0), C.c_size_t(0)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), _ptr(grad), _ptr(sel), n, n_sel, C.byref(got), C.byref(got_sel)), name + "_download")
    if int(got.value) != n or (selecting and int(got_sel.value) != n_sel):
        raise WsError("sample: another call replaced the result before it was downloaded")
    return rec, counts, grad, sel


def _distance_call(L, name, owner, lead, lo, hi, max_dist_vox, unknown_occupied, columns, any_weight, device, default_shape):
    """The distance call `name` (ws_map_distance, ws_store_distance) on owner.handle and its result: `lead` are the arguments of the
    entry point before the box, default_shape() the extent of the box that lo = hi = None stands for.  owner keeps a device tensor's
    memory alive.  Returns (records, sites)."""
    if (lo is None) != (hi is None):
        raise WsError("distance: give both lo and hi, or neither")
    flags = ((_lib.WS_DISTANCE_ANY_WEIGHT if any_weight else 0) | (_lib.WS_DISTANCE_UNKNOWN_OCCUPIED if unknown_occupied else 0)
             | (_lib.WS_DISTANCE_COLUMNS if columns else 0))
    if lo is not None:
        shape = tuple(int(v) for v in (_i3(hi).astype(np.int64) - _i3(lo).astype(np.int64) + 1))
    else:
        shape = default_shape()
    sites = C.c_size_t(0)
    check(getattr(L, name)(owner.handle, *lead, _ptr(_i3(lo)) if lo is not None else None, _ptr(_i3(hi)) if hi is not None else None,
                           int(max_dist_vox), flags, C.byref(sites)), name)
    if columns:
        shape = shape[:2]
    n = int(np.prod(shape, dtype=np.int64))
    cnt = C.c_size_t(0)
    if device:
        ptr = getattr(L, name + "_dev")(owner.handle, C.byref(cnt))
        if int(cnt.value) != n:
            raise WsError("distance: another call replaced the result")
        return _device_tensor(ptr, shape, "<i4", owner), int(sites.value)
    rec = np.empty(n, dtype=np.uint32)
    check(getattr(L, name + "_download")(owner.handle, _ptr(rec), n, C.byref(cnt)), name + "_download")
    if int(cnt.value) != n:
        raise WsError("distance: another call replaced the result before it was downloaded")
    return rec.reshape(shape), int(sites.value)


class DeviceGlobalMap:
    """The global map in device memory (ws_store, include/warpsense_hip.h): the device twin of GlobalMap.  64^3-voxel chunks of raw
    uint32 entries in HBM, index x*4096 + y*64 + z, keyed by floor(world voxel / 64); chunks never seen hold the default entry.  The
    key -> slot directory is the host's.  TSDFMapping(..., device_global_map=this).shift_map_device saves the leaving slabs into
    it and loads the entering ones from it in stream order; flush_to() merges it into a host GlobalMap (and its .h5 file)."""

    CHUNK_SIZE = 64
    CHUNK_WORDS = 64 ** 3

    def __init__(self, default_value, default_weight=0, max_chunks: int = 0, segment_chunks: int = 0, ctx: Context | None = None):
        self.ctx = ctx or Context.default()
        self._L = self.ctx._L
        self.default_raw = int(pack_entry(default_value, default_weight))
        h = C.c_void_p()
        check(self._L.ws_store_create(self.ctx.handle, self.default_raw, int(max_chunks), int(segment_chunks), C.byref(h)), "ws_store_create")
        self.handle = h

    def count(self) -> int:
        n = C.c_uint64(0)
        check(self._L.ws_store_count(self.handle, C.byref(n), None), "ws_store_count")
        return int(n.value)

    def capacity(self) -> int:
        n = C.c_uint64(0)
        check(self._L.ws_store_count(self.handle, None, C.byref(n)), "ws_store_count")
        return int(n.value)

    def reserve(self, n: int):
        """segments for n chunks now, so that no shift has to allocate (and wait for the device)"""
        check(self._L.ws_store_reserve(self.handle, int(n)), "ws_store_reserve")

    def keys(self) -> list:
        """the chunk keys, ascending (cx, cy, cz)"""
        n = C.c_size_t(0)
        check(self._L.ws_store_keys(self.handle, None, 0, C.byref(n)), "ws_store_keys")
        keys = np.zeros((n.value, 3), dtype=np.int32)
        check(self._L.ws_store_keys(self.handle, _ptr(keys), n.value, C.byref(n)), "ws_store_keys")
        return [tuple(int(v) for v in k) for k in keys[:n.value]]

    def has_chunk(self, cx, cy, cz) -> bool:
        return bool(self._L.ws_store_has(self.handle, _i3c((cx, cy, cz))))

    def chunk(self, key):
        """a host copy of one chunk (262 144 uint32), None if the store does not hold it"""
        out = np.empty(self.CHUNK_WORDS, dtype=np.uint32)
        found = C.c_int32(0)
        check(self._L.ws_store_get_chunk(self.handle, _i3c(tuple(key)), _ptr(out), C.byref(found)), "ws_store_get_chunk")
        return out if found.value else None

    def put_chunk(self, key, data):
        data = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1)
        assert data.size == self.CHUNK_WORDS
        check(self._L.ws_store_put_chunk(self.handle, _i3c(tuple(key)), _ptr(data)), "ws_store_put_chunk")

    def drop_chunk(self, key):
        check(self._L.ws_store_drop_chunk(self.handle, _i3c(tuple(key))), "ws_store_drop_chunk")

    def save_box(self, tsdf: "TSDFCuda", lo, hi, which: int = WS_MAP_AVG):
        """the box [lo, hi] of the window of `tsdf` into the chunks (ws_store_save_box; stream-ordered, no wait)"""
        check(self._L.ws_store_save_box(self.handle, tsdf.handle, int(which), _ptr(_i3(lo)), _ptr(_i3(hi))), "ws_store_save_box")

    def load_box(self, tsdf: "TSDFCuda", lo, hi, which: int = WS_MAP_AVG):
        """the chunks into the box [lo, hi] of the window of `tsdf`, the default entry where there is no chunk (ws_store_load_box)"""
        check(self._L.ws_store_load_box(self.handle, tsdf.handle, int(which), _ptr(_i3(lo)), _ptr(_i3(hi))), "ws_store_load_box")

    def timing(self, enable: int = -1):
        """device milliseconds of the save and of the load launches of the last call (ws_debug_store_timing)"""
        ms = (C.c_float * 2)()
        check(self._L.ws_debug_store_timing(self.handle, int(enable), ms), "ws_debug_store_timing")
        return float(ms[0]), float(ms[1])

    def surface(self, tau, resolution, lo=None, hi=None, band=None, marker=False, device=False):
        """The surface cloud of the chunks on the device (ws_store_surface; the rules are those of ws_map_surface, stated in
        include/warpsense_hip.h): every voxel of a present chunk inside the inclusive world-voxel box [lo, hi] (both None: every
        present chunk) with weight > 0 and abs(value) < band (None: tau), in ascending world (x, y, z), z fastest, across chunk
        borders.  Voxels of absent chunks never qualify.  tau, resolution: the map's (the store knows neither); they decide the
        marker's colour and point.

        Returns the same forms as DeviceMapMemWrapper.surface: the records, or with `marker` (records, (n, 7) float32);
        device=True: torch tensors that ALIAS the store's buffers, valid until the next surface() on this store."""
        return _surface_call(self._L, "ws_store_surface", self, (), lo, hi, band, (int(tau), int(resolution)), marker, device)

    def surface_timing(self, enable: int = -1):
        """device milliseconds of the count passes, the scan and the emit pass of the last surface() (ws_debug_store_surface_timing)"""
        ms = (C.c_float * 3)()
        check(self._L.ws_debug_store_surface_timing(self.handle, int(enable), ms), "ws_debug_store_surface_timing")
        return tuple(float(v) for v in ms)

    def mesh(self, resolution, lo=None, hi=None, any_weight=False, device=False):
        """The mesh of the chunks on the device (ws_store_mesh; the rules are those of ws_map_mesh, stated in
        include/warpsense_hip.h): the surface of everything the store holds inside the inclusive world-voxel box [lo, hi] (both
        None: the bounding box of the present chunks), in the order of DeviceMapMemWrapper.mesh across chunk borders.  Voxels of
        absent chunks are not valid.  resolution: the map's, in mm per voxel (the store does not know it).

        Returns (vertices, faces) like DeviceMapMemWrapper.mesh; device=True: torch tensors that ALIAS the store's buffers, valid
        until the next mesh() on this store."""
        return _mesh_call(self._L, "ws_store_mesh", self, (), lo, hi, (int(resolution),), any_weight, device)

    def mesh_timing(self, enable: int = -1):
        """device milliseconds of the count passes, the scan and the emit passes of the last mesh() (ws_debug_store_mesh_timing)"""
        ms = (C.c_float * 3)()
        check(self._L.ws_debug_store_mesh_timing(self.handle, int(enable), ms), "ws_debug_store_mesh_timing")
        return tuple(float(v) for v in ms)

    def raycast(self, resolution, origin_mm, dirs, max_range_mm, lo=None, hi=None, any_weight=False, gradient=False, targets=False):
        """Ray cast of the chunks on the device (ws_store_raycast; the rules are those of ws_map_raycast, stated in
        include/warpsense_hip.h): per ray the first crossing of the surface from the outside within max_range_mm, through
        everything the store holds inside the inclusive world-voxel box [lo, hi] (both None: everything).  Voxels of absent chunks
        are not valid.  resolution: the map's, in mm per voxel.  origin_mm, dirs, targets, any_weight, gradient and the returned
        (records, gradient | None) are those of DeviceMapMemWrapper.raycast; `last_hits` keeps the call's number of hits."""
        if (lo is None) != (hi is None):
            raise WsError("raycast: give both lo and hi, or neither")
        box = (_ptr(_i3(lo)) if lo is not None else None, _ptr(_i3(hi)) if hi is not None else None)
        rec, grad, self.last_hits = _raycast_call(self._L, "ws_store_raycast", self.handle, box, origin_mm, dirs, max_range_mm, (int(resolution),),
                                                  any_weight, gradient, targets)
        return rec, grad

    def sample(self, resolution, points, band_mm, lo=None, hi=None, any_weight=False, gradient=False, select=None, device=False):
        """What the chunks on the device say at `points` (ws_store_sample; the rules are those of ws_map_sample, stated in
        include/warpsense_hip.h), through everything the store holds inside the inclusive world-voxel box [lo, hi] (both None:
        everything).  Voxels of absent chunks are not valid.  resolution: the map's, in mm per voxel; band_mm > 0.  The other arguments
        and the returned (records, counts, gradient | None, selection | None) are those of DeviceMapMemWrapper.sample."""
        if (lo is None) != (hi is None):
            raise WsError("sample: give both lo and hi, or neither")
        box = (_ptr(_i3(lo)) if lo is not None else None, _ptr(_i3(hi)) if hi is not None else None)
        return _sample_call(self._L, "ws_store_sample", self, box, points, band_mm, (int(resolution),), any_weight, gradient, select, device)

    def sample_timing(self, enable: int = -1):
        """device milliseconds of the upload, the sample pass and the select passes of the last sample() (ws_debug_store_sample_timing)"""
        ms = (C.c_float * 3)()
        check(self._L.ws_debug_store_sample_timing(self.handle, int(enable), ms), "ws_debug_store_sample_timing")
        return tuple(float(v) for v in ms)

    def raycast_timing(self, enable: int = -1):
        """device milliseconds of the upload, the march and the gradient pass of the last raycast() (ws_debug_store_raycast_timing)"""
        ms = (C.c_float * 3)()
        check(self._L.ws_debug_store_raycast_timing(self.handle, int(enable), ms), "ws_debug_store_raycast_timing")
        return tuple(float(v) for v in ms)

    def distance(self, lo=None, hi=None, max_dist_vox=20, unknown_occupied=False, columns=False, any_weight=False, device=False):
        """The distance field of the chunks on the device (ws_store_distance; the rules are those of ws_map_distance, stated in
        include/warpsense_hip.h): per voxel of the inclusive world-voxel box [lo, hi] (both None: the bounding box of the present
        chunks) the squared Euclidean distance in voxels to the nearest occupied voxel of the box, clamped at max_dist_vox squared
        (1 .. 255).  Voxels of absent chunks are unknown: with unknown_occupied they are sites.  columns, any_weight, the returned
        uint32 records shaped (nx, ny, nz) or (nx, ny) and `last_sites` are those of DeviceMapMemWrapper.distance.  Unlike mesh()
        and raycast() the result is dense: 8 bytes of device memory per record of the box.
        device=True: a torch int32 tensor of that shape on the GPU that ALIASES the store's buffer, valid until the next distance()
        on this store."""
        def bounding_shape():
            keys = np.asarray(self.keys(), dtype=np.int64).reshape(-1, 3)
            return tuple(int(v) for v in (keys.max(axis=0) - keys.min(axis=0) + 1) * self.CHUNK_SIZE) if len(keys) else (0, 0, 0)
        rec, self.last_sites = _distance_call(self._L, "ws_store_distance", self, (), lo, hi, max_dist_vox, unknown_occupied, columns, any_weight,
                                              device, bounding_shape)
        return rec

    def distance_timing(self, enable: int = -1):
        """device milliseconds of pass 0 and of the x, y and z passes of the last distance() (ws_debug_store_distance_timing)"""
        ms = (C.c_float * 4)()
        check(self._L.ws_debug_store_distance_timing(self.handle, int(enable), ms), "ws_debug_store_distance_timing")
        return tuple(float(v) for v in ms)

    def flush_to(self, global_map: GlobalMap):
        """every chunk merged into a host GlobalMap: into its chunk cache (activate_chunk), or, for a map with a file, straight
        into the file (GlobalMap._write_chunk) unless the chunk is active in the cache"""
        for key in self.keys():
            data = self.chunk(key)
            with global_map.lock:
                if global_map._file is not None and key not in global_map.chunks:
                    global_map._write_chunk(key, data)
                else:
                    global_map.activate_chunk(*key)[:] = data

    def load_from(self, global_map: GlobalMap, keys=None):
        """chunks of a host GlobalMap (None: all it holds, in memory and in its file) into the store, to continue a saved map"""
        if keys is None:
            keys = set(global_map.chunks) | (set(global_map._in_file) if global_map._file is not None else set())
        for key in sorted(tuple(int(v) for v in k) for k in keys):
            if not global_map.has_chunk(*key):
                continue
            with global_map.lock:
                self.put_chunk(key, global_map.activate_chunk(*key))

    def close(self):
        if self.handle:
            self._L.ws_store_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chunks_of_box(lo, hi) -> np.ndarray:
    """host only: the (n, 3) chunk keys an inclusive world-voxel box overlaps, ascending (ws_store_chunks_of_box)"""
    L = _lib.load()
    n = C.c_size_t(0)
    lo, hi = _i3(lo), _i3(hi)
    check(L.ws_store_chunks_of_box(_ptr(lo), _ptr(hi), None, 0, C.byref(n)), "ws_store_chunks_of_box")
    keys = np.zeros((n.value, 3), dtype=np.int32)
    check(L.ws_store_chunks_of_box(_ptr(lo), _ptr(hi), _ptr(keys), n.value, C.byref(n)), "ws_store_chunks_of_box")
    return keys


class LocalMap:
    """HDF5LocalMap without the file (src/map/hdf5_local_map.cpp): a 3-D ring buffer of TSDF entries around `pos`.
    Sizes are forced odd, offset = size/2, every voxel starts as the global map's default entry (:5-20);
    shift() moves the window, saving the slabs that leave to the global map and loading the ones that enter
    (:53-118).  Owns the host arrays a DeviceMap views."""

    def __init__(self, sx, sy, sz, default_value, default_weight=0, global_map: GlobalMap | None = None, host_voxels: bool = True):
        self.size = np.array([s if s % 2 == 1 else s + 1 for s in (int(sx), int(sy), int(sz))], dtype=np.int32)
        self.pos = np.zeros(3, dtype=np.int32)
        self.offset = (self.size // 2).astype(np.int32)
        self.map_ = global_map or GlobalMap(default_value, default_weight)
        # host_voxels=False: the window lives on the device only (a 2049^3 window is 34 GB; the device-side shift and
        # export never need the host copy)
        self.data = np.full(int(np.prod(self.size.astype(np.int64))), self.map_.default_raw, dtype=np.uint32) if host_voxels else None

    def device_map(self) -> DeviceMap:
        return DeviceMap(self.size, self.offset, self.data, self.pos)

    def get_index(self, x, y, z) -> int:
        s, p, o = self.size.astype(np.int64), self.pos.astype(np.int64), self.offset.astype(np.int64)
        xi = (x - p[0] + o[0] + s[0]) % s[0]
        yi = (y - p[1] + o[1] + s[1]) % s[1]
        zi = (z - p[2] + o[2] + s[2]) % s[2]
        return int((xi * s[1] + yi) * s[2] + zi)

    def in_bounds(self, x, y, z) -> bool:
        d = np.abs(np.array([x, y, z], dtype=np.int64) - self.pos)
        return bool(np.all(d <= self.size // 2))

    def value(self, x, y, z):
        if not self.in_bounds(x, y, z):
            raise IndexError(f"Index out of bounds: {x}; {y}; {z}")  # std::out_of_range, hdf5_local_map.h:172-181
        v, w = unpack_entry(self.data[self.get_index(x, y, z)])
        return int(v), int(w)

    def set_value(self, x, y, z, value, weight):
        if not self.in_bounds(x, y, z):
            raise IndexError(f"Index out of bounds: {x}; {y}; {z}")
        self.data[self.get_index(x, y, z)] = pack_entry(value, weight)

    # -- save_load_area<save> (hdf5_local_map.cpp:120-198): one pass per 64^3 chunk the box touches
    def _area(self, start, end, save: bool):
        cs = GlobalMap.CHUNK_SIZE
        start, end = np.minimum(start, end).astype(np.int64), np.maximum(start, end).astype(np.int64)
        s, p, o = self.size.astype(np.int64), self.pos.astype(np.int64), self.offset.astype(np.int64)
        c0, c1 = np.floor_divide(start, cs), np.floor_divide(end, cs)
        for cx in range(c0[0], c1[0] + 1):
            for cy in range(c0[1], c1[1] + 1):
                for cz in range(c0[2], c1[2] + 1):
                    chunk = self.map_.activate_chunk(cx, cy, cz)
                    base = np.array([cx, cy, cz], dtype=np.int64) * cs
                    lo = np.maximum(start, base) - base
                    hi = np.minimum(end, base + cs - 1) - base
                    d = [np.arange(lo[k], hi[k] + 1, dtype=np.int64) for k in range(3)]
                    g = [d[k] + base[k] for k in range(3)]
                    r = [(g[k] - p[k] + o[k] + s[k]) % s[k] for k in range(3)]
                    ring = ((r[0][:, None, None] * s[1] + r[1][None, :, None]) * s[2] + r[2][None, None, :]).reshape(-1)
                    loc = (d[0][:, None, None] * cs * cs + d[1][None, :, None] * cs + d[2][None, None, :]).reshape(-1)
                    if save:
                        chunk[loc] = self.data[ring]
                    else:
                        self.data[ring] = chunk[loc]

    def shift(self, new_pos):
        """HDF5LocalMap::shift (hdf5_local_map.cpp:53-118), axis by axis."""
        new_pos = np.asarray(new_pos, dtype=np.int64)
        diff = new_pos - self.pos
        assert np.all(np.abs(diff) <= self.size)
        for axis in range(3):
            if diff[axis] == 0:
                continue
            start = self.pos.astype(np.int64) - self.size // 2
            end = self.pos.astype(np.int64) + self.size // 2
            if diff[axis] > 0:
                end[axis] = start[axis] + diff[axis] - 1
            else:
                start[axis] = end[axis] + diff[axis] + 1
            self._area(start, end, save=True)
            self.pos[axis] += diff[axis]
            self.offset[axis] = (self.offset[axis] + diff[axis] + self.size[axis]) % self.size[axis]
            start = self.pos.astype(np.int64) - self.size // 2
            end = self.pos.astype(np.int64) + self.size // 2
            if diff[axis] > 0:
                start[axis] = end[axis] - (diff[axis] - 1)
            else:
                end[axis] = start[axis] - diff[axis] - 1
            self._area(start, end, save=False)

    def window(self):
        """(lo, hi) of the window in world voxels, every ring cell once: pos - size/2 .. pos - size/2 + size - 1"""
        lo = self.pos.astype(np.int64) - self.size.astype(np.int64) // 2
        return lo, lo + self.size.astype(np.int64) - 1

    def follow(self, new_pos):
        """pos / offset after a shift the device has made (the data, if any, is not touched)"""
        new_pos = np.asarray(new_pos, dtype=np.int64)
        self.offset[:] = (self.offset + (new_pos - self.pos)) % self.size  # (numpy's % is >= 0 for a negative d)
        self.pos[:] = new_pos

    def write_back(self):
        """hdf5_local_map.cpp:210-217: save the whole window to the global map."""
        self._area(self.pos.astype(np.int64) - self.size // 2, self.pos.astype(np.int64) + self.size // 2, save=True)


class DeviceMapMemWrapper:
    """Device copy of one map (device_map_wrapper.h:10-36); owned by a TSDFCuda."""

    def __init__(self, tsdf: "TSDFCuda", which: int):
        self._t = tsdf
        self._which = which

    def to_device(self, existing_map: DeviceMap):
        t = self._t
        check(t._L.ws_map_upload(t.handle, self._which, _ptr(_i3(existing_map.size_)), _ptr(_i3(existing_map.pos_)),
                                 _ptr(_i3(existing_map.offset_)), _ptr(existing_map.data_)), "ws_map_upload")

    def update_params(self, existing_map: DeviceMap):
        t = self._t
        check(t._L.ws_map_set_params(t.handle, self._which, _ptr(_i3(existing_map.size_)),
                                     _ptr(_i3(existing_map.pos_)), _ptr(_i3(existing_map.offset_))), "ws_map_set_params")

    def to_host(self, existing_map: DeviceMap):
        t = self._t
        size, pos, off = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
        check(t._L.ws_map_download(t.handle, self._which, _ptr(size), _ptr(pos), _ptr(off), _ptr(existing_map.data_)),
              "ws_map_download")
        existing_map.size_[:] = size
        existing_map.pos_[:] = pos
        existing_map.offset_[:] = off

    def extract_box(self, lo, hi) -> np.ndarray:
        """Voxels of the inclusive world-voxel box [lo, hi] (x major, z fastest) — ws_map_extract_box."""
        t = self._t
        lo, hi = _i3(lo), _i3(hi)
        out = np.empty(int(np.prod((hi - lo + 1).astype(np.int64))), dtype=np.uint32)
        check(t._L.ws_map_extract_box(t.handle, self._which, _ptr(lo), _ptr(hi), _ptr(out)), "ws_map_extract_box")
        return out

    def insert_box(self, lo, hi, data):
        t = self._t
        lo, hi = _i3(lo), _i3(hi)
        data = np.ascontiguousarray(data, dtype=np.uint32)
        assert data.size == int(np.prod((hi - lo + 1).astype(np.int64)))
        check(t._L.ws_map_insert_box(t.handle, self._which, _ptr(lo), _ptr(hi), _ptr(data)), "ws_map_insert_box")

    def surface(self, lo=None, hi=None, band=None, marker=False, device=False):
        """The surface cloud of this map — publish_local_map (include/warpsense/visualization/map.h:14-121) on the device
        (ws_map_surface): every voxel of the inclusive world-voxel box [lo, hi] (both None: the whole window) with
        weight > 0 and abs(value) < band (None: tau), in ascending world (x, y, z), z fastest.

        Returns the records as a numpy array of dtype SURFACE_RECORD (x, y, z in world voxels, raw entry); with `marker`
        a pair (records, (n, 7) float32: x y z in metres, r g b a as the reference computes them).
        device=True: torch tensors on the GPU instead — (n, 4) int32 and (n, 7) float32 — that ALIAS the library's buffers:
        valid until the next surface() on this TSDFCuda, copy them (.clone()) to keep them."""
        return _surface_call(self._t._L, "ws_map_surface", self._t, (self._which,), lo, hi, band, (), marker, device)

    def mesh(self, lo=None, hi=None, any_weight=False, device=False):
        """A triangle mesh of this map by naive surface nets on the device (ws_map_mesh; the rules are stated in
        include/warpsense_hip.h): one vertex per active cell of the inclusive world-voxel box [lo, hi] (both None: the whole
        window), two triangles per crossing lattice edge whose four cells are valid.  any_weight: voxels with a negative weight
        count as observed too (the rule of the registration).

        Returns (vertices, faces): a numpy array of dtype VERT (x_mm, y_mm, z_mm, weight) in ascending cell order and an (n, 3)
        uint32 array of vertex indices, normals towards the outside.
        device=True: torch tensors on the GPU instead -- (n, 4) int32 and (n, 3) int32 -- that ALIAS the library's buffers: valid
        until the next mesh() on this TSDFCuda, copy them (.clone()) to keep them."""
        return _mesh_call(self._t._L, "ws_map_mesh", self._t, (self._which,), lo, hi, (), any_weight, device)

    def raycast(self, origin_mm, dirs, max_range_mm, any_weight=False, gradient=False, targets=False):
        """Ray cast of this map on the device (ws_map_raycast; the rules are stated in include/warpsense_hip.h): per ray the first
        crossing of the surface from the outside within max_range_mm.  origin_mm: three int32 (map frame, millimetres); dirs:
        (n, 3) int32 directions of any length (|component| < 2^30), a numpy array or a device array (a CUDA tensor, DevicePoints);
        targets=True: `dirs` holds map-frame points in mm instead and every ray runs from the origin towards its point.
        any_weight: voxels with a negative weight count as observed too (the rule of the registration).

        Returns (records, gradient): a numpy array of dtype RAY (x_mm, y_mm, z_mm, range_mm; no hit: 0, 0, 0, -1) in ray order
        and, with gradient=True, an (n, 3) int32 array of central differences of the TSDF value at the hit (towards the outside,
        not normalised; zeros where a neighbour is unobserved), else None.  `last_hits` keeps the call's number of hits."""
        rec, grad, self.last_hits = _raycast_call(self._t._L, "ws_map_raycast", self._t.handle, (self._which,), origin_mm, dirs, max_range_mm, (),
                                                  any_weight, gradient, targets)
        return rec, grad

    def sample(self, points, band_mm=None, any_weight=False, gradient=False, select=None, device=False):
        """What this map says at `points` (ws_map_sample; the rules are stated in include/warpsense_hip.h): (n, 3) int32 map-frame
        points in millimetres, a numpy array or a device array (a CUDA tensor, DevicePoints).  band_mm: the half-width of the SURFACE
        class (None: the map's tau).  any_weight: voxels with a negative weight count as observed too (the rule of the registration).
        select: class names out of SAMPLE_CLASSES ("unknown", "free", "surface", "inside"); the input points of those classes come
        back in input order.

        Returns (records, counts, gradient, selection): a numpy array of dtype SAMPLE (d_mm, weight, cls, raw) in input order; the
        number of points per class (uint64 [4]); with gradient=True an (n, 3) int32 array of central differences of the TSDF value
        at the nearest voxel (zeros where a neighbour is unobserved), else None; with `select` the (k, 3) int32 selected points, else
        None.  device=True: records and gradient are torch tensors on the GPU ((n, 4) / (n, 3) int32) and the selection is a
        DevicePoints that update_tsdf and prepare_registration accept; all three ALIAS the library's buffers and are valid until the
        next sample() on this TSDFCuda."""
        return _sample_call(self._t._L, "ws_map_sample", self._t, (self._which,), points, 0 if band_mm is None else band_mm, (), any_weight, gradient, select,
                            device)

    def distance(self, lo=None, hi=None, max_dist_vox=20, unknown_occupied=False, columns=False, any_weight=False, device=False):
        """The distance field of this map on the device (ws_map_distance; the rules are stated in include/warpsense_hip.h): per
        voxel of the inclusive world-voxel box [lo, hi] (both None: the whole window) the squared Euclidean distance in voxels to
        the nearest occupied voxel of the box (valid and value < 0; unknown_occupied: or never observed), clamped at
        max_dist_vox squared (1 .. 255).  columns: the 2-D field over the (x, y) columns of the box.  any_weight: voxels with a
        negative weight count as observed too (the rule of the registration).

        Returns the records as a uint32 array shaped (nx, ny, nz), or (nx, ny) with columns: bits 0..23 the squared distance,
        bits 30..31 the class (distance_d2, distance_class, distance_mm take them apart).  `last_sites` keeps the call's number
        of site voxels / columns.
        device=True: a torch int32 tensor of that shape on the GPU instead that ALIASES the library's buffer: valid until the next
        distance() on this TSDFCuda, copy it (.clone()) to keep it."""
        def window_shape():
            size = np.zeros(3, np.int32)
            check(self._t._L.ws_map_get_params(self._t.handle, self._which, _ptr(size), None, None), "ws_map_get_params")
            return tuple(int(v) for v in size)
        rec, self.last_sites = _distance_call(self._t._L, "ws_map_distance", self._t, (self._which,), lo, hi, max_dist_vox, unknown_occupied, columns,
                                              any_weight, device, window_shape)
        return rec

    def dev(self):
        return self._t.handle

    def device_ptr(self) -> int:
        return int(self._t._L.ws_map_device_data(self._t.handle, self._which) or 0)


class TSDFCuda:
    """cuda::TSDFCuda (update_tsdf.h:9-34, update_tsdf.cu:130-221)."""

    n_max_points_ = 1_000_000

    def __init__(self, existing_map: DeviceMap, tau: int, max_weight: int, map_resolution: int, ctx: Context | None = None):
        self.ctx = ctx or Context.default()
        self._L = self.ctx._L
        self.tau_, self.max_weight_, self.map_resolution_ = int(tau), int(max_weight), int(map_resolution)
        self.n_voxels_ = existing_map.n_voxels()
        h = C.c_void_p()
        check(self._L.ws_map_create(self.ctx.handle, _ptr(_i3(existing_map.size_)), _ptr(_i3(existing_map.pos_)),
                                    _ptr(_i3(existing_map.offset_)), _ptr(existing_map.data_), self.tau_, self.max_weight_,
                                    self.map_resolution_, C.byref(h)), "ws_map_create")
        self.handle = h
        self._avg = DeviceMapMemWrapper(self, WS_MAP_AVG)
        self._new = DeviceMapMemWrapper(self, WS_MAP_NEW)
        self._scan_in_flight = None  # the device tensor of the last update (kept until the next one is enqueued behind it)

    # -- the three update_tsdf overloads of the reference (update_tsdf.cu:143-191)
    def update_tsdf(self, scan_points, scanner_pos, up, result: DeviceMap | None = None, latest_map: DeviceMap | None = None):
        n = int(scan_points.shape[0])
        sp, u = _i3c(scanner_pos), _i3c(up)
        if _is_device(scan_points):
            # ws_tsdf_update_dev returns after its launches: the tensor must not go back to torch's allocator before the kernels have
            # read it (torch's allocator only knows torch's streams) -- keep it until the next update has been enqueued behind it
            prev = self._scan_in_flight
            rc = self._L.ws_tsdf_update_dev(self.handle, _ptr(scan_points), n, _ptr(sp), _ptr(u))
            self._scan_in_flight = scan_points
            del prev
        else:
            pts = np.ascontiguousarray(scan_points, dtype=np.int32)
            rc = self._L.ws_tsdf_update(self.handle, _ptr(pts), n, _ptr(sp), _ptr(u))
        if rc == -3:
            # update_tsdf.cu:146-150: message on stderr, no work, no exception
            import sys
            print("HIP Error: " + self._L.ws_last_error().decode(), file=sys.stderr)
            return
        check(rc, "ws_tsdf_update")
        if result is not None:
            self._avg.to_host(result)
        if latest_map is not None:
            self._new.to_host(latest_map)

    def scatter(self, scan_points_dev, scanner_pos, up):
        """cu_min_tsdf_krnl alone (parity tests): leaves the resolved scan in new_map."""
        prev = self._scan_in_flight  # (see update_tsdf)
        check(self._L.ws_tsdf_scatter_dev(self.handle, _ptr(scan_points_dev), int(scan_points_dev.shape[0]),
                                          _ptr(_i3c(scanner_pos)), _ptr(_i3c(up))), "ws_tsdf_scatter_dev")
        self._scan_in_flight = scan_points_dev
        del prev

    def integrate(self):
        check(self._L.ws_tsdf_integrate(self.handle), "ws_tsdf_integrate")

    def set_integrate(self, mode: int):
        check(self._L.ws_tsdf_set_integrate(self.handle, int(mode)), "ws_tsdf_set_integrate")

    def set_capacity(self, records: int):
        check(self._L.ws_tsdf_set_capacity(self.handle, int(records)), "ws_tsdf_set_capacity")

    def debug_chunk_policy(self, budget_bytes: int, est_shift: int):
        """test entry: size the chunk buffer by estimate (see ws_debug_tsdf_chunk_policy)"""
        check(self._L.ws_debug_tsdf_chunk_policy(self.handle, int(budget_bytes), int(est_shift)), "ws_debug_tsdf_chunk_policy")

    def stats(self, raise_on_error: bool = False) -> dict:
        st = _lib.TsdfStats()
        rc = self._L.ws_tsdf_stats(self.handle, C.byref(st))
        out = {"contested_voxels": st.contested_voxels, "records": st.records, "tiles": st.tiles, "error_flags": st.error_flags,
               "runs": st.runs, "free_space_hits": st.free_space_hits, "record_slots": st.record_slots,
               "record_capacity": st.record_capacity, "hash_entries": st.hash_entries, "status": rc}
        if rc != 0 and raise_on_error:
            check(rc, "ws_tsdf_stats")
        return out

    def device_map(self):
        return self.handle

    def avg_map(self) -> DeviceMapMemWrapper:
        return self._avg

    def new_map(self) -> DeviceMapMemWrapper:
        return self._new

    def close(self):
        if self.handle:
            self._L.ws_map_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RegistrationCuda:
    """cuda::RegistrationCuda (registration.h:10-45, registration.cu:259-368)."""

    def __init__(self, map_: DeviceMap | None = None, ctx: Context | None = None, flags: int = WS_REG_ALL_POINTS):
        self.ctx = ctx or Context.default()
        self._L = self.ctx._L
        self.flags = int(flags)
        h = C.c_void_p()
        check(self._L.ws_reg_create(self.ctx.handle, 128 * 1024, C.byref(h)), "ws_reg_create")
        self.handle = h
        self.curr_n_points = 0

    def prepare_registration(self, points):
        n = int(points.shape[0])
        self.curr_n_points = n
        if _is_device(points):
            # (an asynchronous device-to-device copy on the context's stream: like TSDFCuda.update_tsdf, keep the tensor away from
            # torch's allocator until the next cloud's copy has been enqueued behind it)
            prev = getattr(self, "_cloud_in_flight", None)
            check(self._L.ws_reg_prepare_dev(self.handle, _ptr(points), n), "ws_reg_prepare_dev")
            self._cloud_in_flight = points
            del prev
        else:
            pts = np.ascontiguousarray(points, dtype=np.int32)
            check(self._L.ws_reg_prepare(self.handle, _ptr(pts), n), "ws_reg_prepare")

    def perform_registration(self, map_dev, pretransform, map_resolution: int):
        """Returns (h 6x6 int64 math layout, g[6] int64, e, c) — the out-parameters of the reference."""
        T = _colmajor(pretransform)
        h = np.zeros(36, dtype=np.int64)
        g = np.zeros(6, dtype=np.int64)
        e, c = C.c_int32(0), C.c_int32(0)
        check(self._L.ws_reg_iterate(self.handle, map_dev, _ptr(T), int(map_resolution), self.flags, _ptr(h), _ptr(g),
                                     C.byref(e), C.byref(c)), "ws_reg_iterate")
        return h.reshape(6, 6).T.copy(), g, e.value, c.value

    def register_cloud(self, map_dev, pretransform, max_iterations, it_weight_gradient, epsilon, map_resolution):
        # (two ctypes buffers kept for the life of the object: numpy's .ctypes costs 3 us per array, and this call sits in the gap
        # between the end of one registration and the first kernel of the next update)
        buf = getattr(self, "_rc_buf", None)
        if buf is None:
            buf = self._rc_buf = ((C.c_float * 16)(), (C.c_float * 16)(), C.c_int32(0))
        T_c, out_c, it = buf
        T_c[:] = np.asarray(pretransform, dtype=np.float32).reshape(4, 4).T.reshape(16).tolist()
        check(self._L.ws_register_cloud(self.handle, map_dev, T_c, int(max_iterations), C.c_float(it_weight_gradient),
                                        C.c_float(epsilon), int(map_resolution), self.flags, out_c, C.byref(it)),
              "ws_register_cloud")
        return np.array(out_c, dtype=np.float32).reshape(4, 4).T.copy(), it.value

    def register_cloud_batch(self, map_dev, poses, max_iterations, it_weight_gradient, epsilon, map_resolution):
        """K registrations of the prepared cloud, one per start pose, in one launch (ws_register_cloud_batch).
        poses: (k, 4, 4).  Returns (T[k, 4, 4] float32, iterations[k], e[k], c[k]): pose k and its iteration count are what
        register_cloud returns from poses[k] alone; e[k], c[k] are perform_registration's e and c at T[k]."""
        P = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
        k = int(P.shape[0])
        T_in = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(k, 16)
        T_out = np.zeros((k, 16), dtype=np.float32)
        it, e, c = (np.zeros(k, dtype=np.int32) for _ in range(3))
        check(self._L.ws_register_cloud_batch(self.handle, map_dev, _ptr(T_in), k, int(max_iterations), C.c_float(it_weight_gradient),
                                              C.c_float(epsilon), int(map_resolution), self.flags, _ptr(T_out), _ptr(it), _ptr(e), _ptr(c)),
              "ws_register_cloud_batch")
        return np.ascontiguousarray(T_out.reshape(k, 4, 4).transpose(0, 2, 1)), it, e, c

    def last_sums(self):
        """(h 6x6 int64, g[6], e, c) the last Gauss-Newton update of the last register_cloud was made from (test entry)"""
        out = np.empty(44, dtype=np.int64)
        check(self._L.ws_debug_reg_sums(self.handle, _ptr(out)), "ws_debug_reg_sums")
        return out[:36].reshape(6, 6).T.copy(), out[36:42].copy(), int(out[42]), int(out[43])

    def set_loop(self, mode: int):
        """WS_REG_LOOP_RESIDENT (one launch, grid barrier; default) or WS_REG_LOOP_LAUNCHES (one launch per iteration)."""
        check(self._L.ws_reg_set_loop(self.handle, int(mode)), "ws_reg_set_loop")

    def close(self):
        if self.handle:
            self._L.ws_reg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def batch_best(e, c, min_count: int = 1) -> int:
    """Index of the best hypothesis of a batch (ws_reg_batch_best): among those with c[i] >= min_count the smallest mean error
    e[i] / c[i], compared exactly; ties: larger c, then lower index.  -1 if none qualifies."""
    e = np.ascontiguousarray(e, dtype=np.int32).reshape(-1)
    c = np.ascontiguousarray(c, dtype=np.int32).reshape(-1)
    if e.shape != c.shape:
        raise ValueError("batch_best: e and c differ in length")
    best = C.c_int64(-1)
    check(_lib.load().ws_reg_batch_best(_ptr(e), _ptr(c), int(e.shape[0]), int(min_count), C.byref(best)), "ws_reg_batch_best")
    return int(best.value)


def candidate_poses(guess, radius_m: float, step_m: float, yaw_range_deg: float = 0.0, yaw_step_deg: float = 0.0) -> np.ndarray:
    """The local pose lattice of TSDFRegistration.relocalize around `guess` (4x4, translation in mm): (n, 4, 4) float32.

    x and y offsets i * step_m, |i| <= floor(radius_m / step_m), on a square grid in the map frame; yaw offsets j * yaw_step_deg,
    |j| <= floor(yaw_range_deg / yaw_step_deg), about the map's z axis through the guess's own position (the rotation is
    multiplied from the left, the translation keeps its place).  A step <= 0 leaves that axis at the guess.  Candidate 0 is the
    guess itself, unchanged; the others follow row-major (x slowest, then y, yaw fastest, each from its most negative offset
    upwards) without the node of all-zero offsets, whose place the guess has taken: (2 nx + 1)(2 ny + 1)(2 nyaw + 1) poses.
    Computed in float64, rounded once to float32."""
    G = np.asarray(guess, dtype=np.float64).reshape(4, 4)
    n_xy = int(np.floor(radius_m / step_m + 1e-9)) if step_m > 0 and radius_m > 0 else 0
    n_yaw = int(np.floor(yaw_range_deg / yaw_step_deg + 1e-9)) if yaw_step_deg > 0 and yaw_range_deg > 0 else 0
    out = [G.copy()]
    for ix in range(-n_xy, n_xy + 1):
        for iy in range(-n_xy, n_xy + 1):
            for iw in range(-n_yaw, n_yaw + 1):
                if ix == 0 and iy == 0 and iw == 0:
                    continue
                a = np.deg2rad(iw * float(yaw_step_deg))
                Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
                Tc = G.copy()
                Tc[:3, :3] = Rz @ G[:3, :3]
                Tc[0, 3] = G[0, 3] + ix * float(step_m) * 1000.0
                Tc[1, 3] = G[1, 3] + iy * float(step_m) * 1000.0
                out.append(Tc)
    return np.stack(out).astype(np.float32)


class DevicePoints:
    """(n, 3) int32 points resident on the device (what ScanPreprocessor returns); accepted wherever a CUDA
    tensor of points is (TSDFCuda.update_tsdf, RegistrationCuda.prepare_registration)."""

    is_cuda = True

    def __init__(self, ptr: int, n: int, owner):
        self._ptr, self.shape, self._owner = int(ptr), (int(n), 3), owner

    def data_ptr(self) -> int:
        return self._ptr

    def __len__(self):
        return self.shape[0]

    def to_host(self) -> np.ndarray:
        return self._owner.download()


class ScanPreprocessor:
    """App::preprocess on the device (src/warpsense/app.cpp:119-148): sensor cloud in float metres -> distinct
    voxel-centre points in int mm, transformed by the pose, in first-occurrence order."""

    def __init__(self, max_points: int = 128 * 1024, ctx: Context | None = None):
        self.ctx = ctx or Context.default()
        self._L = self.ctx._L
        h = C.c_void_p()
        check(self._L.ws_scan_create(self.ctx.handle, int(max_points), C.byref(h)), "ws_scan_create")
        self.handle = h
        self.n_out = 0

    def preprocess(self, cloud, pose, map_resolution: int) -> DevicePoints:
        """cloud: (n, k >= 3) float32, numpy or CUDA tensor (x y z first); pose: 4x4, translation in mm."""
        n, stride = int(cloud.shape[0]), int(cloud.shape[1])
        T = _colmajor(pose)
        out = C.c_size_t(0)
        if _is_device(cloud):
            check(self._L.ws_scan_preprocess_dev(self.handle, _ptr(cloud), n, stride, _ptr(T), int(map_resolution), C.byref(out)),
                  "ws_scan_preprocess_dev")
        else:
            a = np.ascontiguousarray(cloud, dtype=np.float32)
            check(self._L.ws_scan_preprocess(self.handle, _ptr(a), n, stride, _ptr(T), int(map_resolution), C.byref(out)),
                  "ws_scan_preprocess")
        self.n_out = int(out.value)
        return DevicePoints(self._L.ws_scan_points_dev(self.handle) or 0, self.n_out, self)

    def preprocess_sweep(self, cloud, poses, map_resolution: int, *, columns=None, ring_major: bool = True, time_field=None,
                         t_begin: float = 0.0, t_end: float = 1.0) -> DevicePoints:
        """preprocess with one sensor pose per time bin of the sweep (ws_scan_preprocess_sweep): poses (k, 4, 4), translation in
        mm, e.g. from sweep_poses.  The bin of point i follows its column -- `columns` firing columns (default: k), ring_major
        True for index = ring * columns + column -- or, with time_field, the float at that index of its record between t_begin
        and t_end.  De-duplicated over the whole sweep, first-occurrence order."""
        n, stride = int(cloud.shape[0]), int(cloud.shape[1])
        P = np.asarray(poses, dtype=np.float32)
        if P.ndim != 3 or P.shape[1:] != (4, 4):
            raise ValueError("preprocess_sweep: poses must be (k, 4, 4)")
        k = int(P.shape[0])
        Pc = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1)  # column-major rows of 16
        rule = _sweep_rule(k, columns, ring_major, time_field, t_begin, t_end)
        out = C.c_size_t(0)
        if _is_device(cloud):
            check(self._L.ws_scan_preprocess_sweep_dev(self.handle, _ptr(cloud), n, stride, _ptr(Pc) if k else None, k, C.byref(rule), int(map_resolution),
                                                       C.byref(out)), "ws_scan_preprocess_sweep_dev")
        else:
            a = np.ascontiguousarray(cloud, dtype=np.float32)
            check(self._L.ws_scan_preprocess_sweep(self.handle, _ptr(a), n, stride, _ptr(Pc) if k else None, k, C.byref(rule), int(map_resolution),
                                                   C.byref(out)), "ws_scan_preprocess_sweep")
        self.n_out = int(out.value)
        return DevicePoints(self._L.ws_scan_points_dev(self.handle) or 0, self.n_out, self)

    def download(self) -> np.ndarray:
        pts = np.zeros((max(self.n_out, 1), 3), dtype=np.int32)
        n = C.c_size_t(0)
        check(self._L.ws_scan_download(self.handle, _ptr(pts), pts.shape[0], C.byref(n)), "ws_scan_download")
        return pts[:int(n.value)].copy()

    def close(self):
        if self.handle:
            self._L.ws_scan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def to_int_mat(mat):
    """(mat * MATRIX_RESOLUTION).cast<int>() — include/util/util.h:8-11."""
    return (np.asarray(mat, dtype=np.float32) * np.float32(MATRIX_RESOLUTION)).astype(np.int32)


def _sweep_rule(k, columns, ring_major, time_field, t_begin, t_end) -> _lib.Sweep:
    if time_field is None:
        return _lib.Sweep(int(k if columns is None else columns), int(bool(ring_major)), -1, 0.0, 1.0)
    if int(time_field) < 0:
        raise ValueError("preprocess_sweep: time_field is the index of a float of the point record")
    return _lib.Sweep(0, 0, int(time_field), float(t_begin), float(t_end))


def sweep_poses(pose_end, motion, k: int) -> np.ndarray:
    """The k sensor poses of a sweep (ws_sweep_poses, host code in double; no GPU needed): pose_end is the pose at the end of the
    sweep (4x4, translation in mm), motion the sensor's pose at the end expressed in its frame at the beginning
    (inv(T_begin) @ T_end).  Pose b is the pose at s = (b + 0.5) / k.  Returns (k, 4, 4) float32."""
    k = int(k)
    out = np.zeros((max(k, 1), 16), dtype=np.float32)
    check(_lib.load().ws_sweep_poses(_ptr(_colmajor(pose_end)), _ptr(_colmajor(motion)), max(k, 0), _ptr(out)), "ws_sweep_poses")
    return np.ascontiguousarray(out[:k].reshape(k, 4, 4).transpose(0, 2, 1))


def sweep_bins(n: int, k: int, cloud=None, *, columns=None, ring_major: bool = True, time_field=None, t_begin: float = 0.0, t_end: float = 1.0):
    """The bin of every point of a sweep, as the kernel computes it (include/warpsense_hip.h): (n,) int64, -1 for a point whose
    time gives a NaN.  Raises ValueError for what the library refuses."""
    if not 1 <= int(k) <= _lib.WS_SWEEP_MAX_BINS:
        raise ValueError("sweep: 1 <= k <= 4096 poses")
    if time_field is None:
        columns = int(k if columns is None else columns)
        if columns < 1 or n % columns != 0:
            raise ValueError("sweep: the point count is not a multiple of the columns")
        i = np.arange(n, dtype=np.int64)
        col = i % columns if ring_major else i // max(n // columns, 1)
        return col * int(k) // columns
    a = np.asarray(cloud, dtype=np.float32)
    f = np.float32
    if not 3 <= int(time_field) < a.shape[1]:
        raise ValueError("sweep: time_field must index a float of the record after x y z")
    if not (np.isfinite(f(t_begin)) and np.isfinite(f(t_end))) or f(t_begin) == f(t_end):
        raise ValueError("sweep: t_begin and t_end must be finite and differ")
    with np.errstate(all="ignore"):
        s = (a[:, int(time_field)] - f(t_begin)) / f(f(t_end) - f(t_begin))  # float32, step by step
        v = s * f(k)
        b = np.where(v >= f(k), int(k) - 1, np.where(v > 0, np.minimum(v, f(k)).astype(np.int64), 0))
    return np.where(np.isnan(s), -1, b).astype(np.int64)


def preprocess_sweep_host(cloud, poses, map_resolution: int, *, columns=None, ring_major: bool = True, time_field=None, t_begin: float = 0.0,
                          t_end: float = 1.0) -> np.ndarray:
    """Host model of ScanPreprocessor.preprocess_sweep in plain numpy, the yardstick of its tests: float32 arithmetic step by step,
    wrapping int32 products, truncating division, a first-occurrence set over the whole sweep.  A coordinate beyond +-2^20 mm
    raises WsError (the library's WS_ERR_RANGE)."""
    f = np.float32
    a = np.asarray(cloud, dtype=np.float32)
    P = np.asarray(poses, dtype=np.float32)
    n, res = a.shape[0], int(map_resolution)
    b = sweep_bins(n, P.shape[0], a, columns=columns, ring_major=ring_major, time_field=time_field, t_begin=t_begin, t_end=t_end)
    M = to_int_mat(P).astype(np.int64)  # (k, 4, 4), math layout
    xyz = a[:, :3]
    with np.errstate(all="ignore"):
        keep = np.isfinite(xyz).all(axis=1) & ~(xyz.astype(np.float64) < 0.3).all(axis=1) & (b >= 0)
        idx = np.nonzero(keep)[0]
        p = xyz[idx]
        c = (np.floor((p * f(1000.0)) / f(res)) * f(res) + f(res // 2)).astype(np.int32).astype(np.int64)  # float32 throughout

    def wrap(v):
        return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31

    Mi = M[b[idx]]
    acc = np.zeros((len(idx), 3), dtype=np.int64)
    for j in range(3):
        acc = wrap(acc + wrap(Mi[:, :3, j] * c[:, j:j + 1]))
    acc = wrap(acc + Mi[:, :3, 3])
    q = np.sign(acc) * (np.abs(acc) // MATRIX_RESOLUTION)  # C division truncates toward zero
    if np.any(np.abs(q) >= 2 ** 20):
        raise WsError("preprocess_sweep_host: a transformed coordinate is beyond +-2^20 mm")
    _, first = np.unique(q, axis=0, return_index=True)
    return q[np.sort(first)].astype(np.int32).reshape(-1, 3)


def to_map(pose, map_resolution: int):
    """floor(translation / resolution) in float — include/util/util.h:52-56."""
    t = np.asarray(pose, dtype=np.float32)[:3, 3]
    return np.floor(t / np.float32(map_resolution)).astype(np.int32)


class MapParams:
    """The hot-path knobs of params/params.yaml with the scaling rules of include/params/map_params.h:100-114."""

    def __init__(self, resolution=64, max_distance=1.0, max_weight=10, size=(40.0, 40.0, 25.0), shift=10.0, initial_weight=0):
        self.resolution = int(resolution)
        self.max_distance = float(max_distance)
        self.tau = int(max_distance * 1000)
        self.max_weight = int(max_weight * WEIGHT_RESOLUTION)
        self.size = tuple(int(s * 1000 / self.resolution) for s in size)
        self.shift = float(shift)
        self.initial_weight = int(initial_weight)

    def size_voxels(self):
        return self.size


class RegistrationParams:
    def __init__(self, max_iterations=200, it_weight_gradient=0.1, epsilon=0.03):
        self.max_iterations = int(max_iterations)
        self.it_weight_gradient = float(it_weight_gradient)
        self.epsilon = float(epsilon)


class Params:
    def __init__(self, map_params: MapParams | None = None, registration: RegistrationParams | None = None):
        self.map = map_params or MapParams()
        self.registration = registration or RegistrationParams()


class TSDFMapping:
    """cuda::TSDFMapping without ROS (the protected constructor path, tsdf_mapping.cpp:30-41)."""

    def __init__(self, params: Params, local_map: LocalMap, ctx: Context | None = None, device_global_map: "DeviceGlobalMap | None" = None):
        self.params_ = params
        self.local_map_ = local_map
        self.cuda_map_ = local_map.device_map()
        self.tsdf_ = TSDFCuda(self.cuda_map_, params.map.tau, params.map.max_weight, params.map.resolution, ctx)
        self.mutex_ = threading.RLock()  # the reference's shared_mutex: one writer or many readers
        # the global map in device memory: shift_map_device and write_back go through it (shift_map / shift_map_async do not)
        self.device_global_map_ = device_global_map

    def convert_pose_to_gpu(self, pose):
        """tsdf_mapping.cpp:77-85: pos = floor(t/res) voxels, up = (R_int * (0,0,MR)) / MR."""
        # (R_int * (0, 0, MR) + 0) / MR == third column of R_int exactly (|R_int| <= 32768, no int overflow)
        up = to_int_mat(pose)[:3, 2].astype(np.int32)
        return to_map(pose, self.params_.map.resolution), up

    def update_tsdf(self, scan_points, pose=None, pos_rm=None, up_rm=None, result: DeviceMap | None = None):
        if pose is not None:
            pos_rm, up_rm = self.convert_pose_to_gpu(pose)
        with self.mutex_:
            self.tsdf_.update_tsdf(scan_points, pos_rm, up_rm, result=result)

    def tsdf(self) -> TSDFCuda:
        return self.tsdf_

    def surface_cloud(self, **kw):
        """publish_local_map's cloud of the averaged map (visualization/map.h:14-121; the reference publishes it after every
        update, src/cpu/fastsense.cpp:115): DeviceMapMemWrapper.surface on avg_map(), under the mapping's lock like a reader."""
        with self.mutex_:
            return self.tsdf_.avg_map().surface(**kw)

    def surface_mesh(self, **kw):
        """A triangle mesh of the averaged map (DeviceMapMemWrapper.mesh on avg_map()), under the mapping's lock like a reader."""
        with self.mutex_:
            return self.tsdf_.avg_map().mesh(**kw)

    def distance_field(self, lo=None, hi=None, max_dist_m=1.0, unknown_occupied=False, columns=False, any_weight=False):
        """The distance field of the averaged map (DeviceMapMemWrapper.distance on avg_map()), under the mapping's lock like a
        reader: how far every voxel of the box (None: the window) is from the nearest obstacle, up to max_dist_m metres
        (rounded to whole millimetres, then ceil(mm / resolution) voxels, 1 .. 255).  columns: the 2-D cost map of a ground robot whose height band is the box's
        z range.  Returns the uint32 records shaped (nx, ny, nz) or (nx, ny); distance_mm(rec, resolution) gives millimetres."""
        mm = int(np.rint(float(max_dist_m) * 1000.0))
        res = int(self.params_.map.resolution)
        with self.mutex_:
            return self.tsdf_.avg_map().distance(lo=lo, hi=hi, max_dist_vox=-(-mm // res), unknown_occupied=unknown_occupied, columns=columns,
                                                 any_weight=any_weight)

    def global_mesh(self, **kw):
        """The mesh of everything the run has seen: the window goes into the chunks of device_global_map (ws_store_save_box, the
        first step of write_back, with its capacity refusals), then DeviceGlobalMap.mesh at the map's resolution -- under the
        mapping's lock like a writer, nothing leaves the device but the mesh.  Keywords: lo, hi, any_weight, device."""
        if self.device_global_map_ is None:
            raise WsError("global_mesh: this TSDFMapping has no device_global_map")
        self.wait_shift()
        with self.mutex_:
            lo, hi = self.local_map_.window()
            self.device_global_map_.save_box(self.tsdf_, lo, hi)
            return self.device_global_map_.mesh(int(self.params_.map.resolution), **kw)

    def global_surface_cloud(self, **kw):
        """The surface cloud of everything the run has seen, including what the window has left: the window goes into the chunks of
        device_global_map exactly as in global_mesh (ws_store_save_box behind wait_shift, under the mapping's lock like a writer),
        then DeviceGlobalMap.surface with the map's tau and resolution.  Keywords: lo, hi, band, marker, device."""
        if self.device_global_map_ is None:
            raise WsError("global_surface_cloud: this TSDFMapping has no device_global_map")
        self.wait_shift()
        with self.mutex_:
            lo, hi = self.local_map_.window()
            self.device_global_map_.save_box(self.tsdf_, lo, hi)
            return self.device_global_map_.surface(self.tsdf_.tau_, int(self.params_.map.resolution), **kw)

    def global_distance_field(self, lo=None, hi=None, max_dist_m=1.0, unknown_occupied=False, columns=False, any_weight=False, device=False):
        """The distance field of everything the run has seen: the window goes into the chunks of device_global_map exactly as in
        global_mesh (ws_store_save_box behind wait_shift, under the mapping's lock like a writer), then DeviceGlobalMap.distance.
        The box (None: the bounding box of the chunks) need not lie in the window; max_dist_m becomes voxels by the rule of
        distance_field (nearest millimetre, then ceil(mm / resolution), 1 .. 255).  The result is dense: 8 bytes of device memory
        per record of the box."""
        if self.device_global_map_ is None:
            raise WsError("global_distance_field: this TSDFMapping has no device_global_map")
        mm = int(np.rint(float(max_dist_m) * 1000.0))
        res = int(self.params_.map.resolution)
        self.wait_shift()
        with self.mutex_:
            wlo, whi = self.local_map_.window()
            self.device_global_map_.save_box(self.tsdf_, wlo, whi)
            return self.device_global_map_.distance(lo=lo, hi=hi, max_dist_vox=-(-mm // res), unknown_occupied=unknown_occupied, columns=columns,
                                                    any_weight=any_weight, device=device)

    @staticmethod
    def raycast_rays(pose, dirs):
        """The integers of a ray cast from a pose, in float64 numpy: origin = the pose's translation in metres times 1000, rounded
        to nearest (ties to even); every direction (unit-free, sensor frame) is rotated by the pose's 3 x 3 block and scaled so
        that its longest component is 2^20 in magnitude, then rounded to nearest; a zero direction stays zero (a no-hit).
        Returns (origin_mm (3,) int32, dirs (n, 3) int32)."""
        pose = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        origin = np.rint(pose[:3, 3] * 1000.0).astype(np.int32)
        d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3) @ pose[:3, :3].T
        longest = np.max(np.abs(d), axis=1)
        d = d * (float(1 << 20) / np.where(longest > 0, longest, 1.0))[:, None]
        return origin, np.rint(d).astype(np.int32)

    def _diagonal_mm(self):
        size = np.asarray(self.local_map_.size, dtype=np.float64) * float(self.params_.map.resolution)
        return int(np.ceil(np.sqrt(np.sum(size * size))))

    def raycast(self, pose, dirs=None, max_range_mm=None, **kw):
        """The predicted scan of the averaged map from `pose` (4 x 4, metres): DeviceMapMemWrapper.raycast on avg_map(), under the
        mapping's lock like a reader.  dirs: (n, 3) float directions in the sensor frame (None: the 128 x 1024 table of the
        OS1-128 pattern, synthetic.os1_128_dirs); they and the pose become integers by the rule of raycast_rays.
        max_range_mm None: the window's diagonal.  Returns (records, gradient | None)."""
        if dirs is None:
            from .synthetic import os1_128_dirs
            dirs = os1_128_dirs()
        origin, d = self.raycast_rays(pose, dirs)
        with self.mutex_:
            return self.tsdf_.avg_map().raycast(origin, d, self._diagonal_mm() if max_range_mm is None else max_range_mm, **kw)

    def scan_residual(self, points_mm, pose, **kw):
        """Per point of a scan in the map frame (n x 3 int32 millimetres, numpy or on the device as it lies: a CUDA tensor,
        DevicePoints) the range the averaged map shows along the ray from the pose's origin (raycast_rays) towards the point,
        minus the point's own distance |point - origin|, in millimetres (float64; NaN where the ray does not hit within the
        window's diagonal).  The median of its absolute value is the quality figure of a registration."""
        origin = self.raycast_rays(pose, np.zeros((0, 3)))[0]
        with self.mutex_:
            rec, _ = self.tsdf_.avg_map().raycast(origin, points_mm, self._diagonal_mm(), targets=True, **kw)
        if _is_device(points_mm):
            points_mm = points_mm.to_host() if hasattr(points_mm, "to_host") else points_mm.cpu().numpy()
        d = np.asarray(points_mm, dtype=np.float64).reshape(-1, 3) - origin.astype(np.float64)
        return np.where(rec["range_mm"] >= 0, rec["range_mm"].astype(np.float64) - np.sqrt(np.sum(d * d, axis=1)), np.nan)

    def sample(self, points_mm, **kw):
        """DeviceMapMemWrapper.sample on avg_map() at map-frame points (n x 3 int32 millimetres, numpy or on the device), under the
        mapping's lock like a reader.  Returns (records, counts, gradient | None, selection | None)."""
        with self.mutex_:
            return self.tsdf_.avg_map().sample(points_mm, **kw)

    def global_sample(self, points_mm, band_mm=None, **kw):
        """sample against the chunks of device_global_map: the window goes into the chunks as in global_raycast, then
        DeviceGlobalMap.sample at the map's resolution.  band_mm None: the map's tau.  Keywords: lo, hi, any_weight, gradient, select,
        device."""
        if self.device_global_map_ is None:
            raise WsError("global_sample: this TSDFMapping has no device_global_map")
        self.wait_shift()
        with self.mutex_:
            lo, hi = self.local_map_.window()
            self.device_global_map_.save_box(self.tsdf_, lo, hi)
            return self.device_global_map_.sample(int(self.params_.map.resolution), points_mm, int(self.params_.map.tau) if band_mm is None else band_mm, **kw)

    def scan_consistency(self, points_mm, pose=None, band_mm=None):
        """How a scan agrees with the averaged map, in one pass over its points: points_mm are the scan in the map frame (n x 3 int32
        millimetres, numpy or on the device); with `pose` (4 x 4, translation in mm) they are in the sensor frame and are moved by it
        first (on the host, rounded to nearest).  Returns a dict: the fractions "unknown", "free", "surface", "inside" of the points
        per class of sample() at band_mm (None: tau), and "mean_abs_d_mm", the mean |d_mm| over the SURFACE class (NaN without
        one)."""
        if pose is not None:
            if _is_device(points_mm):
                points_mm = points_mm.to_host() if hasattr(points_mm, "to_host") else points_mm.cpu().numpy()
            P = np.asarray(pose, dtype=np.float64).reshape(4, 4)
            points_mm = np.rint(np.asarray(points_mm, dtype=np.float64).reshape(-1, 3) @ P[:3, :3].T + P[:3, 3]).astype(np.int32)
        rec, counts, _, _ = self.sample(points_mm, band_mm=band_mm)
        n = max(int(counts.sum()), 1)
        out = {name: float(counts[c]) / n for c, name in enumerate(SAMPLE_CLASSES)}
        surf = rec["cls"] == 2
        out["mean_abs_d_mm"] = float(np.mean(np.abs(rec["d_mm"][surf].astype(np.float64)))) if surf.any() else float("nan")
        return out

    def _global_range_mm(self, origin):
        """the diagonal of the bounding box of the present chunks in mm, capped so that |origin| + range + 2 res fits int32"""
        res = int(self.params_.map.resolution)
        keys = np.asarray(self.device_global_map_.keys(), dtype=np.float64).reshape(-1, 3)
        ext = (keys.max(axis=0) - keys.min(axis=0) + 1.0) * 64.0 * res if len(keys) else np.ones(3)
        cap = 2 ** 31 - 1 - 2 * res - int(np.max(np.abs(np.asarray(origin, dtype=np.int64))))
        return int(max(1, min(cap, np.ceil(np.sqrt(np.sum(ext * ext))))))

    def global_raycast(self, pose, dirs=None, max_range_mm=None, **kw):
        """The predicted scan from `pose` through everything the run has seen, not only the window: the window goes into the
        chunks of device_global_map exactly as in global_mesh (ws_store_save_box behind wait_shift, under the mapping's lock like a
        writer), then DeviceGlobalMap.raycast at the map's resolution with the integers of raycast_rays.  dirs None: the OS1-128
        table; max_range_mm None: the diagonal of the bounding box of the present chunks (capped to what the range check admits).
        Keywords: lo, hi, any_weight, gradient, targets.  Returns (records, gradient | None)."""
        if self.device_global_map_ is None:
            raise WsError("global_raycast: this TSDFMapping has no device_global_map")
        if kw.get("targets"):
            origin, d = self.raycast_rays(pose, np.zeros((0, 3)))[0], dirs
        else:
            if dirs is None:
                from .synthetic import os1_128_dirs
                dirs = os1_128_dirs()
            origin, d = self.raycast_rays(pose, dirs)
        self.wait_shift()
        with self.mutex_:
            lo, hi = self.local_map_.window()
            self.device_global_map_.save_box(self.tsdf_, lo, hi)
            rng = self._global_range_mm(origin) if max_range_mm is None else max_range_mm
            return self.device_global_map_.raycast(int(self.params_.map.resolution), origin, d, rng, **kw)

    def global_scan_residual(self, points_mm, pose, **kw):
        """scan_residual against the chunks of device_global_map (global_raycast with the points as targets): the pose may lie
        anywhere the run has been.  NaN where the ray does not hit within the diagonal of the present chunks' bounding box."""
        rec, _ = self.global_raycast(pose, points_mm, targets=True, **kw)
        origin = self.raycast_rays(pose, np.zeros((0, 3)))[0]
        if _is_device(points_mm):
            points_mm = points_mm.to_host() if hasattr(points_mm, "to_host") else points_mm.cpu().numpy()
        d = np.asarray(points_mm, dtype=np.float64).reshape(-1, 3) - origin.astype(np.float64)
        return np.where(rec["range_mm"] >= 0, rec["range_mm"].astype(np.float64) - np.sqrt(np.sum(d * d, axis=1)), np.nan)

    def shift_map(self, new_pos):
        """TSDFMapping::map_shift (tsdf_mapping.cpp:109-126) with the window moved ON THE DEVICE: per axis, the slab
        that leaves is packed and saved to the global map, pos/offset move, the slab that enters is loaded and
        unpacked (the three steps of HDF5LocalMap::shift, hdf5_local_map.cpp:53-118).  The reference copies the whole
        map device -> host -> device instead.  The host LocalMap only follows pos/offset; its voxel array is stale
        until avg_map().to_host() is called."""
        self.wait_shift()
        lm, avg, new = self.local_map_, self.tsdf_.avg_map(), self.tsdf_.new_map()
        with self.mutex_:
            plan = _lib.ShiftPlan()  # per axis that moves: the boxes that leave and enter
            check(self.tsdf_._L.ws_shift_plan(_ptr(_i3(lm.size)), _ptr(_i3(lm.pos)), _ptr(_i3(lm.offset)), _ptr(_i3(new_pos)), C.byref(plan)),
                  "ws_shift_plan")
            for i in range(plan.n):
                lo, hi = np.array(plan.leave_lo[i], dtype=np.int64), np.array(plan.leave_hi[i], dtype=np.int64)
                lm.map_.save_box(lo, hi, avg.extract_box(lo, hi))
                step = lm.pos.copy()
                step[plan.axis[i]] += plan.d[i]
                lm.follow(step)
                view = lm.device_map()
                avg.update_params(view)
                new.update_params(view)  # new_map is (tau, 0) everywhere: only its window moves
                lo, hi = np.array(plan.enter_lo[i], dtype=np.int64), np.array(plan.enter_hi[i], dtype=np.int64)
                avg.insert_box(lo, hi, lm.map_.load_box(lo, hi))

    # ---- the same shift off the scan path ---------------------------------------------------------------
    def shift_map_async(self, new_pos):
        """TSDFMapping::map_shift as the reference runs it — on its own thread, the scans only wait for the swap
        (tsdf_mapping.cpp:97-136).  On the scan path: ws_shift_begin (device kernels: pack the leaving slabs into a staging
        buffer, move the window, fill the entering slabs with the default entry — stream-ordered, no waiting) and, only for
        revisited space, the upload of the chunks the global map already holds for the entering slabs.  The leaving slabs
        travel to the host on a second stream and a worker thread files them into the global map.  Same result as
        shift_map(); wait_shift() joins the worker (write_back() and the next shift do that themselves)."""
        self.wait_shift()  # one shift in flight; its slabs must be in the global map before entering data is looked up
        lm, avg = self.local_map_, self.tsdf_.avg_map()
        new_pos = _i3(new_pos)
        L = self.tsdf_._L
        ticket = C.c_void_p()
        n = 0
        self._shift_error = None

        def file_slabs():
            # the ticket is closed whatever happens, and a failure travels to wait_shift() (a daemon thread's traceback
            # would be the only trace of slabs that never reached the global map)
            try:
                file_slabs_body()
            except BaseException as exc:  # noqa: BLE001 - re-raised by wait_shift()
                self._shift_error = exc
            finally:
                L.ws_shift_end(ticket)

        def file_slabs_body():
            check(L.ws_shift_wait(ticket), "ws_shift_wait")
            slo, shi = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
            elo, ehi = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
            for i in range(n):
                data = C.c_void_p()
                check(L.ws_shift_slab(ticket, i, _ptr(slo), _ptr(shi), C.byref(data)), "ws_shift_slab")
                ext = shi.astype(np.int64) - slo + 1
                buf = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint32)), shape=(int(np.prod(ext)),))
                box = buf.reshape(int(ext[0]), int(ext[1]), int(ext[2]))
                # A corner that ENTERED with an earlier axis of this shift and leaves again with this one was packed as
                # default fill; the synchronous route would have loaded it from the global map and saved it back
                # unchanged.  Put the global map's own data there, so the save below changes nothing for it.
                for j in range(i):
                    check(L.ws_shift_entering(ticket, j, _ptr(elo), _ptr(ehi)), "ws_shift_entering")
                    a, b = np.maximum(slo, elo).astype(np.int64), np.minimum(shi, ehi).astype(np.int64)
                    if np.all(a <= b):
                        e = b - a + 1
                        sl = tuple(slice(int(a[k] - slo[k]), int(b[k] - slo[k]) + 1) for k in range(3))
                        box[sl] = lm.map_.load_box(a, b).reshape(int(e[0]), int(e[1]), int(e[2]))
                lm.map_.save_box(slo.copy(), shi.copy(), buf)

        with self.mutex_:
            check(L.ws_shift_begin(self.tsdf_.handle, _ptr(new_pos), int(lm.map_.default_raw), C.byref(ticket)), "ws_shift_begin")
            n = L.ws_shift_count(ticket)
            try:
                self._shift_enter(L, ticket, n, new_pos, lm, avg)
            except BaseException:
                # the window has moved on the device: the leaving slabs are still filed and the ticket is closed (an open
                # ticket makes every later ws_shift_begin fail); the failure itself goes to the caller
                file_slabs()
                raise
        self._shift_worker = threading.Thread(target=file_slabs, name="warpsense-map-shift", daemon=True)
        self._shift_worker.start()

    def _shift_enter(self, L, ticket, n, new_pos, lm, avg):
        """the host side of an asynchronous shift between ws_shift_begin and the start of the worker"""
        lm.follow(new_pos)  # the host view of the window
        # revisited space: chunks the global map already has overwrite the default fill
        cs = GlobalMap.CHUNK_SIZE
        lo, hi = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
        for i in range(n):
            check(L.ws_shift_entering(ticket, i, _ptr(lo), _ptr(hi)), "ws_shift_entering")
            # a later axis step moves the window again: only the part of the slab still inside the FINAL window counts
            wlo, whi = lm.window()
            a, b = np.maximum(lo.astype(np.int64), wlo), np.minimum(hi.astype(np.int64), whi)
            if np.any(a > b):
                continue
            c0, c1 = np.floor_divide(a, cs), np.floor_divide(b, cs)
            for cx in range(int(c0[0]), int(c1[0]) + 1):
                for cy in range(int(c0[1]), int(c1[1]) + 1):
                    for cz in range(int(c0[2]), int(c1[2]) + 1):
                        if not lm.map_.has_chunk(cx, cy, cz):
                            continue
                        base = np.array([cx, cy, cz], dtype=np.int64) * cs
                        sa, sb = np.maximum(a, base), np.minimum(b, base + cs - 1)
                        avg.insert_box(sa, sb, lm.map_.load_box(sa, sb))

    def shift_map_device(self, new_pos):
        """TSDFMapping::map_shift with the global map in device memory (ws_shift_device): per axis the leaving slab goes into
        the chunks of device_global_map, pos / offset of both maps move, and the entering slab comes out of them -- revisited
        space and corners included -- as device-to-device copies in stream order.  Nothing is transferred, staged or filed on the
        host; the call returns after enqueueing.  The host LocalMap follows pos / offset."""
        if self.device_global_map_ is None:
            raise WsError("shift_map_device: this TSDFMapping has no device_global_map")
        self.wait_shift()
        lm = self.local_map_
        new_pos = _i3(new_pos)
        with self.mutex_:
            check(self.tsdf_._L.ws_shift_device(self.tsdf_.handle, self.device_global_map_.handle, _ptr(new_pos)), "ws_shift_device")
            lm.follow(new_pos)

    def reserve_shift(self, shift_voxels: int):
        """staging for asynchronous shifts of up to `shift_voxels` per axis (plus slack), allocated now instead of inside
        the first shift (a pinned allocation of that size takes tens of milliseconds)"""
        s = self.local_map_.size.astype(np.int64)
        d = int(shift_voxels) + 8
        total = int(d * (s[0] * s[1] + s[1] * s[2] + s[0] * s[2]))
        check(self.tsdf_._L.ws_shift_reserve(self.tsdf_.handle, total), "ws_shift_reserve")

    def wait_shift(self):
        w = getattr(self, "_shift_worker", None)
        if w is not None:
            w.join()
            self._shift_worker = None
            err, self._shift_error = getattr(self, "_shift_error", None), None
            if err is not None:
                raise WsError(f"asynchronous map shift: the leaving slabs were not filed into the global map ({err!r})") from err

    def write_back(self, box_lo=None, box_hi=None):
        """HDF5LocalMap::write_back + HDF5GlobalMap::write_back (hdf5_local_map.cpp:210-217, app.cpp:220) from the
        DEVICE map: every 64^3 chunk the window overlaps is gathered out of the ring buffer by the GPU
        (ws_map_extract_box: chunk layout, x major / z fastest), merged into the global map's chunk and written to
        its file.  The reference downloads the whole window and copies voxel by voxel on the host.
        box_lo / box_hi (inclusive world voxels) restrict the export to a part of the window.
        With a device_global_map: ws_store_save_box of the (clipped) window, DeviceGlobalMap.flush_to the host global map, its
        write_back -- the same chunks and the same file."""
        self.wait_shift()
        lm, avg = self.local_map_, self.tsdf_.avg_map()
        cs = GlobalMap.CHUNK_SIZE
        with self.mutex_:
            lo, hi = lm.window()
            if box_lo is not None:
                lo = np.maximum(lo, np.asarray(box_lo, dtype=np.int64))
            if box_hi is not None:
                hi = np.minimum(hi, np.asarray(box_hi, dtype=np.int64))
            if self.device_global_map_ is not None:
                # the window goes into the device chunks in one launch, and the chunks into the host map and its file
                self.device_global_map_.save_box(self.tsdf_, lo, hi)
                self.device_global_map_.flush_to(lm.map_)
                lm.map_.write_back()
                return
            # one gather per 64-voxel-thick x slab of chunks (a few large device->host copies instead of one small one
            # per chunk); save_box cuts the slab into its chunks
            for cx in range(int(np.floor_divide(lo[0], cs)), int(np.floor_divide(hi[0], cs)) + 1):
                a, b = lo.copy(), hi.copy()
                a[0], b[0] = max(lo[0], cx * cs), min(hi[0], cx * cs + cs - 1)
                lm.map_.save_box(a, b, avg.extract_box(a, b))
            lm.map_.write_back()


class TSDFRegistration(TSDFMapping):
    """cuda::TSDFRegistration (tsdf_registration.cpp:22-96)."""

    def __init__(self, params: Params, local_map: LocalMap, ctx: Context | None = None, flags: int = WS_REG_ALL_POINTS,
                 device_global_map: "DeviceGlobalMap | None" = None):
        super().__init__(params, local_map, ctx, device_global_map)
        self.reg_ = RegistrationCuda(self.cuda_map_, ctx, flags)
        self.last_iterations = 0

    def register_cloud(self, cloud, pretransform):
        """Returns total_transform (4x4 float32); Gauss-Newton loop on the device."""
        self.reg_.prepare_registration(cloud)
        r, m = self.params_.registration, self.params_.map
        with self.mutex_:
            T, it = self.reg_.register_cloud(self.tsdf_.device_map(), pretransform, r.max_iterations, r.it_weight_gradient,
                                             r.epsilon, m.resolution)
        self.last_iterations = it
        return T

    def register_candidates(self, cloud, poses):
        """register_cloud from every pose of `poses` (k, 4, 4) in one launch: (T[k, 4, 4], iterations[k], e[k], c[k]); rank them
        with batch_best(e, c, min_count)."""
        self.reg_.prepare_registration(cloud)
        r, m = self.params_.registration, self.params_.map
        with self.mutex_:
            return self.reg_.register_cloud_batch(self.tsdf_.device_map(), poses, r.max_iterations, r.it_weight_gradient, r.epsilon,
                                                  m.resolution)

    def relocalize(self, cloud, guess, radius_m, step_m, yaw_range_deg=0.0, yaw_step_deg=0.0, min_fraction=0.5):
        """Re-localise inside the map: register `cloud` from every pose of candidate_poses(guess, ...) and keep the one whose final
        mean error is smallest among those that matched at least min_fraction of the points.
        Returns (best_pose 4x4 float32, best_index, table) with table = dict(start=, pose=, iterations=, e=, c=) over all candidates;
        raises WsError if no candidate reaches min_fraction."""
        poses = candidate_poses(guess, radius_m, step_m, yaw_range_deg, yaw_step_deg)
        T, it, e, c = self.register_candidates(cloud, poses)
        n = int(cloud.shape[0])
        min_count = max(1, int(np.ceil(float(min_fraction) * n)))
        best = batch_best(e, c, min_count)
        table = {"start": poses, "pose": T, "iterations": it, "e": e, "c": c}
        if best < 0:
            raise WsError(f"relocalize: none of the {len(poses)} candidates matched {min_count} of {n} points (best count {int(c.max()) if len(c) else 0})")
        self.last_iterations = int(it[best])
        return T[best].copy(), best, table
