"""Packed snapshots of the global map (ws_store_pack / ws_store_unpack, ws_pack_*; the format is stated in include/warpsense_hip.h):
PackedMap, what DeviceGlobalMap.pack returns and .unpack takes, its `.wspk` file, and the host-only route between a PackedMap and a
host GlobalMap, which needs no GPU."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._abi import _device_tensor, _i3c, _ptr
from ._lib import WS_PACK_HEADER_WORDS, WsError, check

CHUNK_WORDS = 64 ** 3
CHUNK_BYTES = 4 * CHUNK_WORDS
WSPK_VERSION = 1


@dataclass
class PackedMap:
    """Chunks of a global map in packed form.  headers: (n, 40) uint32, one per chunk, ascending keys; payload: the uint32 stream (a
    numpy array, or with DeviceGlobalMap.pack(device=True) an int32 torch tensor that ALIASES the store's buffer, valid until the
    next pack() on that store); fill: the raw word the default bricks stand for; stats: (default, uniform, dense bricks, bytes)."""
    headers: np.ndarray
    payload: object
    fill: int
    resolution: int | None = None
    tau: int | None = None
    stats: tuple | None = None
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        self.headers = np.ascontiguousarray(self.headers, dtype=np.uint32).reshape(-1, WS_PACK_HEADER_WORDS)
        if isinstance(self.payload, np.ndarray):
            self.payload = np.ascontiguousarray(self.payload, dtype=np.uint32).reshape(-1)
        if self.stats is None:
            uniform, dense = int(self.headers[:, 3].sum(dtype=np.uint64)), int(self.headers[:, 4].sum(dtype=np.uint64))
            self.stats = (512 * self.n_chunks - uniform - dense, uniform, dense, 4 * (self.headers.size + self.payload_words))

    @property
    def n_chunks(self) -> int:
        return int(self.headers.shape[0])

    @property
    def payload_words(self) -> int:
        return int(self.payload.shape[0])

    @property
    def on_device(self) -> bool:
        return not isinstance(self.payload, np.ndarray)

    @property
    def keys(self) -> list:
        return [tuple(int(v) for v in k) for k in self.headers[:, :3].view(np.int32)]

    @property
    def offsets(self) -> np.ndarray:
        """the index of every chunk's first payload word (uint64)"""
        return self.headers[:, 5].astype(np.uint64) | (self.headers[:, 6].astype(np.uint64) << np.uint64(32))

    @property
    def ratio(self) -> float:
        """packed bytes (headers + payload) / (chunks x 1 MiB); 0 for no chunk"""
        return float(self.stats[3]) / (self.n_chunks * CHUNK_BYTES) if self.n_chunks else 0.0

    def to_host(self) -> "PackedMap":
        if not self.on_device:
            return self
        payload = self.payload.cpu().numpy().view(np.uint32)
        return PackedMap(self.headers, payload, self.fill, self.resolution, self.tau, self.stats, dict(self.meta))

    def check(self):
        """ws_pack_check: raises WsError unless the headers are a valid stream of payload_words words"""
        check(_lib.load().ws_pack_check(_ptr(self.headers), self.n_chunks, self.payload_words), "ws_pack_check")

    def chunk(self, i: int) -> np.ndarray:
        """chunk i expanded on the host (ws_pack_expand_chunk): 262 144 uint32"""
        if self.on_device:
            raise WsError("PackedMap.chunk: the payload is on the device (to_host() first)")
        out = np.empty(CHUNK_WORDS, dtype=np.uint32)
        h = self.headers[i]
        first, words = int(self.offsets[i]), int(h[3]) + 512 * int(h[4])
        own = np.ascontiguousarray(self.payload[first:first + words])
        if own.size != words:
            raise WsError("PackedMap.chunk: the payload is shorter than the header says")
        check(_lib.load().ws_pack_expand_chunk(_ptr(np.ascontiguousarray(h)), _ptr(own) if words else None, int(self.fill), _ptr(out)), "ws_pack_expand_chunk")
        return out

    def save(self, path, **meta):
        """the `.wspk` file: a plain, uncompressed np.savez of version, fill, headers, payload and the metadata"""
        host = self.to_host()
        extra = {**host.meta, **meta}
        for name, value in (("resolution", host.resolution), ("tau", host.tau)):
            if value is not None:
                extra.setdefault(name, value)
        with open(path, "wb") as f:
            np.savez(f, version=np.int32(WSPK_VERSION), fill=np.uint32(host.fill), headers=host.headers, payload=host.payload,
                     **{k: np.asarray(v) for k, v in extra.items()})

    @classmethod
    def load(cls, path) -> "PackedMap":
        with np.load(path, allow_pickle=False) as z:
            if int(z["version"]) != WSPK_VERSION:
                raise WsError(f"{path}: .wspk version {int(z['version'])}, this library reads {WSPK_VERSION}")
            meta = {k: z[k][()] if z[k].ndim == 0 else z[k] for k in z.files if k not in ("version", "fill", "headers", "payload")}
            p = cls(z["headers"], z["payload"], int(z["fill"]), meta=meta)
        p.resolution = int(meta.pop("resolution")) if "resolution" in meta else None
        p.tau = int(meta.pop("tau")) if "tau" in meta else None
        p.check()
        return p

    def to_global_map(self, global_map):
        """every chunk expanded into a host GlobalMap, whole (its chunk cache, or its file as DeviceGlobalMap.flush_to does); no GPU"""
        for i, key in enumerate(self.keys):
            data = self.chunk(i)
            with global_map.lock:
                if global_map._file is not None and key not in global_map.chunks:
                    global_map._write_chunk(key, data)
                else:
                    global_map.activate_chunk(*key)[:] = data
        return global_map

    @classmethod
    def from_global_map(cls, global_map, keys=None, **meta) -> "PackedMap":
        """chunks of a host GlobalMap (None: all it holds, in memory and in its file) packed on the host (ws_pack_chunk) against the
        map's default entry; no GPU"""
        L = _lib.load()
        if keys is None:
            keys = set(global_map.chunks) | (set(global_map._in_file) if global_map._file is not None else set())
        keys = sorted({tuple(int(v) for v in k) for k in keys})
        if any(not global_map.has_chunk(*k) for k in keys):
            raise WsError("PackedMap.from_global_map: the map does not hold a named chunk")
        headers = np.zeros((len(keys), WS_PACK_HEADER_WORDS), dtype=np.uint32)
        parts, first = [], 0
        own = np.empty(CHUNK_WORDS, dtype=np.uint32)
        for i, key in enumerate(keys):
            words = C.c_uint64(0)
            with global_map.lock:
                data = np.ascontiguousarray(global_map.activate_chunk(*key), dtype=np.uint32)
                check(L.ws_pack_chunk(_ptr(data), _i3c(key), int(global_map.default_raw), _ptr(headers[i]), _ptr(own), CHUNK_WORDS, C.byref(words)), "ws_pack_chunk")
            headers[i, 5], headers[i, 6] = first & 0xFFFFFFFF, first >> 32
            parts.append(own[:words.value].copy())
            first += int(words.value)
        payload = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
        return cls(headers, payload, int(global_map.default_raw), meta=dict(meta))


class PackQueries:
    """save_global_packed and load_global_packed of TSDFMapping (mapping.py): the packed file behind the mapping's lock and its window"""

    def save_global_packed(self, path, **meta):
        """Everything the run has seen as one `.wspk` file: the window goes into the chunks of device_global_map exactly as in
        global_mesh, then DeviceGlobalMap.save_packed with the map's resolution and tau as metadata.  The host global map and its
        .h5 file are not touched.  Returns the PackedMap."""
        with self._window_in_store("save_global_packed") as store:
            return store.save_packed(path, **{"resolution": int(self.params_.map.resolution), "tau": int(self.tsdf_.tau_), **meta})

    def load_global_packed(self, path):
        """The chunks of a `.wspk` file into device_global_map, to continue a saved map: the window goes into the chunks first, the
        file's chunks replace those they name, and the window is loaded back from the chunks, so that it holds the loaded voxels.
        A file of another resolution is refused.  Returns the PackedMap."""
        packed = PackedMap.load(path)
        if packed.resolution is not None and packed.resolution != int(self.params_.map.resolution):
            raise WsError(f"load_global_packed: {path} has resolution {packed.resolution}, the map {int(self.params_.map.resolution)}")
        with self._window_in_store("load_global_packed") as store:
            store.unpack(packed)
            lo, hi = self.local_map_.window()
            store.load_box(self.tsdf_, lo, hi)
            self._pyramid_touch()  # (the file's chunks may lie anywhere: global_pyramid rebuilds)
        return packed


def _pack_call(L, store, keys, device, direct=False) -> PackedMap:
    """ws_store_pack on store.handle and its result"""
    n, words = C.c_size_t(0), C.c_uint64(0)
    stats = (C.c_uint64 * 4)()
    if keys is None:
        kp, nk = None, 0
    else:
        karr = np.ascontiguousarray(np.asarray(keys, dtype=np.int32).reshape(-1, 3))
        kp, nk = _ptr(karr), int(karr.shape[0])
        if nk == 0:
            return PackedMap(np.zeros((0, WS_PACK_HEADER_WORDS), np.uint32), np.zeros(0, np.uint32), store.default_raw, stats=(0, 0, 0, 0))
    check(L.ws_store_pack(store.handle, kp, nk, _lib.WS_PACK_EMIT_DIRECT if direct else _lib.WS_PACK_DEFAULT, C.byref(n), C.byref(words), stats), "ws_store_pack")
    n, words = int(n.value), int(words.value)
    headers = np.zeros((n, WS_PACK_HEADER_WORDS), dtype=np.uint32)
    payload = np.zeros(0 if device else words, dtype=np.uint32)
    n2, w2 = C.c_size_t(0), C.c_uint64(0)
    check(L.ws_store_pack_download(store.handle, _ptr(headers) if n else None, _ptr(payload) if words and not device else None, n, payload.size, C.byref(n2),
                                   C.byref(w2)), "ws_store_pack_download")
    if device:
        w3 = C.c_uint64(0)
        ptr = L.ws_store_pack_payload_dev(store.handle, C.byref(w3))
        payload = _device_tensor(ptr, (words,), "<i4", store)
    return PackedMap(headers, payload, store.default_raw, stats=tuple(int(v) for v in stats))


def _unpack_call(L, store, packed: PackedMap):
    """ws_store_unpack / ws_store_unpack_dev of `packed` into store.handle"""
    n, words = packed.n_chunks, packed.payload_words
    if packed.on_device:
        ptr = C.c_void_p(int(packed.payload.data_ptr())) if words else None
        check(L.ws_store_unpack_dev(store.handle, _ptr(packed.headers) if n else None, ptr, n, words, int(packed.fill), 0), "ws_store_unpack_dev")
    else:
        check(L.ws_store_unpack(store.handle, _ptr(packed.headers) if n else None, _ptr(packed.payload) if words else None, n, words, int(packed.fill), 0),
              "ws_store_unpack")
