#!/usr/bin/env python3
"""Timing and ratio of the packed snapshots (ws_store_pack / ws_store_unpack) on the store a replayed run leaves; writes
profiles/pack_timing.json.

The store is the one that
    python tools/replay_stream.py --map 1024 --scans 60 --shift 2.0 --room 10 8 2.5 --device-global-map --global-packed run.wspk
leaves: its snapshot is lossless, so --wspk run.wspk gives this tool that store byte for byte (DeviceGlobalMap.load_packed).

Measured, per 2 warm-up calls and --calls timed ones (medians with minimum and maximum):
  * the three class shares and ratio = packed bytes / (chunks x 1 MiB);
  * device ms of classify, scan and emit (staged through LDS, and WS_PACK_EMIT_DIRECT) and of the unpack launch, with the chunk bytes
    each pass reads or writes over its time in TB/s, next to a device-to-device copy of the store's size measured in the same run;
  * wall clock of pack() with its download against [store.chunk(k) for k in store.keys()] on the same store in the same process;
  * wall clock of load_packed against load_from on the equivalent host GlobalMap;
  * the file's size against the .npz of tools/merge_maps.py (np.savez_compressed of whole chunks)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warpsense_amd as W  # noqa: E402
from changes_timing import copy_ms  # noqa: E402
from fuse_timing import spread  # noqa: E402
from merge_maps import save as save_any  # noqa: E402

MIB = 4 * 64 ** 3


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wspk", required=True, help="the snapshot of the store to measure on (replay_stream.py --global-packed)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--wall-calls", type=int, default=3)
    ap.add_argument("--no-npz", action="store_true", help="skip the .npz of whole chunks (minutes of zlib on a large store)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_timing.json"))
    a = ap.parse_args()
    warm = 2
    file_packed = W.PackedMap.load(a.wspk)
    value, weight = (int(v) for v in W.unpack_entry(file_packed.fill))
    store = W.DeviceGlobalMap(value, weight)
    store.reserve(file_packed.n_chunks)
    store.unpack(file_packed)
    n = store.count()
    chunk_bytes = n * MIB
    d2d = copy_ms(min(chunk_bytes, 4 << 30), warm, a.calls)
    d2d_bytes = min(chunk_bytes, 4 << 30)
    copy_tbs = 2.0 * d2d_bytes / (float(np.median(d2d)) * 1e-3) / 1e12  # a copy reads and writes every byte
    out = dict(wspk=os.path.basename(a.wspk), resolution=file_packed.resolution, tau=file_packed.tau, chunks=n, chunk_bytes=chunk_bytes,
               d2d_copy_bytes=d2d_bytes, d2d_copy_ms=spread(d2d), d2d_copy_tb_s=copy_tbs)

    # ---- classes and ratio
    p = store.pack()
    assert p.headers.tobytes() == file_packed.headers.tobytes() and p.payload.tobytes() == file_packed.payload.tobytes()  # lossless, and the same bytes again
    bricks = 512 * n
    out.update(bricks=dict(default=p.stats[0], uniform=p.stats[1], dense=p.stats[2]),
               shares=dict(default=p.stats[0] / bricks, uniform=p.stats[1] / bricks, dense=p.stats[2] / bricks),
               packed_bytes=p.stats[3], payload_words=p.payload_words, ratio=p.ratio)

    # ---- device milliseconds
    store.pack_timing(1)
    dev = {}
    for name, direct in (("staged", False), ("direct", True)):
        rows = []
        for i in range(warm + a.calls):
            store.pack(device=True, direct=direct)
            if i >= warm:
                rows.append(store.pack_timing())
        dev[name] = np.asarray(rows)
    store.pack_timing(0)
    payload_bytes = 4 * p.payload_words
    nondefault_columns = int(sum(len({b >> 3 for b in range(512) if (int(h[8 + b // 16]) >> (2 * (b % 16))) & 3}) for h in p.headers))
    emit_read = nondefault_columns * 8 * 512 * 4  # the brick columns with a non-default brick are read whole
    tbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12
    cls = float(np.median(dev["staged"][:, 0]))
    out["pack_device_ms"] = dict(classify=spread(dev["staged"][:, 0]), scan=spread(dev["staged"][:, 1]), emit_staged=spread(dev["staged"][:, 2]),
                                 emit_direct=spread(dev["direct"][:, 2]))
    out["pack_device_tb_s"] = dict(classify_read=tbs(chunk_bytes, cls), emit_staged_read_plus_write=tbs(emit_read + payload_bytes, float(np.median(dev["staged"][:, 2]))),
                                   emit_direct_read_plus_write=tbs(emit_read + payload_bytes, float(np.median(dev["direct"][:, 2]))), emit_bytes_read=emit_read,
                                   emit_bytes_written=payload_bytes)
    target = W.DeviceGlobalMap(value, weight)
    target.reserve(n)
    target.pack_timing(1)
    rows = []
    on_dev = store.pack(device=True)
    for i in range(warm + a.calls):
        target.unpack(on_dev)
        ms = target.pack_timing()
        if i >= warm:
            rows.append(ms[0])
    target.pack_timing(0)
    out["unpack_device_ms"] = spread(rows)
    out["unpack_device_tb_s"] = dict(write_plus_read=tbs(chunk_bytes + payload_bytes, float(np.median(rows))))
    clone_ms = [wall(lambda: store.clone().close())[1] for _ in range(a.wall_calls)]
    out["clone_wall_ms"] = spread(clone_ms)
    target.close()

    # ---- wall clock out of the device
    keys = store.keys()
    pack_ms = [wall(lambda: store.pack())[1] for _ in range(a.wall_calls)]
    loop_ms = [wall(lambda: [store.chunk(k) for k in keys])[1] for _ in range(a.wall_calls)]
    out["export_wall_ms"] = dict(pack_and_download=spread(pack_ms), per_chunk_loop=spread(loop_ms), loop_over_pack=float(np.median(loop_ms)) / float(np.median(pack_ms)))

    # ---- wall clock into the device
    host = file_packed.to_global_map(W.GlobalMap(value, weight))
    load_packed_ms, load_from_ms = [], []
    for _ in range(a.wall_calls):
        fresh = W.DeviceGlobalMap(value, weight)
        fresh.reserve(n)
        load_packed_ms.append(wall(lambda: fresh.load_packed(a.wspk))[1])
        fresh.close()
        fresh = W.DeviceGlobalMap(value, weight)
        fresh.reserve(n)
        load_from_ms.append(wall(lambda: fresh.load_from(host))[1])
        fresh.close()
    out["import_wall_ms"] = dict(load_packed_with_file_read=spread(load_packed_ms), load_from_host_map=spread(load_from_ms),
                                 load_from_over_load_packed=float(np.median(load_from_ms)) / float(np.median(load_packed_ms)))

    # ---- the files
    out["wspk_file_bytes"] = os.path.getsize(a.wspk)
    if not a.no_npz:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "whole.npz")
            _, npz_ms = wall(lambda: save_any(store, path, file_packed.tau or value, None))
            _, wspk_ms = wall(lambda: store.save_packed(os.path.join(d, "again.wspk")))
            out["npz_file_bytes"], out["npz_save_wall_ms"], out["wspk_save_wall_ms"] = os.path.getsize(path), npz_ms, wspk_ms
            out["wspk_over_npz_bytes"] = out["wspk_file_bytes"] / out["npz_file_bytes"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
