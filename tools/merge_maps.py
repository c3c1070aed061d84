#!/usr/bin/env python3
"""Merge two global maps on the device (ws_store_fuse): SRC is resampled on the lattice of DST under a pose and integrated into it.

    python tools/merge_maps.py dst.h5 src.h5 merged.h5 --resolution 64 --tau 600 --max-weight 640 --xyz-mm 13 -7 4 --rpy-deg 0 3 17
    python tools/merge_maps.py dst.npz src.npz merged.npz --pose pose.txt --align --window 257

Maps are .h5 global maps (where libwarpsense_h5.so is built), .npz chunk dumps with `keys` (n, 3) int32 and `chunks` (n, 262144)
uint32, or .wspk packed snapshots (warpsense_amd.PackedMap: written by the device's pack, read on the host).  The pose takes points of SRC into the frame of DST: a text file with a 4 x 4 matrix in mm, or --xyz-mm and --rpy-deg (roll,
pitch, yaw; R = Rz Ry Rx).  --align refines it first (TSDFRegistration.align_map against a window of DST around --centre-vox).
Prints the statistics as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import warpsense_amd as W  # noqa: E402


def load(path, tau):
    """a host GlobalMap of the file"""
    if path.endswith(".wspk"):
        return W.PackedMap.load(path).to_global_map(W.GlobalMap(tau, 0))
    if path.endswith(".npz"):
        z = np.load(path)
        g = W.GlobalMap(tau, 0)
        for key, data in zip(z["keys"], z["chunks"]):
            g.activate_chunk(*(int(v) for v in key))[:] = data
        return g
    return W.GlobalMap(tau, 0, filename=path, open_existing=True)


def save(store, path, tau, params):
    if path.endswith(".wspk"):
        store.save_packed(path, tau=int(tau), **({"resolution": int(params.resolution)} if hasattr(params, "resolution") else {}))
        return
    if path.endswith(".npz"):
        keys = store.keys()
        np.savez_compressed(path, keys=np.asarray(keys, dtype=np.int32).reshape(-1, 3),
                            chunks=np.stack([store.chunk(k) for k in keys]) if keys else np.zeros((0, 64 ** 3), dtype=np.uint32))
        return
    g = W.GlobalMap(tau, 0, filename=path, map_params=params)
    store.flush_to(g)
    g.close()


def pose_of(a):
    if a.pose:
        return np.loadtxt(a.pose, dtype=np.float64).reshape(4, 4)
    r, p, y = np.deg2rad(a.rpy_deg)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, a.xyz_mm
    return T


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dst")
    ap.add_argument("src")
    ap.add_argument("out")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--tau", type=int, default=600)
    ap.add_argument("--max-weight", type=int, default=640, help="as the entries hold it (map/max_weight x 64)")
    ap.add_argument("--pose", help="text file, 4 x 4, mm")
    ap.add_argument("--xyz-mm", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--rpy-deg", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--pivot-src-mm", type=float, nargs=3, default=None)
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--window", type=int, default=257, help="--align: edge of the window of DST, voxels")
    ap.add_argument("--centre-vox", type=int, nargs=3, default=(0, 0, 0), help="--align: where that window stands")
    ap.add_argument("--max-points", type=int, default=65536)
    ap.add_argument("--count-only", action="store_true", help="print the statistics, write nothing")
    a = ap.parse_args()
    T = pose_of(a)
    dst, src = W.DeviceGlobalMap(a.tau, 0), W.DeviceGlobalMap(a.tau, 0)
    dst.load_from(load(a.dst, a.tau))
    src.load_from(load(a.src, a.tau))
    params = W.MapParams(resolution=a.resolution, max_distance=a.tau / 1000.0, max_weight=a.max_weight / 64.0, size=(a.window * a.resolution / 1000.0,) * 3)
    if a.align:
        lm = W.LocalMap(a.window, a.window, a.window, a.tau, 0)
        lm.pos[:] = a.centre_vox
        reg = W.TSDFRegistration(W.Params(params), lm)
        lo, hi = lm.window()
        dst.load_box(reg.tsdf(), lo, hi)
        T = reg.align_map(src, T, max_points=a.max_points)
    st = dst.fuse(src, T, a.max_weight, count_only=a.count_only, pivot_src_mm=a.pivot_src_mm, resolution=a.resolution)
    if not a.count_only:
        save(dst, a.out, a.tau, params)
    print(json.dumps(dict(candidates=st.candidates, created=st.created, averaged=st.averaged, set=st.set, sum_abs_diff=st.sum_abs_diff,
                          sum_min_weight=st.sum_min_weight, disagreement_mm=None if not st.averaged else st.disagreement_mm,
                          chunks=dst.count(), pose=np.asarray(T, dtype=np.float64).tolist())))


if __name__ == "__main__":
    main()
