#!/usr/bin/env python3
"""Where two global maps differ, on the device (ws_store_changes): CUR ("now") is compared on its own lattice with REF ("before")
under a pose -- what has appeared, what has been taken away, how large and where.

    python tools/diff_maps.py now.h5 before.h5 --resolution 64 --tau 600 --xyz-mm 13 -7 4 --rpy-deg 0 3 17 --ply changes.ply
    python tools/diff_maps.py now.npz before.npz --pose pose.txt --align --window 257 --min-size 20

The maps (.h5, .npz or .wspk), the pose options and --align are those of tools/merge_maps.py; the pose takes points of REF into the frame of CUR.  --band
and --free-value are raw values (defaults: the resolution and tau).  Prints the statistics and the clusters of at least --min-size
voxels (largest first: kinds, size, volume, centroid in metres, bounding box in voxels) as one JSON line; --ply writes the records
as a point cloud, appeared green and vanished red."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warpsense_amd as W  # noqa: E402
from merge_maps import load, pose_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cur")
    ap.add_argument("ref")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--tau", type=int, default=600)
    ap.add_argument("--band", type=int, default=None, help="occupied iff |value| < band (default: the resolution)")
    ap.add_argument("--free-value", type=int, default=None, help="free iff value >= free_value (default: tau)")
    ap.add_argument("--min-weight", type=int, default=1)
    ap.add_argument("--kinds", choices=("both", "appeared", "vanished"), default="both")
    ap.add_argument("--min-size", type=int, default=1, help="clusters below this many voxels are not printed")
    ap.add_argument("--pose", help="text file, 4 x 4, mm")
    ap.add_argument("--xyz-mm", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--rpy-deg", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--pivot-src-mm", type=float, nargs=3, default=None, help="the pivot in the frame of REF")
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--window", type=int, default=257, help="--align: edge of the window of CUR, voxels")
    ap.add_argument("--centre-vox", type=int, nargs=3, default=(0, 0, 0), help="--align: where that window stands")
    ap.add_argument("--max-points", type=int, default=65536)
    ap.add_argument("--ply", help="write the records as a PLY point cloud")
    a = ap.parse_args()
    T = pose_of(a)
    cur, ref = W.DeviceGlobalMap(a.tau, 0), W.DeviceGlobalMap(a.tau, 0)
    cur.load_from(load(a.cur, a.tau))
    ref.load_from(load(a.ref, a.tau))
    if a.align:
        params = W.MapParams(resolution=a.resolution, max_distance=a.tau / 1000.0, max_weight=10.0, size=(a.window * a.resolution / 1000.0,) * 3)
        lm = W.LocalMap(a.window, a.window, a.window, a.tau, 0)
        lm.pos[:] = a.centre_vox
        reg = W.TSDFRegistration(W.Params(params), lm)
        lo, hi = lm.window()
        cur.load_box(reg.tsdf(), lo, hi)
        T = reg.align_map(ref, T, max_points=a.max_points)
    res = cur.changes(ref, T, a.pivot_src_mm, resolution=a.resolution, band=a.resolution if a.band is None else a.band,
                      free_value=a.tau if a.free_value is None else a.free_value, min_weight=a.min_weight, kinds=a.kinds, clusters=True)
    if a.ply:
        W.write_changes_ply(a.ply, res, a.resolution)
    st, table, kinds = res.stats, res.clusters, res.cluster_kinds()
    order = [int(i) for i in np.lexsort((table["first"], -table["count"].astype(np.int64))) if table["count"][i] >= a.min_size]
    names = {1: "appeared", 2: "vanished", 3: "moved"}
    clusters = [dict(kind=names[int(kinds[i])], voxels=int(table["count"][i]), volume_m3=int(table["count"][i]) * (a.resolution / 1000.0) ** 3,
                     centroid_m=((table["sum"][i] / table["count"][i] + 0.5) * a.resolution / 1000.0).tolist(), lo=table["lo"][i].tolist(), hi=table["hi"][i].tolist())
                for i in order]
    print(json.dumps(dict(chunks=st.chunks, known_both=st.known_both, appeared=st.appeared, vanished=st.vanished, new_ground=st.new_ground,
                          sum_abs_diff=st.sum_abs_diff, disagreement_mm=None if not st.known_both else st.disagreement_mm,
                          changed_volume_m3=st.changed_volume_m3(a.resolution), records=len(res.records), clusters_total=len(table), clusters=clusters,
                          pose=np.asarray(T, dtype=np.float64).tolist())))


if __name__ == "__main__":
    main()
