"""Randomised parity soak of the TSDF update against the CPU oracle (bit-exact avg_map after 1-2 scans): random map
sizes, resolutions, truncation distances, sensor positions (incl. off-centre windows), rooms larger and smaller than the
window, tilted `up` vectors, odd resolutions, any tau and max_weight, windows with a ring offset and far from the origin (beyond
the biased route's reach, MarchFrame::biased_ok).  The fixed-seed cases live in tests/test_gpu_tsdf.py and
tests/test_gpu_tsdf_domain.py; this is for changes to the ray arithmetic (ws_march.h, ray_setup_kernel).

    python tools/soak_tsdf.py [--cases 30] [--seed 1]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=30)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch
    import oracle_lib as O
    import warpsense_amd as W
    from warpsense_amd import synthetic as S
    rng = np.random.default_rng(args.seed)
    bad = 0
    for case in range(args.cases):
        res = int(rng.choice([3, 7, 16, 20, 25, 32, 50, 51, 64, 75, 100, 333])) if rng.random() < 0.7 else int(rng.integers(2, 200))
        tau = int(min(32767, rng.integers(max(2, res // 2), 25 * res + 1)))
        size = tuple(int(rng.integers(20, 70)) * 2 + 1 for _ in range(3))  # (odd: the window is centred on pos)
        mw = int(rng.choice([1, 64, 65, 640, 640, 32767]))
        # the window: centred on the origin, or anywhere with a ring offset, or far away (biased_ok false)
        kind = rng.choice(["origin", "shifted", "far"], p=[0.4, 0.4, 0.2])
        pos = np.zeros(3, dtype=np.int64)
        offset = np.array([s // 2 for s in size], dtype=np.int64)
        if kind != "origin":
            offset = np.array([int(rng.integers(0, s)) for s in size], dtype=np.int64)
            pos = np.array([int(rng.integers(-500, 501)) for _ in range(3)], dtype=np.int64)
        if kind == "far":
            pos[0] = ((1 << 22) if res < 256 else (1 << 30) // res) + int(rng.integers(0, 50))
            pos[0] *= int(rng.choice([-1, 1]))
        n_vox = int(np.prod(size))
        view = W.DeviceMap(size, offset, np.full(n_vox, O.pack(tau, 0), dtype=np.uint32), pos)
        oa = O.OracleMap(size, tau, 0, pos=tuple(int(v) for v in pos), offset=tuple(int(v) for v in offset))
        on = oa.copy()
        t = W.TSDFCuda(view, tau, mw, res)
        ext = np.array(size, dtype=np.float64) * res
        he = ext * rng.uniform(0.2, 0.7, 3)  # rooms smaller and larger than the window (half extent 0.5)
        sensor_vox = np.array([int(rng.integers(-s // 5, s // 5 + 1)) for s in size])  # relative to the window's centre
        up = (0, 0, 32768) if rng.random() < 0.6 else tuple(int(v) for v in np.round(32768 * np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 0.97])))
        ok = True
        for scan in range(int(rng.integers(1, 3))):
            sensor_mm = tuple((sensor_vox * res + res // 2).astype(np.float64) + rng.uniform(-5, 5, 3))
            sensor_mm = tuple(np.clip(sensor_mm, -he * 0.9, he * 0.9))
            pts = S.os1_128_scan(sensor_mm=sensor_mm, rings=int(rng.choice([8, 16, 32])), azimuths=int(rng.choice([64, 128, 256])),
                                 half_extents_mm=tuple(he), seed=int(rng.integers(1, 1 << 30)), yaw_rad=float(rng.uniform(0, 6.28)))
            # the room moves with the window
            pts = (pts.astype(np.int64) + pos * res).astype(np.int32)
            sp = tuple(int(np.floor(v / res)) + int(p) for v, p in zip(sensor_mm, pos))
            O.update_tsdf(oa, on, pts, sp, up, tau, mw, res)
            t.update_tsdf(torch.from_numpy(pts).cuda(), sp, up)
        host = W.DeviceMap(view.size_.copy(), view.offset_.copy(), np.empty_like(view.data_), view.pos_.copy())
        t.avg_map().to_host(host)
        diff = int((host.data_ != oa.data).sum())
        st = t.stats(raise_on_error=False)
        if diff or st["error_flags"]:
            ok = False
            bad += 1
        t.close()
        print(f"case {case:3d}: res {res:3d} tau {tau:5d} mw {mw:5d} size {size} {kind:7s} pos {tuple(int(v) for v in pos)} up {up} records {st['records']:8d} touched tiles {st['tiles']:6d} "
              f"errors {st['error_flags']} -> {'ok' if ok else 'DIFF ' + str(diff)}")
    print(f"{args.cases} cases, {bad} with differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
