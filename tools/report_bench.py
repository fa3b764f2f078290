#!/usr/bin/env python3
"""Device-path timing of sfmx_reprojection_errors and sfmx_colorize_pointcloud at the BA bench size (not run by
any test).

The scene is sfmx.synth.ba_problem: `--shots` cameras on a ring, `--points` points with `--obs` origin records
each (200 / 200 000 / 6: 1.2 M records), resident on the device, with one 720x405 BGR image per shot.  Prints one
JSON line per kernel: the kernel time from the call's HIP events (median of `--steps` calls after `--warmup`),
min, max, records or points per second, the bytes the kernel must touch (reprojection: 4 + 16 B read and 8 B
written per record, 24 + 8 B read per point; colour: 4 B per record, 8 + 16 + 3 B read and 3 + 8 B written per
point) over the kernel time and the HBM peak.  A third line has the host wall time of the statistics and the
histogram of the same error list, whose sort is not on the device.

    python tools/report_bench.py [--shots 200] [--points 200000] [--obs 6] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sfm-mvs-pipeline_amd"))

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak, as bench.py


def line(tool, unit, count, ms, touched, **extra):
    t = float(np.median(ms)) * 1e-3
    return dict(tool=tool, **extra, kernel_ms=round(t * 1e3, 4), kernel_ms_min=round(min(ms), 4), kernel_ms_max=round(max(ms), 4),
                **{unit + "_per_s": round(count / t, 1)}, bytes_touched=int(touched), hbm_frac=round(touched / t / (HBM_PEAK_GBS * 1e9), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=200)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--obs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from sfmx import report, synth
    if not torch.cuda.is_available():
        sys.exit("report_bench: no GPU visible (there is no CPU path to time)")
    W, H = 720, 405
    p = synth.ba_problem(a.shots, a.points, a.obs, cam_model=3, width=W, height=H)
    n, m = a.points, a.points * a.obs
    K = np.array([[p["intr"][0], 0, p["cx"]], [0, p["intr"][0], p["cy"]], [0, 0, 1.0]])
    cameras = [(K, np.array([p["intr"][1], p["intr"][2], 0, 0, 0]))]
    pose = np.zeros((a.shots, 3, 4))
    for i, q in enumerate(p["poses"]):
        pose[i, :, :3] = synth._R_from_aa(q[:3])
        pose[i, :, 3] = q[3:]
    xyz = torch.from_numpy(p["points"]).cuda()
    off = torch.arange(0, m + 1, a.obs, dtype=torch.int64, device="cuda")
    osh = torch.from_numpy(p["obs_cam"].astype(np.int32)).cuda()
    oxy = torch.from_numpy(np.ascontiguousarray(p["obs_xy"], np.float64)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    images = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(a.shots)]
    common = dict(shots=a.shots, points=n, records=m, steps=a.steps, warmup=a.warmup)
    ms, err = [], None
    for i in range(a.warmup + a.steps):
        err = report.reprojection_errors_device(xyz, off, osh, oxy, cameras, np.zeros(a.shots, np.int32), pose)
        if i >= a.warmup:
            ms.append(report.reprojection_last_kernel_ms())
    print(json.dumps(line("report_bench.reprojection", "records", m, ms, m * (4 + 16 + 8) + n * (24 + 8), **common,
                          mean_error=float(err.mean().item()))))
    ms = []
    for i in range(a.warmup + a.steps):
        rgb, rec = report.colorize_pointcloud_device(n, off, osh, oxy, images)
        if i >= a.warmup:
            ms.append(report.colorize_last_kernel_ms())
    print(json.dumps(line("report_bench.colorize", "points", n, ms, m * 4 + n * (8 + 16 + 3 + 3 + 8), **common,
                          coloured=int((rec >= 0).sum().item()))))
    e = err.cpu().numpy()
    t0 = time.perf_counter()
    s = report.error_statistics(e)
    t1 = time.perf_counter()
    k, _ = report.error_histogram(e)
    t2 = time.perf_counter()
    print(json.dumps(dict(tool="report_bench.host", records=m, statistics_wall_ms=round((t1 - t0) * 1e3, 3),
                          histogram_wall_ms=round((t2 - t1) * 1e3, 3), histogram_rows=len(k), mean=s["mean"], median=s["median"])))


if __name__ == "__main__":
    main()
