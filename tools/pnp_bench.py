#!/usr/bin/env python3
"""Device-path timing of sfmx_register_poses (not run by any test).

`--sets` candidate sets of `--points` 3D-2D points each: landmarks at depth 4-9 seen by a 1200-focal camera
under a planted pose, `--noise` px noise, every 4th point with a wrong partner (25 %), points resident on the
device.  Prints one JSON line per configuration: kernel time from the call's HIP events
(sfmx_register_poses_last_kernel_ms, median of `--steps` calls after `--warmup`, with min and max), sets/s and
what the call found.  Without --sets both configurations of DESIGN.md §8i run: 1 set (the loop's own call) and 50.

    python tools/pnp_bench.py [--sets 50] [--points 2000] [--steps 20] [--warmup 3] [--threshold -8.0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "sfm-mvs-pipeline_amd")]


def candidate_sets(n_sets, n_points, noise, seed):
    """-> (points3d, points2d, offsets, camera (K, dist), size)."""
    rng = np.random.default_rng(seed)
    f, w, h = 1200.0, 1600, 1200
    K = np.array([f, 0, w / 2, 0, f, h / 2, 0, 0, 1.0])
    p3, p2 = [], []
    for s in range(n_sets):
        a = 0.1 + 0.01 * s                                   # a rotation about y and a shift, different per set
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        t = np.array([0.2 - 0.01 * s, -0.1, 0.5])
        X = np.stack([rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(4, 9, n_points)], axis=1)
        Xc = X @ R.T + t
        px = np.stack([Xc[:, 0] / Xc[:, 2] * f + w / 2, Xc[:, 1] / Xc[:, 2] * f + h / 2], axis=1)
        px += noise * rng.standard_normal(px.shape)
        px[3::4] = np.stack([rng.uniform(0, w, len(px[3::4])), rng.uniform(0, h, len(px[3::4]))], axis=1)
        p3.append(X)
        p2.append(px)
    off = np.arange(n_sets + 1, dtype=np.int64) * n_points
    return np.concatenate(p3), np.concatenate(p2), off, (K, np.zeros(5)), (w, h)


def run(a, n_sets):
    import torch
    from sfmx import pnp
    p3, p2, off, cam, size = candidate_sets(n_sets, a.points, a.noise, a.seed)
    d3, d2, do = torch.from_numpy(p3).cuda(), torch.from_numpy(p2).cuda(), torch.from_numpy(off).cuda()
    call = lambda: pnp.register_poses_device(d3.data_ptr(), d2.data_ptr(), do.data_ptr(), len(p3), np.zeros(n_sets, np.int32),
                                             [cam], [0], [size], threshold=a.threshold)
    for _ in range(a.warmup):
        r = call()
    ms, wall = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        r = call()                                   # returns after its stream synchronised
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(pnp.last_kernel_ms())
    kernel_ms = float(np.median(ms))
    print(json.dumps({
        "tool": "pnp_bench", "sets": n_sets, "points_per_set": a.points, "noise_px": a.noise, "threshold": a.threshold,
        "posed": int((r["status"] == 1).sum().item()), "inliers": int(r["n_inliers"].sum().item()),
        "kernel_ms": round(kernel_ms, 4), "kernel_ms_min": round(float(np.min(ms)), 4),
        "kernel_ms_max": round(float(np.max(ms)), 4), "call_wall_ms": round(float(np.median(wall)), 4),
        "sets_per_s": round(n_sets / (kernel_ms * 1e-3), 1), "steps": a.steps, "warmup": a.warmup}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=0)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=-8.0)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pnp_bench: no GPU visible (there is no CPU path to time)")
    for n_sets in ([a.sets] if a.sets else [1, 50]):
        run(a, n_sets)


if __name__ == "__main__":
    main()
