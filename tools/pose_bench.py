#!/usr/bin/env python3
"""Device-path timing of sfmx_relative_poses on a C2-shaped graph (not run by any test).

The scene of tools/triangulate_bench.py: 50 shots on a ring looking at a landmark cloud, all 1225 unordered
pairs, `--matches-per-pair` matches each, every 4th with a wrong partner (25 %), keypoints and match lists
resident on the device.  Prints one JSON line: kernel time from the call's HIP events
(sfmx_relative_poses_last_kernel_ms, median of `--steps` calls after `--warmup`, with min and max), pairs/s,
matches/s and what the call found.

    python tools/pose_bench.py [--matches-per-pair 4000] [--steps 20] [--warmup 3] [--threshold -1.0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "sfm-mvs-pipeline_amd"), os.path.dirname(os.path.abspath(__file__))]

from triangulate_bench import graph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=50)
    ap.add_argument("--landmarks", type=int, default=8192)
    ap.add_argument("--matches-per-pair", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=-1.0)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    from sfmx import pose
    if not torch.cuda.is_available():
        sys.exit("pose_bench: no GPU visible (there is no CPU path to time)")
    kps, cams, sc, _, pairs, m, off = graph(a.shots, a.landmarks, a.matches_per_pair, a.seed)
    rng = np.random.default_rng(a.seed + 2)
    t = m["queryIdx"].copy()                               # the right partner is the same landmark ...
    t[3::4] = rng.integers(0, a.landmarks, len(t[3::4]))   # ... but for every 4th match
    m["trainIdx"] = t
    K = cams[0][0]
    size = np.tile(np.array([[int(2 * K[2]), int(2 * K[5])]], np.int32), (a.shots, 1))
    dk = [torch.from_numpy(k).cuda() for k in kps]
    dm = torch.from_numpy(m.view(np.uint8)).cuda()
    do = torch.from_numpy(off).cuda()
    call = lambda: pose.relative_poses_device([x.data_ptr() for x in dk], [len(k) for k in kps], cams, sc, size, pairs,
                                              dm.data_ptr(), do.data_ptr(), len(m), threshold=a.threshold)
    for _ in range(a.warmup):
        r = call()
    ms, wall = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        r = call()                                   # returns after its stream synchronised
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(pose.last_kernel_ms())
    n = len(m)
    kernel_ms = float(np.median(ms))
    print(json.dumps({
        "tool": "pose_bench", "shots": a.shots, "pairs": len(pairs), "matches": n, "matches_per_pair": a.matches_per_pair,
        "threshold": a.threshold, "posed": int(r["status"].sum().item()), "inliers": int(r["pair_offsets"][-1].item()),
        "kernel_ms": round(kernel_ms, 4), "kernel_ms_min": round(float(np.min(ms)), 4),
        "kernel_ms_max": round(float(np.max(ms)), 4), "call_wall_ms": round(float(np.median(wall)), 4),
        "pairs_per_s": round(len(pairs) / (kernel_ms * 1e-3), 1), "matches_per_s": round(n / (kernel_ms * 1e-3), 1),
        "steps": a.steps, "warmup": a.warmup}))


if __name__ == "__main__":
    main()
