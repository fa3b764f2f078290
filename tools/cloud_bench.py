#!/usr/bin/env python3
"""Device-path timing of sfmx_cloud_neighbor_distances on a synthetic surface cloud (not run by any test).

`--points` points on a few noisy spheres and planes (the shape of a dense MVS cloud: two-dimensional
sheets in space) plus 0.01 % far outliers 10^3 .. 10^6 scene sizes away, shuffled, resident on the device.
Prints one JSON line: the kernel time from the call's HIP events (sfmx_cloud_last_stats, median of
`--steps` calls after `--warmup`), points/s, evaluations of d per point, the queries resolved by the
brute-force kernel, and the bytes the kernels must touch (12 B per point read by each of the seven passes
over the input: min/max, three histograms, two counts, the scatter; cell and rank written twice and read once;
the 16-byte sorted record written and read once; 8 + 8 B of output; the cell counters cleared once) over the
kernel time and the HBM peak.  The records the search re-reads from the caches are not counted.

    python tools/cloud_bench.py [--points 4000000] [--steps 10] [--warmup 2] [--max-equal 0]
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


def surface_cloud(n, seed):
    rng = np.random.default_rng(seed)
    n_out = max(1, n // 10000)
    n_surf = n - n_out
    parts, left = [], n_surf
    shapes = [("sphere", (0, 0, 0), 1.0), ("sphere", (2.5, 0.3, -0.4), 0.6), ("sphere", (-1.0, 2.0, 0.5), 0.8),
              ("plane", (0, 0, -1.2), 4.0), ("plane", (0, -2.0, 0), 3.0)]
    for k, (kind, c, s) in enumerate(shapes):
        m = left if k == len(shapes) - 1 else n_surf // len(shapes)
        left -= m
        if kind == "sphere":
            v = rng.normal(size=(m, 3))
            p = v / np.linalg.norm(v, axis=1, keepdims=True) * s * (1 + 0.001 * rng.normal(size=(m, 1)))
        else:
            p = np.concatenate([(rng.random((m, 2)) - 0.5) * s, 0.001 * rng.normal(size=(m, 1))], 1)
            if k == len(shapes) - 1:
                p = p[:, [0, 2, 1]]
        parts.append(p + np.asarray(c))
    far = rng.normal(size=(n_out, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * 10.0 ** rng.uniform(3, 6, size=(n_out, 1)) * 5.0
    x = np.concatenate(parts + [far]).astype(np.float32)
    return x[rng.permutation(len(x))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--max-equal", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    from sfmx import cloud
    if not torch.cuda.is_available():
        sys.exit("cloud_bench: no GPU visible (there is no CPU path to time)")
    x = torch.from_numpy(surface_cloud(a.points, a.seed)).cuda()
    n = x.shape[0]
    ms, wall, st = [], [], {}
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        d, nb = cloud.neighbor_distances(x, a.max_equal, neighbors=True)   # returns after its stream synchronised
        w = (time.perf_counter() - t0) * 1e3
        st = cloud.last_stats()
        if i >= a.warmup:
            ms.append(st["kernel_ms"])
            wall.append(w)
    t = float(np.median(ms)) * 1e-3
    cells = 16 * min(max(n, 64), 1 << 23) + 2
    touched = n * (7 * 12 + 3 * 8 + 2 * 16 + 16) + cells * 4
    finite = torch.isfinite(d)
    print(json.dumps({
        "tool": "cloud_bench", "points": n, "max_equal": a.max_equal, "steps": a.steps, "warmup": a.warmup,
        "kernel_ms": round(t * 1e3, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
        "call_wall_ms": round(float(np.median(wall)), 4),
        "points_per_s": round(n / t, 1), "evaluations_per_point": round(st["evaluations"] / n, 2),
        "brute_queries": st["brute_queries"], "bytes_touched": touched,
        "hbm_frac": round(touched / t / (HBM_PEAK_GBS * 1e9), 4),
        "mean_distance": float(d[finite].mean().item()), "zero_distances": int((d == 0).sum().item()),
    }))


if __name__ == "__main__":
    main()
