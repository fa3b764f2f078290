#!/usr/bin/env python3
"""Device-path timing of sfmx_merge_pointcloud_3d2d on a C2-shaped graph (not run by any test).

tools/triangulate_bench.py's scene: 50 shots on a ring, all 1225 unordered pairs, `--matches-per-pair`
matches each (every 8th a wrong partner), keypoints 0.5 px off the projections, everything resident
on the device.  The pairs are triangulated on the device; the cloud is the merge of the first
`--cloud-pairs` pairs' points into an empty cloud (not timed), and the timed call merges the remaining
pairs' points into that cloud.  Prints one JSON line: kernel time from the call's HIP events
(sfmx_merge_pointcloud_last_kernel_ms, median of `--steps` calls after `--warmup`), wall time of the call
(it includes the per-round word reads and, after a fallback, the host resolution and the staging copies), the
resolve rounds, whether the call fell back to the host and the bytes it copied between host and device
(sfmx_merge_pointcloud_last_path), elements/s on both, the merges into points that
qualify through call-start records (static) and only through what the call itself added (dynamic), and the bytes the kernels must
touch (inputs read, tables written and probed once, outputs written) over the kernel time and the HBM peak.

    python tools/merge_bench.py [--matches-per-pair 1000] [--cloud-pairs 600] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sfm-mvs-pipeline_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak, as bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=50)
    ap.add_argument("--landmarks", type=int, default=8192)
    ap.add_argument("--matches-per-pair", type=int, default=1000)
    ap.add_argument("--cloud-pairs", type=int, default=600)
    ap.add_argument("--point-merge-distance", type=float, default=0.01)
    ap.add_argument("--feature-merge-distance", type=float, default=20.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--max-rounds", type=int, default=0,
                    help="cap on the resolve rounds: 0 the library default, < 0 the host resolution always")
    a = ap.parse_args()
    import torch
    from sfmx import scene, triangulate
    import triangulate_bench
    if not torch.cuda.is_available():
        sys.exit("merge_bench: no GPU visible (there is no CPU path to time)")
    kps, cams, sc, poses, pairs, m, off = triangulate_bench.graph(a.shots, a.landmarks, a.matches_per_pair, a.seed)
    dk = [torch.from_numpy(k).cuda() for k in kps]
    dm = torch.from_numpy(m.view(np.uint8)).cuda()
    do = torch.from_numpy(off).cuda()
    kptr, nkp = [t.data_ptr() for t in dk], [len(k) for k in kps]
    tri = triangulate.triangulate_matches_device(kptr, nkp, cams, sc, poses, pairs, dm.data_ptr(), do.data_ptr(), len(m))
    k0 = int(tri["point_offsets"][min(a.cloud_pairs, len(pairs))].item())
    n = tri["n_points"]

    def part(lo, hi):
        return (tri["xyz"][lo:hi].contiguous(), (tri["origin_offsets"][lo:hi + 1] - 2 * lo).contiguous(),
                tri["origin_shot"][2 * lo:2 * hi].contiguous(), tri["origin_xy"][2 * lo:2 * hi].contiguous())
    dev = tri["xyz"].device
    empty = (torch.zeros((0, 3), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
             torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros((0, 2), dtype=torch.float64, device=dev))
    D, F = a.point_merge_distance, a.feature_merge_distance
    scene.merge_set_max_rounds(a.max_rounds)
    merge = lambda cloud, new: scene.merge_pointcloud_3d2d_device(kptr, nkp, pairs, dm.data_ptr(), do.data_ptr(), *cloud, *new, D, F)
    t0 = time.perf_counter()
    c = merge(empty, part(0, k0))
    setup_ms = (time.perf_counter() - t0) * 1e3
    setup_stats = scene.merge_last_stats()
    cloud = tuple(c[k].contiguous() for k in ("xyz", "origin_offsets", "origin_shot", "origin_xy"))
    new = part(k0, n)
    for _ in range(a.warmup):
        r = merge(cloud, new)
    ms, wall = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        r = merge(cloud, new)                        # returns after its stream synchronised
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(scene.merge_last_kernel_ms())
    st = scene.merge_last_stats()
    path = scene.merge_last_path()
    n_cloud, n_new = len(cloud[0]), len(new[0])
    rc, rn, ro = len(cloud[2]), len(new[2]), len(r["origin_shot"])
    kernel_ms, wall_ms = float(np.median(ms)), float(np.median(wall))
    bytes_in = len(m) * (16 + 16) + 8 * (len(pairs) + 1) + (rc + rn) * 20 + 8 * (n_cloud + n_new + 2) + 24 * (n_cloud + n_new)
    bytes_tables = len(m) * 2 * (12 + 2 * 4) + (rc + rn) * (4 + 2 * 4)     # entries and slots written, slots cleared
    bytes_out = 24 * len(r["xyz"]) + 8 * (len(r["xyz"]) + 1) + 20 * ro + 12 * n_new + (rc + rn) * 20 + 8 * rn
    moved = bytes_in + bytes_tables + bytes_out
    print(json.dumps({
        "tool": "merge_bench", "shots": a.shots, "pairs": len(pairs), "matches": len(m), "cloud_points": n_cloud,
        "cloud_records": rc, "new_elements": n_new, "out_points": len(r["xyz"]), "out_records": ro,
        "merged_static": st["merged_static"], "merged_dynamic": st["merged_dynamic"], "new_new_links": st["links"],
        "kernel_ms": round(kernel_ms, 4), "kernel_ms_min": round(float(np.min(ms)), 4),
        "kernel_ms_max": round(float(np.max(ms)), 4), "call_wall_ms": round(wall_ms, 3),
        "call_wall_ms_min": round(float(np.min(wall)), 3), "call_wall_ms_max": round(float(np.max(wall)), 3),
        "max_rounds": a.max_rounds, "rounds": path["rounds"], "host_fallback": path["host_fallback"],
        "host_bytes": path["host_bytes"],
        "elements_per_s_kernel": round(n_new / (kernel_ms * 1e-3), 1), "elements_per_s_wall": round(n_new / (wall_ms * 1e-3), 1),
        "bytes_moved": moved, "io_gbs": round(moved / (kernel_ms * 1e-3) / 1e9, 2),
        "hbm_frac": round(moved / (kernel_ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 5),
        "cloud_build": {"elements": k0, "wall_ms": round(setup_ms, 1), **setup_stats},
        "point_merge_distance": D, "feature_merge_distance": F, "steps": a.steps, "warmup": a.warmup}))


if __name__ == "__main__":
    main()
