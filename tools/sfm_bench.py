#!/usr/bin/env python3
"""Timing of the reconstruction loop's rows (not run by any test).  One JSON line per case.

(a) --case count: the candidate ranking.  The BA bench scene's origin CSR (synth.ba_problem: 200 shots, 200 000
    points, 1.2 M records), keypoints = the observations as float, an unordered match graph (every pair i < j; a
    pair's list joins the keypoints of the points both shots see), half the shots as candidates.  Inputs are
    resident on the device.  Times sfmx_count_3d2d_matches and the loop of per-shot sfmx_find_3d2d_matches calls
    it replaces, alternating, median of --steps after --warmup: kernel time (HIP events) and wall time of both.
(b) --case loop: sfmx_sfm_triangulate end to end on a synthetic scene of --shots x --points (tests/sfm_cases.py
    geometry, every shot matched with its next --seq shots): wall ms per registered shot, split by row, and the
    bytes of host arrays each row is handed (the merge row's: every byte its calls copied between host and device),
    and the rounds, host fallback and bytes of the loop's last merge call.

    python tools/sfm_bench.py --case count [--steps 10] [--warmup 2]
    python tools/sfm_bench.py --case loop [--shots 50] [--points 2000] [--seq 5] [--steps 3] [--warmup 1]
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sfm-mvs-pipeline_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def count_scene(n_cams, n_points):
    """-> keypoints, pairs, matches, offsets, origin CSR of the BA bench scene."""
    from sfmx import synth
    from sfmx.matching import DMATCH_DTYPE
    p = synth.ba_problem(n_cams, n_points)
    op, oc = np.asarray(p["obs_point"], np.int64), np.asarray(p["obs_cam"], np.int64)
    xy = np.asarray(p["obs_xy"], np.float64).reshape(-1, 2).astype(np.float32)
    order = np.lexsort((np.arange(len(op)), op))           # point-major records
    op, oc, xy = op[order], oc[order], xy[order]
    oo = np.zeros(n_points + 1, np.int64)
    oo[1:] = np.cumsum(np.bincount(op, minlength=n_points))
    by_cam = np.lexsort((np.arange(len(oc)), oc))
    kp_of_rec = np.empty(len(oc), np.int64)                # keypoint index = rank of the record within its shot
    first = np.zeros(n_cams + 1, np.int64)
    first[1:] = np.cumsum(np.bincount(oc, minlength=n_cams))
    kp_of_rec[by_cam] = np.arange(len(oc)) - first[oc[by_cam]]
    kps = [xy[by_cam[first[c]:first[c + 1]]] for c in range(n_cams)]
    pairs = np.array(list(itertools.combinations(range(n_cams), 2)), np.int32)
    pid = np.full((n_cams, n_cams), -1, np.int64)
    pid[pairs[:, 0], pairs[:, 1]] = np.arange(len(pairs))
    k = int(oo[1] - oo[0])
    assert np.all(np.diff(oo) == k), "every point is seen by the same number of shots"
    cam, kpi = oc.reshape(-1, k), kp_of_rec.reshape(-1, k)
    P, Q, T = [], [], []
    for a, b in itertools.combinations(range(k), 2):
        swap = cam[:, a] > cam[:, b]
        l, r = np.where(swap, cam[:, b], cam[:, a]), np.where(swap, cam[:, a], cam[:, b])
        P.append(pid[l, r])
        Q.append(np.where(swap, kpi[:, b], kpi[:, a]))
        T.append(np.where(swap, kpi[:, a], kpi[:, b]))
    P, Q, T = np.concatenate(P), np.concatenate(Q), np.concatenate(T)
    srt = np.argsort(P, kind="stable")
    m = np.zeros(len(P), DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"], m["distance"] = Q[srt], T[srt], 1.0
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(P, minlength=len(pairs)))
    return kps, pairs, m, off, oo, oc.astype(np.int32), xy.astype(np.float64)


def case_count(a):
    import torch
    from sfmx import scene
    kps, pairs, m, off, oo, osh, oxy = count_scene(a.cams, a.cloud_points)
    cand = np.arange(0, a.cams, 2, dtype=np.int32)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dk = [d(k) for k in kps]
    kp_ptrs, nkp = [t.data_ptr() for t in dk], [len(k) for k in kps]
    dm, doff, doo, dsh, dxy = d(m.view(np.uint8)), d(off), d(oo), d(osh), d(oxy)
    n = len(osh)
    out = torch.zeros(len(cand), dtype=torch.int32, device="cuda")
    fk, fp = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rows = {"count": [], "find_loop": []}
    per_shot = None
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        scene.count_3d2d_matches_device(kp_ptrs, nkp, pairs, dm.data_ptr(), doff.data_ptr(), doo.data_ptr(), len(oo) - 1,
                                        dsh.data_ptr(), dxy.data_ptr(), cand, out.data_ptr())
        w = (time.perf_counter() - t0) * 1e3
        k_ms = scene.count_last_kernel_ms()
        counts = out.cpu().numpy().copy()
        t0 = time.perf_counter()
        lk, got = 0.0, []
        for s in cand:
            scene.find_3d2d_matches_device(kp_ptrs, nkp, pairs, dm.data_ptr(), doff.data_ptr(), doo.data_ptr(), len(oo) - 1,
                                           dsh.data_ptr(), dxy.data_ptr(), int(s), fk.data_ptr(), fp.data_ptr())
            lk += scene.last_kernel_ms()
            got.append(int((fk >= 0).sum().item()))     # the list size the reference sorts by
        lw = (time.perf_counter() - t0) * 1e3
        per_shot = np.array(got, np.int32)
        if i >= a.warmup:
            rows["count"].append((k_ms, w))
            rows["find_loop"].append((lk, lw))
    assert np.array_equal(counts, per_shot), "the batched counts differ from the per-shot calls"
    med = lambda v, j: round(float(np.median([x[j] for x in v])), 4)
    print(json.dumps({"tool": "sfm_bench", "case": "count", "shots": a.cams, "points": a.cloud_points, "records": n,
                      "pairs": len(pairs), "matches": len(m), "candidates": len(cand), "steps": a.steps, "warmup": a.warmup,
                      "count_kernel_ms": med(rows["count"], 0), "count_wall_ms": med(rows["count"], 1),
                      "find_loop_kernel_ms": med(rows["find_loop"], 0), "find_loop_wall_ms": med(rows["find_loop"], 1),
                      "count_sum": int(counts.sum()), "equal_to_per_shot_calls": True}))


def case_loop(a):
    import sfm_cases
    from sfmx import ba, scene, sfm
    sc = sfm_cases.build(a.shots, a.points, graph=("seq", a.seq), seed=31)
    scene.merge_set_max_rounds(a.max_rounds)
    runs = []
    for i in range(a.warmup + a.steps):
        ba.release_cache()
        t0 = time.perf_counter()
        r = sfm.triangulate(sc["keypoints"], sc["shot_size"], sfm_cases.camera(), ba.CAM_SIMPLE_RADIAL, sc["pairs"],
                            sc["matches"], sc["offsets"], sc["homography"])
        w = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            runs.append((w, r))
    path = scene.merge_last_path()   # the loop's last merge call: the one into the largest cloud
    w, r = sorted(runs, key=lambda x: x[0])[len(runs) // 2]
    reg = max(int(r["recovered"].sum()), 1)
    t = r["timing"]
    total_rows = sum(v["wall_ms"] for v in t.values())
    print(json.dumps({"tool": "sfm_bench", "case": "loop", "shots": a.shots, "points": a.points, "pairs": len(sc["pairs"]),
                      "matches": int(sc["offsets"][-1]), "steps": a.steps, "warmup": a.warmup,
                      "recovered": int(r["recovered"].sum()), "cloud_points": len(r["xyz"]), "records": len(r["origin_shot"]),
                      "ba_calls": r["summary"]["ba_calls"], "ba_iterations": r["summary"]["ba_iterations"],
                      "last_termination_type": r["summary"]["last_termination_type"],
                      "wall_ms": round(w, 2), "wall_ms_per_registered_shot": round(w / reg, 3),
                      "outside_rows_ms": round(w - total_rows, 2),
                      "merge_max_rounds": a.max_rounds, "merge_last_call": path,
                      "rows": {k: {"calls": v["calls"], "wall_ms": round(v["wall_ms"], 2), "device_ms": round(v["device_ms"], 2),
                                   "wall_ms_per_registered_shot": round(v["wall_ms"] / reg, 3),
                                   "share": round(v["wall_ms"] / w, 4), "handoff_bytes": v["handoff_bytes"]} for k, v in t.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["count", "loop"], required=True)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--cloud-points", type=int, default=200_000)
    ap.add_argument("--shots", type=int, default=50)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--seq", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=0,
                    help="loop case: cap on the merge's resolve rounds (0 the library default, < 0 the host resolution always)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sfm_bench: no GPU visible (there is no CPU path to time)")
    if a.steps is None:
        a.steps = 10 if a.case == "count" else 3
    if a.warmup is None:
        a.warmup = 2 if a.case == "count" else 1
    (case_count if a.case == "count" else case_loop)(a)


if __name__ == "__main__":
    main()
