"""Writes tests/golden/report_small.npz: a small scene (5 shots over 2 cameras, about 300 points with 0 to 7
origin records, empty CSR rows at the start, middle and end, one point with 300 records, five small images)
and what the numpy restatement (tests/report_ref.py) makes of it: the reprojection errors, their statistics and
histogram, the colours, and the bytes of the four files a reference run ends with.  tests/test_report_host.py
and tests/test_gpu_report.py pin the library to them.
Run from the repository root: python tests/golden/make_report_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import report_cases  # noqa: E402
import report_ref  # noqa: E402


def main():
    sc = report_cases.golden_scene()
    ims = report_cases.images(5)
    n = len(sc["xyz"])
    err = report_ref.reprojection_errors(*report_cases.args(sc))
    s = report_ref.error_statistics(err)
    k, c = report_ref.error_histogram(err)
    rgb, rec = report_ref.colorize(n, sc["origin_offsets"], sc["origin_shot"], sc["origin_xy"], ims)
    recovered = [True, True, False, True, True]
    cams, shots = report_cases.mvs_cameras(sc), report_cases.mvs_shots(sc, recovered)
    as_u8 = lambda b: np.frombuffer(b, np.uint8)
    np.savez_compressed(
        os.path.join(HERE, "report_small.npz"), xyz=sc["xyz"], origin_offsets=sc["origin_offsets"], origin_shot=sc["origin_shot"],
        origin_xy=sc["origin_xy"], cam_K=np.stack([K for K, _ in sc["cameras"]]), cam_dist=np.stack([d for _, d in sc["cameras"]]),
        cam_size=np.array([(w, h) for w, h, _ in cams], np.int32), shot_camera=sc["shot_camera"], shot_pose=sc["shot_pose"],
        recovered=np.array(recovered), **{"image%d" % i: np.ascontiguousarray(im) for i, im in enumerate(ims)},
        err=err, stats=np.array([s[f] for f in ("max", "min", "mean", "median", "variance", "deviation")]), hist_key=k,
        hist_count=c, rgb=rgb, record=rec, stats_csv=as_u8(report_ref.stats_csv(s)), hist_csv=as_u8(report_ref.hist_csv(k, c)),
        cloud_ply=as_u8(report_ref.pointcloud_ply(sc["xyz"], rgb)), cloud_plain_ply=as_u8(report_ref.pointcloud_ply(sc["xyz"])),
        cameras_ply=as_u8(report_ref.cameras_ply(cams, shots)))


if __name__ == "__main__":
    main()
