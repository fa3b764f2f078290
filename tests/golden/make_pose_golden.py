"""Writes tests/golden/pose_small.npz: the outputs of tests/pose_ref.py on the cases of tests/pose_cases.py
(every threshold of THRESHOLDS on small_case, noise_case with max_iters = 64).  Data only.
Run from the repository root: python tests/golden/make_pose_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "sfm-mvs-pipeline_amd")]

import pose_cases  # noqa: E402
import pose_ref  # noqa: E402

KEYS = ("status", "E", "pose", "mask", "n_ransac_inliers", "n_inliers", "matches", "pair_offsets")


def main():
    out = {}
    case = pose_cases.small_case()
    for i, thr in enumerate(pose_cases.THRESHOLDS):
        r = pose_ref.relative_poses(*pose_cases.args(case), threshold=thr)
        for k in KEYS:
            out[f"t{i}_{k}"] = r[k]
    r = pose_ref.relative_poses(*pose_cases.args(pose_cases.noise_case()), threshold=-1.0,
                                max_iters=pose_cases.NOISE_MAX_ITERS)
    for k in KEYS:
        out[f"noise_{k}"] = r[k]
    np.savez_compressed(os.path.join(HERE, "pose_small.npz"), **out)


if __name__ == "__main__":
    main()
