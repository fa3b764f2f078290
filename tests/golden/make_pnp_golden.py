"""Writes tests/golden/pnp_small.npz: the outputs of tests/pnp_ref.py on tests/pnp_cases.small_case() for every
threshold of pnp_cases.THRESHOLDS (data only).  Run from the repository root:  python tests/golden/make_pnp_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "sfm-mvs-pipeline_amd")]

import pnp_cases  # noqa: E402
import pnp_ref    # noqa: E402


def main():
    case = pnp_cases.small_case()
    out = {"names": np.array(case["names"]), "thresholds": np.array(pnp_cases.THRESHOLDS)}
    for k, thr in enumerate(pnp_cases.THRESHOLDS):
        r = pnp_ref.register_poses(*pnp_cases.args(case), threshold=thr)
        for key in ("status", "pose", "ransac_pose", "mask", "n_inliers", "inlier_ratio", "refit_start"):
            out[f"t{k}_{key}"] = r[key]
        print(thr, dict(zip(case["names"], zip(r["status"].tolist(), r["n_inliers"].tolist()))))
    np.savez_compressed(os.path.join(HERE, "pnp_small.npz"), **out)


if __name__ == "__main__":
    main()
