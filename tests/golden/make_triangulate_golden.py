"""Writes tests/golden/triangulate_small.npz: the outputs of the numpy restatement (tests/tri_ref.py) on
tests/tri_cases.small_case, which tests/test_tri_ref.py pins the restatement to.
Run from the repository root after the library is built: python tests/golden/make_triangulate_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "sfm-mvs-pipeline_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import tri_cases  # noqa: E402
import tri_ref  # noqa: E402


def main():
    c = tri_cases.small_case()
    r = {t: tri_ref.triangulate_matches(*tri_cases.args(c), t) for t in (10.0, 0.5, 0.0)}
    out = {k: r[10.0][k] for k in ("point_offsets", "xyz", "match", "origin_shot", "origin_xy", "err")}
    for t, tag in ((0.5, "t05"), (0.0, "t0")):
        out[f"point_offsets_{tag}"] = r[t]["point_offsets"]
        out[f"match_{tag}"] = r[t]["match"]
    np.savez_compressed(os.path.join(HERE, "triangulate_small.npz"), **out)


if __name__ == "__main__":
    main()
