"""Writes tests/golden/cloud_small.npz: a small mesh (about 600 points with duplicates, 200 faces: one with
256 vertices, one with an index outside the cloud) and what the numpy restatement (tests/cloud_ref.py) makes
of it: distances, neighbours and the bytes of the three files of -Prun=pcl-stats.  tests/test_cloud_host.py
pins the library's host code to them.
Run from the repository root: python tests/golden/make_cloud_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cloud_ref  # noqa: E402


def mesh():
    rng = np.random.default_rng(2021)
    base = rng.normal(size=(520, 3)).astype(np.float32)
    base[:40] = np.round(base[:40] * 4) / 4                     # a few points on a coarse lattice: tied distances
    x = np.concatenate([base, base[100:160], base[100:120]])    # 60 points twice, 20 of them three times
    x = x[rng.permutation(len(x))]
    n = len(x)
    sizes = [3] * 150 + [4] * 40 + [5] * 8 + [256] + [3]
    idx = [int(v) for v in rng.integers(0, n, size=sum(sizes) - 3)] + [1, n, 2]   # the last face leaves the cloud
    return x, np.asarray(sizes, np.int32), np.asarray(idx, np.int32)


def main():
    x, fs, fi = mesh()
    d, nb = cloud_ref.neighbor_distances(x, 0)
    s = cloud_ref.statistics(d, len(x))
    k, c = cloud_ref.histogram(d, -1.0)
    as_u8 = lambda b: np.frombuffer(b, np.uint8)
    np.savez_compressed(os.path.join(HERE, "cloud_small.npz"), xyz=x, face_sizes=fs, face_indices=fi, distance=d,
                        neighbor=nb, stats=np.array([s[f] for f in ("max", "min", "mean", "median", "variance", "deviation")]),
                        hist_key=k, hist_count=c, stats_csv=as_u8(cloud_ref.stats_csv(s)),
                        neighbors_csv=as_u8(cloud_ref.neighbors_csv(k, c)),
                        quality_ply=as_u8(cloud_ref.quality_ply(x, d, fs, fi)))


if __name__ == "__main__":
    main()
