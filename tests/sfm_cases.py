"""Synthetic scenes for the reconstruction loop, fixed seeds: shots on an arc around points
in a box, 720 x 405 images, f = 1.2 * 720, SimpleRadial.  Keypoints are the projections plus Gaussian noise, stored
as float; match lists come from shared point ids with a share of wrong partners; the homography ratios are given
per pair (they are the loop's input), so a scene does not depend on what the homography row makes of a synthetic
geometry.  No scene is larger than 6 shots x 400 points."""
import numpy as np

from sfmx.matching import DMATCH_DTYPE

W, H = 720, 405
F = 1.2 * W
K1, K2 = -0.05, 0.01


def camera(distorted=True):
    """(K 3x3, dist k1 k2 p1 p2 k3); distorted=False: the Simple model's camera, which has no distortion"""
    return (np.array([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1.0]]),
            np.array([K1, K2, 0, 0, 0.0]) if distorted else np.zeros(5))


def _project(P, X, distorted=True):
    x = X @ P[:, :3].T + P[:, 3]
    u, v = x[:, 0] / x[:, 2], x[:, 1] / x[:, 2]
    r2 = u * u + v * v
    d = 1 + K1 * r2 + K2 * r2 * r2 if distorted else 1.0
    return np.stack([F * u * d + W / 2, F * v * d + H / 2], 1), x[:, 2]


def scene(n_shots=5, n_points=300, noise=0.3, wrong=0.1, graph="complete", seed=11, all_wrong_shot=None, distorted=True):
    """-> dict(keypoints: list of n x 2 float32, point_id: list of int arrays (the point behind each keypoint),
    poses: n_shots x 3 x 4 ground truth, pairs, matches, offsets, homography: given ratios, shot_size)"""
    assert n_shots <= 6 and n_points <= 400, "test scenes stay small"
    return build(n_shots, n_points, noise, wrong, graph, seed, all_wrong_shot, distorted)


def build(n_shots, n_points, noise=0.3, wrong=0.1, graph="complete", seed=11, all_wrong_shot=None, distorted=True):
    """scene() without the size limit (tools/sfm_bench.py); graph: "complete", "chain2", ("seq", k) or a pair list."""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-1.0, -0.6, -1.0], [1.0, 0.6, 1.0], (n_points, 3))
    poses, kps, ids = [], [], []
    for s in range(n_shots):
        arc = max(48.0, 6.0 * (n_shots - 1))   # 48 degrees for the test scenes, 6 degrees a step beyond 9 shots
        a = np.deg2rad(-arc / 2 + arc * s / max(n_shots - 1, 1))
        c = np.array([5 * np.sin(a), 0.3 * np.cos(3 * a), -5 * np.cos(a)])   # on an arc, looking at the origin
        z = -c / np.linalg.norm(c)
        x = np.cross([0, 1.0, 0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        P = np.hstack([R, (-R @ c)[:, None]])
        uv, depth = _project(P, X, distorted)
        uv = uv + rng.normal(0, noise, uv.shape)
        seen = (depth > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H) & (rng.random(n_points) < 0.9)
        order = rng.permutation(np.flatnonzero(seen))
        poses.append(P)
        kps.append(uv[order].astype(np.float32))
        ids.append(order)
    if graph == "complete":
        pairs = [(i, j) for i in range(n_shots) for j in range(i + 1, n_shots)]
    elif graph == "chain2":   # sequence 2: every shot with its next two
        pairs = [(i, j) for i in range(n_shots) for j in (i + 1, i + 2) if j < n_shots]
    elif isinstance(graph, tuple) and graph[0] == "seq":
        pairs = [(i, j) for i in range(n_shots) for j in range(i + 1, min(i + 1 + graph[1], n_shots))]
    else:
        pairs = list(graph)
    lists = []
    for l, r in pairs:
        where_r = {int(p): k for k, p in enumerate(ids[r])}
        lst = []
        for q, p in enumerate(ids[l]):
            t = where_r.get(int(p))
            if t is None:
                continue
            bad = rng.random() < wrong or all_wrong_shot in (l, r)
            if bad:
                t = int(rng.integers(len(ids[r])))
            lst.append((q, t, 0, float(rng.uniform(10, 200))))
        lists.append(lst)
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    m = np.array([e for x in lists for e in x], DMATCH_DTYPE) if off[-1] else np.zeros(0, DMATCH_DTYPE)
    homography = 0.55 + 0.4 * rng.random(len(pairs))
    return dict(keypoints=kps, point_id=ids, poses=np.array(poses), pairs=np.array(pairs, np.int32).reshape(-1, 2),
                matches=m, offsets=off, homography=homography, shot_size=np.array([[W, H]] * n_shots, np.int32), points=X)
