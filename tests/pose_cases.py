"""Shared fixed-seed cases for the relative-pose step (SfM::findCameraPoseFromMatch, SfM.cpp:491-540).
Inputs only — the expected outputs come from tests/pose_ref.py (tests/golden/pose_small.npz pins them).

The six shots and two cameras of tests/tri_cases.py; keypoints = landmarks in front of every view projected
with 0.5 px noise.  small_case(): pair lists of 0, 4, 5, 6, 63, 64, 65, 257 and LDS capacity + 1 matches (30 %
wrong partners from 63 on), a planar scene, a pure-rotation pair, one correspondence repeated, NaN keypoints.
noise_case(): one pair of random partners, run with max_iters = 64.  Odd shots are wider than every height, so
a positive threshold shows whether the right width is looked at.
"""
import numpy as np

from sfmx.matching import DMATCH_DTYPE
import tri_cases
import tri_ref

LDS_CAP = 1024                     # csrc/pose.hip CAP
MAIN_LENGTHS = (0, 4, 5, 6, 63, 64, 65, 257, LDS_CAP + 1)
THRESHOLDS = (-1.0, -0.25, 0.002)
NOISE = 0.5
N_LAND = 1400
SHOT_SIZE = np.array([(640, 480) if s % 2 == 0 else (900, 500) for s in range(tri_cases.N_SHOTS)], np.int32)
OUTLIER_PAIR = "len257"            # the 30 %-outlier pair of the chain test
SMALL = ("len0", "len4", "len5", "len6", "len63", "len64", "len65", "repeated")   # recomputed live on the GPU test


def _project(land, pose, cam_index, noise, rng):
    cam = tri_ref.cam_params(*tri_cases.CAMERAS[cam_index])
    u, v = tri_ref.project(land[:, 0], land[:, 1], land[:, 2], pose, cam)
    pt = np.stack([u, v], axis=1).astype(np.float64) + noise * rng.standard_normal((len(land), 2))
    return pt.astype(np.float32)


def small_case(seed=20261020):
    """-> dict(kps, cameras, shot_camera, shot_size, poses, pairs, matches, offsets, names, slot)."""
    rng = np.random.default_rng(seed)
    poses = tri_cases.arc_poses()
    land = tri_cases.landmarks(rng, N_LAND)
    kps, slot = tri_cases.observe(land, poses, NOISE, rng)
    cam_of = tri_cases.SHOT_CAMERA

    def append(s, pts):
        base = len(kps[s])
        kps[s] = np.concatenate([kps[s], np.asarray(pts, np.float32).reshape(-1, 2)])
        return np.arange(base, base + len(pts))

    def ordinary(L, R, m, outliers):
        js = rng.choice(N_LAND, m, replace=False)
        q, t = slot[L][js], slot[R][js].copy()
        if outliers and m:
            bad = rng.choice(m, int(round(0.3 * m)), replace=False)
            t[bad] = rng.integers(0, N_LAND, len(bad))
        return np.stack([q, t], axis=1).reshape(-1, 2)

    names, pairs, lists = [], [], []
    main_pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 2), (1, 3), (2, 5), (0, 3)]
    for (L, R), m in zip(main_pairs, MAIN_LENGTHS):
        names.append(f"len{m}")
        pairs.append((L, R))
        lists.append(ordinary(L, R, m, m >= 63))
    # a planar scene (every landmark on z = 6): the five-point solver has no planar degeneracy
    n = 80
    plane = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.2, 1.2, n), np.full(n, 6.0)], axis=1).astype(np.float32)
    q = append(0, _project(plane, poses[0], cam_of[0], NOISE, rng))
    t = append(3, _project(plane, poses[3], cam_of[3], NOISE, rng))
    names.append("planar"); pairs.append((0, 3)); lists.append(np.stack([q, t], axis=1))
    # pure rotation: the right keypoints are seen from shot 2's centre with shot 4's rotation (t = 0: E is degenerate)
    R2, t2, R4 = poses[2].reshape(3, 4)[:, :3], poses[2].reshape(3, 4)[:, 3], poses[4].reshape(3, 4)[:, :3]
    rot_pose = np.concatenate([R4, (R4 @ R2.T @ t2)[:, None]], axis=1).reshape(12)
    some = land[rng.choice(N_LAND, n, replace=False)]
    q = append(2, _project(some, poses[2], cam_of[2], NOISE, rng))
    t = append(4, _project(some, rot_pose, cam_of[4], NOISE, rng))
    names.append("rotation"); pairs.append((2, 4)); lists.append(np.stack([q, t], axis=1))
    # one correspondence, 20 times: every sample's system has rank 1
    j = int(rng.integers(0, N_LAND))
    names.append("repeated"); pairs.append((1, 4)); lists.append(np.tile([[slot[1][j], slot[4][j]]], (20, 1)))
    # NaN keypoints among 64 ordinary matches
    lst = ordinary(3, 5, 64, True)
    nq = append(3, [[np.nan, np.nan], [np.nan, 100.0]])
    nt = append(5, [[50.0, np.nan]])
    lst[5, 0], lst[17, 0], lst[40, 1] = nq[0], nq[1], nt[0]
    names.append("nan"); pairs.append((3, 5)); lists.append(lst)
    m, off = tri_cases._pack(lists)
    return dict(kps=kps, cameras=tri_cases.CAMERAS, shot_camera=cam_of, shot_size=SHOT_SIZE, poses=poses,
                pairs=np.array(pairs, np.int32), matches=m, offsets=off, names=names, slot=slot)


def noise_case(seed=7, n=200):
    """One pair whose partners are random: RANSAC runs its max_iters (64 in the tests) and keeps what it finds."""
    rng = np.random.default_rng(seed)
    c = small_case()
    lst = np.stack([rng.integers(0, N_LAND, n), rng.integers(0, N_LAND, n)], axis=1)
    m, off = tri_cases._pack([lst])
    return dict(c, pairs=np.array([[0, 5]], np.int32), matches=m, offsets=off, names=["noise"])


NOISE_MAX_ITERS = 64


def args(case):
    return (case["kps"], case["cameras"], case["shot_camera"], case["shot_size"], case["pairs"], case["matches"],
            case["offsets"])


def minimal_samples(n=200, seed=11):
    """n noise-free minimal samples of a two-view scene with a planted pose.
    -> (samples (n x 5 x 4: x1 y1 x2 y2, normalised), all points (m x 4), R, t unit, E unit Frobenius)."""
    rng = np.random.default_rng(seed)
    w = np.array([0.07, -0.21, 0.05])
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.9, 0.1, -0.25])
    t /= np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    E /= np.linalg.norm(E)
    X = np.stack([rng.uniform(-2, 2, 600), rng.uniform(-2, 2, 600), rng.uniform(4, 9, 600)], axis=1)
    Xc = X @ R.T + t
    P = np.concatenate([X[:, :2] / X[:, 2:], Xc[:, :2] / Xc[:, 2:]], axis=1)
    samples = np.stack([P[rng.choice(len(P), 5, replace=False)] for _ in range(n)])
    return samples, P, R, t, E
