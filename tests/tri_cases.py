"""Shared fixed-seed case for the triangulation step (SfM::triangulateMatch, SfM.cpp:383-451).
Inputs only — the expected outputs come from tests/tri_ref.py.

Six shots on an arc around a landmark cloud at depth 4-9 (neighbouring baseline about 1), two cameras
(one distorted, one not), keypoints = projected landmarks + 0.7 px noise, every 8th match of an ordinary
pair replaced by a random keypoint.  Pair lists of 0, 1, 63, 64, 65, 257 and 1000 matches, 44 short pairs
(so the 256-match blocks of the kernel straddle many pair boundaries and the count scan covers several
blocks), and the edge pairs of `EDGE`.
"""
import numpy as np

from sfmx.matching import DMATCH_DTYPE
import tri_ref

N_SHOTS = 6
N_LAND = 1400
CAMERAS = [
    (np.array([800.0, 0, 320.0, 0, 790.0, 240.0, 0, 0, 1.0]), np.array([-0.12, 0.03, 0.001, -0.0007, 0.0])),
    (np.array([705.5, 0, 330.25, 0, 700.0, 250.5, 0, 0, 1.0]), np.zeros(5)),
]
SHOT_CAMERA = np.array([0, 1, 0, 1, 0, 1], np.int32)
MAIN_LENGTHS = (0, 1, 63, 64, 65, 257, 1000)
N_SHORT = 44
EDGE = ("all_fail", "all_pass", "same_pose")   # small_case()["edge"]: name -> index in the pair list


def arc_poses(n=N_SHOTS, radius=6.5):
    """3x4 [R|t] of n shots on a circle arc around (0, 0, radius), all looking at that point."""
    poses = np.zeros((n, 12))
    centre = np.array([0.0, 0.0, radius])
    for i in range(n):
        th = (i - (n - 1) / 2) / radius                  # arc length 1 between neighbours
        C = np.array([radius * np.sin(th), 0.05 * (i % 2), radius - radius * np.cos(th)])
        z = (centre - C) / np.linalg.norm(centre - C)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        poses[i] = np.concatenate([R, (-R @ C)[:, None]], axis=1).reshape(12)
    return poses


def landmarks(rng, n=N_LAND):
    return np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.2, 1.2, n), rng.uniform(4.0, 9.0, n)], axis=1).astype(np.float32)


def observe(land, poses, noise, rng):
    """Per shot: the landmarks' projections (+ noise) under a shot-specific permutation.
    -> keypoints [n x 2 float32], slot[s][j] = keypoint index of landmark j in shot s."""
    kps, slot = [], []
    for s in range(len(poses)):
        cam = tri_ref.cam_params(*CAMERAS[SHOT_CAMERA[s]])
        u, v = tri_ref.project(land[:, 0], land[:, 1], land[:, 2], poses[s], cam)
        pt = np.stack([u, v], axis=1).astype(np.float64) + noise * rng.standard_normal((len(land), 2))
        perm = rng.permutation(len(land))
        k = np.zeros((len(land), 2), np.float32)
        k[perm] = pt.astype(np.float32)
        kps.append(k)
        slot.append(perm)
    return kps, slot


def _pack(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    m = np.zeros(int(off[-1]), DMATCH_DTYPE)
    if len(m):
        qt = np.concatenate([np.asarray(x, np.int32).reshape(-1, 2) for x in lists])
        m["queryIdx"], m["trainIdx"] = qt[:, 0], qt[:, 1]
        m["distance"] = 1.0
    return m, off


def small_case(seed=20261019):
    """-> dict(kps, cameras, shot_camera, poses, pairs, matches, offsets, land, slot, edge, ordinary)."""
    rng = np.random.default_rng(seed)
    poses = arc_poses()
    land = landmarks(rng)
    kps, slot = observe(land, poses, 0.7, rng)
    # shot 2 also carries NaN keypoints (used by the same-pose pair only)
    nan_q = len(kps[2])
    kps[2] = np.concatenate([kps[2], np.array([[np.nan, np.nan], [np.nan, 100.0]], np.float32)])

    def ordinary_list(L, R, m, outliers=True):
        js = rng.choice(N_LAND, m, replace=False)
        q, t = slot[L][js], slot[R][js].copy()
        if outliers:
            t[7::8] = rng.integers(0, N_LAND, len(t[7::8]))
        return np.stack([q, t], axis=1)

    pairs, lists = [], []
    main_pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 2), (1, 3)]
    for (L, R), m in zip(main_pairs, MAIN_LENGTHS):
        pairs.append((L, R))
        lists.append(ordinary_list(L, R, m))
    ordered = [(a, b) for a in range(N_SHOTS) for b in range(N_SHOTS) if a != b]
    for i in range(N_SHORT):
        L, R = ordered[(7 * i + 3) % len(ordered)]
        m = 0 if i in (5, 6, 30) else int(rng.integers(1, 40))
        pairs.append((L, R))
        lists.append(ordinary_list(L, R, m))
    ordinary = list(range(len(pairs)))          # well-conditioned pairs (test_tri_ref's DLT comparison)
    edge = {}
    # every match fails: the right keypoint belongs to the landmark farthest away vertically in the right image
    js = rng.choice(N_LAND, 40, replace=False)
    yR = np.empty(N_LAND, np.float32)
    yR[:] = kps[4][slot[4], 1]
    far = np.array([int(np.argmax(np.abs(yR - yR[j]))) for j in js])
    edge["all_fail"] = len(pairs)
    pairs.append((2, 4))
    lists.append(np.stack([slot[2][js], slot[4][far]], axis=1))
    # every match passes: no outliers
    edge["all_pass"] = len(pairs)
    pairs.append((3, 5))
    lists.append(ordinary_list(3, 5, 50, outliers=False))
    # identical poses (a shot against itself): rank-deficient systems, NaN keypoints
    js = rng.choice(N_LAND, 32, replace=False)
    same = [(slot[2][j], slot[2][j]) for j in js[:16]] + [(slot[2][a], slot[2][b]) for a, b in zip(js[16:], js[:16])]
    same += [(nan_q, slot[2][js[0]]), (slot[2][js[1]], nan_q), (nan_q + 1, nan_q + 1), (nan_q, nan_q)]
    edge["same_pose"] = len(pairs)
    pairs.append((2, 2))
    lists.append(np.array(same))
    m, off = _pack(lists)
    return dict(kps=kps, cameras=CAMERAS, shot_camera=SHOT_CAMERA, poses=poses, pairs=np.array(pairs, np.int32),
                matches=m, offsets=off, land=land, slot=slot, edge=edge, ordinary=ordinary)


def exact_case(seed=5):
    """A rectified stereo pair (baseline 1 along x, no distortion) whose landmarks project to integer
    pixels in both views, so the float keypoints are noise-free: the landmark comes back."""
    rng = np.random.default_rng(seed)
    n, f = 300, 700.0
    cams = [(np.array([f, 0, 320.0, 0, f, 240.0, 0, 0, 1.0]), np.zeros(5))]
    poses = np.zeros((2, 12))
    poses[:, [0, 5, 10]] = 1.0
    poses[1, 3] = -1.0                                    # C = (1, 0, 0)
    d = rng.integers(78, 176, n)                          # integer disparity -> depth 4 .. 9
    u, v = rng.integers(100, 540, n), rng.integers(60, 420, n)
    Z = f / d
    land = np.stack([(u - 320.0) * Z / f, (v - 240.0) * Z / f, Z], axis=1)
    kps = [np.stack([u, v], axis=1).astype(np.float32), np.stack([u - d, v], axis=1).astype(np.float32)]
    m, off = _pack([np.stack([np.arange(n), np.arange(n)], axis=1)])
    return dict(kps=kps, cameras=cams, shot_camera=np.zeros(2, np.int32), poses=poses,
                pairs=np.array([[0, 1]], np.int32), matches=m, offsets=off, land=land)


def args(case):
    return (case["kps"], case["cameras"], case["shot_camera"], case["poses"], case["pairs"], case["matches"],
            case["offsets"])
