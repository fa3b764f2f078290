"""Shared fixed-seed cases for the registration pose (the RANSAC stage of SfM::findCameraPoseFrom3d2dMatch,
SfM.cpp:453-489).  Inputs only — the expected outputs come from tests/pnp_ref.py (tests/golden/pnp_small.npz
pins them).

The six shots and two cameras of tests/tri_cases.py (one camera with distortion, one without); a set is a list
of (3-D landmark, 2-D observation in the set's shot) with 0.5 px noise.  small_case(): sets of 0, 3, 4, 5, 6, 7,
63, 64, 65, 257 and 1025 points (30 % wrong partners from 63 on), a planar scene, a set of pure noise, one point
repeated 20 times and a set with NaN points.  Odd shots are 900 x 500, even ones 640 x 480, so a positive
threshold differs between them.
"""
import numpy as np

import tri_cases
import tri_ref

MAIN_LENGTHS = (0, 3, 4, 5, 6, 7, 63, 64, 65, 257, 1025)
THRESHOLDS = (-8.0, -1.0, 0.004)
NOISE = 0.5
N_LAND = 1400
SHOT_SIZE = np.array([(640, 480) if s % 2 == 0 else (900, 500) for s in range(tri_cases.N_SHOTS)], np.int32)
SMALL = ("len0", "len3", "len4", "len5", "len6", "len7", "len63", "len64", "len65", "repeated")   # recomputed live


def observe(land, pose, cam_index, noise, rng):
    """The landmarks' projections under the pose, + noise, as doubles (Point2d)."""
    cam = tri_ref.cam_params(*tri_cases.CAMERAS[cam_index])
    land = np.asarray(land, np.float32)
    u, v = tri_ref.project(land[:, 0], land[:, 1], land[:, 2], pose, cam)
    return np.stack([u, v], axis=1).astype(np.float64) + noise * rng.standard_normal((len(land), 2))


def small_case(seed=20261021):
    """-> dict(p3, p2, offsets, set_shot, names, cameras, shot_camera, shot_size, poses)."""
    rng = np.random.default_rng(seed)
    poses = tri_cases.arc_poses()
    land = tri_cases.landmarks(rng, N_LAND).astype(np.float64)
    land += 1e-9 * rng.standard_normal(land.shape)       # Point3d coordinates that are no floats
    cam_of = tri_cases.SHOT_CAMERA
    names, shots, p3s, p2s = [], [], [], []

    def add(name, shot, X, x):
        names.append(name); shots.append(shot)
        p3s.append(np.asarray(X, np.float64).reshape(-1, 3)); p2s.append(np.asarray(x, np.float64).reshape(-1, 2))

    def ordinary(shot, m, outliers):
        js = rng.choice(N_LAND, m, replace=False)
        X = land[js]
        x = observe(X, poses[shot], cam_of[shot], NOISE, rng)
        if outliers and m:
            bad = rng.choice(m, int(round(0.3 * m)), replace=False)
            x[bad] = observe(land[rng.integers(0, N_LAND, len(bad))], poses[shot], cam_of[shot], NOISE, rng)
        return X, x

    for i, m in enumerate(MAIN_LENGTHS):
        shot = i % tri_cases.N_SHOTS
        add(f"len{m}", shot, *ordinary(shot, m, m >= 63))
    # a planar scene: every landmark on z = 6
    n = 80
    plane = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.2, 1.2, n), np.full(n, 6.0)], axis=1)
    add("planar", 3, plane, observe(plane, poses[3], cam_of[3], NOISE, rng))
    # pure noise: landmarks against random pixels
    n = 120
    add("noise", 2, land[rng.choice(N_LAND, n, replace=False)],
        np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], axis=1))
    # one point, 20 times
    X, x = ordinary(4, 1, False)
    add("repeated", 4, np.tile(X, (20, 1)), np.tile(x, (20, 1)))
    # NaN points among 64 ordinary ones (point 0 among them)
    X, x = ordinary(5, 64, True)
    X[0, 1] = np.nan
    X[17] = np.nan
    x[40, 0] = np.nan
    add("nan", 5, X, x)
    off = np.zeros(len(names) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in p3s])
    return dict(p3=np.concatenate(p3s), p2=np.concatenate(p2s), offsets=off, set_shot=np.array(shots, np.int32),
                names=names, cameras=tri_cases.CAMERAS, shot_camera=cam_of, shot_size=SHOT_SIZE, poses=poses)


def args(case):
    return (case["p3"], case["p2"], case["offsets"], case["set_shot"], case["cameras"], case["shot_camera"],
            case["shot_size"])


def subset(case, names):
    """The case reduced to the named sets, in the given order."""
    idx = [case["names"].index(n) for n in names]
    o = case["offsets"]
    p3 = [case["p3"][o[i]:o[i + 1]] for i in idx]
    p2 = [case["p2"][o[i]:o[i + 1]] for i in idx]
    off = np.zeros(len(idx) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in p3])
    return dict(case, p3=np.concatenate(p3) if idx else np.zeros((0, 3)), p2=np.concatenate(p2) if idx else np.zeros((0, 2)),
                offsets=off, set_shot=case["set_shot"][idx], names=list(names))


def planted_pose():
    w = np.array([0.1, -0.2, 0.05])
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    return R, np.array([0.3, -0.2, 6.0])


def planted_scene(seed, n=65, noise=0.0, f=1200.0):
    """n float-representable points in a 4-unit cube at depth about 6, seen by a distortion-free camera of
    focal length f under planted_pose().  -> (p3 (n x 3), p2 (n x 2) pixels, camera (K, dist), R, t)."""
    rng = np.random.default_rng(seed)
    R, t = planted_pose()
    X = rng.uniform(-2, 2, (n, 3)).astype(np.float32).astype(np.float64)
    Xc = X @ R.T + t
    px = np.stack([Xc[:, 0] / Xc[:, 2] * f + 320.0, Xc[:, 1] / Xc[:, 2] * f + 240.0], axis=1)
    px = px + noise * rng.standard_normal(px.shape)
    return X, px, (np.array([f, 0, 320.0, 0, f, 240.0, 0, 0, 1.0]), np.zeros(5)), R, t


def minimal_samples(n=200, seed=11):
    """n noise-free five-point samples of planted_pose(): (n x 5 x 3 float-representable points, n x 5 x 2
    normalised image points), R, t."""
    rng = np.random.default_rng(seed)
    R, t = planted_pose()
    X = rng.uniform(-2, 2, (n, 5, 3)).astype(np.float32).astype(np.float64)
    Xc = X @ R.T + t
    return X, Xc[..., :2] / Xc[..., 2:], R, t
