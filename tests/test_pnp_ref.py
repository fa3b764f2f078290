"""CPU: the restatement tests/pnp_ref.py (the RANSAC stage of SfM::findCameraPoseFrom3d2dMatch, SfM.cpp:453-489)
against an independent computation (numpy.linalg eigh / inv / lstsq / svd), on planted scenes, on exact known
answers, and against the pinned golden file.  DESIGN.md §8i has the measured / tolerance table."""
import os

import numpy as np
import pytest

import pnp_cases
import pnp_ref
import tri_ref

HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64 = np.float32, np.float64
KEYS = ("status", "ransac_pose", "mask", "n_inliers", "inlier_ratio")

# 10 x the largest difference measured on the CPU: restatement vs the LAPACK route, 200 samples
POSE_TOL = 3.8e-12        # measured 3.68e-13 between the two routes, 3.74e-13 against the planted pose
REP_TOL = 4.0e-13         # measured 3.93e-14
# 10 x the restatement's own largest error of the refit's pose on the noise-free 65-point scenes (float pixels):
# measured 5.35e-8 (the EPnP model before the refit: 2.02e-7)
SCENE_TOL = 5.4e-7


def lapack_epnp5(pw, uv):
    """EPnP on five points by LAPACK routines; shares no code with pnp_ref."""
    pw, uv = np.asarray(pw, F64), np.asarray(uv, F64)
    c0 = pw.mean(axis=0)
    d = pw - c0
    lam, vec = np.linalg.eigh(d.T @ d)
    cws = np.vstack([c0] + [c0 + np.sqrt(lam[i] / 5.0) * vec[:, i] for i in (2, 1, 0)])
    al3 = d @ np.linalg.inv((cws[1:] - c0).T).T
    al = np.hstack([1.0 - al3.sum(axis=1, keepdims=True), al3])
    M = np.zeros((10, 12))
    for i in range(5):
        for k in range(4):
            M[2 * i, 3 * k], M[2 * i, 3 * k + 2] = al[i, k], -al[i, k] * uv[i, 0]
            M[2 * i + 1, 3 * k + 1], M[2 * i + 1, 3 * k + 2] = al[i, k], -al[i, k] * uv[i, 1]
    _, ev = np.linalg.eigh(M.T @ M)
    v = ev[:, :4].T.reshape(4, 4, 3)                      # v[i][control point]
    prs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    terms = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]
    L = np.array([[(1.0 if i == j else 2.0) * np.dot(v[i, a] - v[i, b], v[j, a] - v[j, b]) for i, j in terms] for a, b in prs])
    rho = np.array([np.sum((cws[a] - cws[b]) ** 2) for a, b in prs])

    def quad(b):
        return np.array([b[i] * b[j] for i, j in terms])

    def start(which):
        cols = ((0, 1, 3, 6), (0, 1, 2), (0, 1, 2, 3, 4))[which]
        x = np.linalg.lstsq(L[:, cols], rho, rcond=None)[0]
        if which == 0:
            b0 = np.sqrt(abs(x[0]))
            return np.array([b0, *(np.sign(x[0]) * x[1:] / b0)]) if x[0] != 0 else None
        b0 = np.sqrt(abs(x[0]))
        b1 = np.sqrt(abs(x[2])) if x[2] * x[0] > 0 else 0.0
        if x[1] < 0:
            b0 = -b0
        return np.array([b0, b1, x[3] / b0 if which == 2 else 0.0, 0.0])

    best = None
    for which in range(3):
        b = start(which)
        for _ in range(5):
            dq = np.zeros((10, 4))                        # d (b_i b_j) / d b_k
            for k, (i, j) in enumerate(terms):
                dq[k, i] += b[j]
                dq[k, j] += b[i]
            b = b + np.linalg.lstsq(L @ dq, rho - L @ quad(b), rcond=None)[0]
        ccs = np.einsum("i,ijk->jk", b, v)
        pcs = al @ ccs
        if pcs[0, 2] < 0:
            pcs = -pcs
        pc0 = pcs.mean(axis=0)
        U, _, Vt = np.linalg.svd((pcs - pc0).T @ d)
        R = U @ Vt
        if np.linalg.det(R) < 0:
            R[2] = -R[2]
        t = pc0 - R @ c0
        Xc = pw @ R.T + t
        e = np.mean(np.linalg.norm(uv - Xc[:, :2] / Xc[:, 2:], axis=1))
        if best is None or e < best[1]:
            best = (np.hstack([R, t[:, None]]).reshape(12), e)
    return best


def test_epnp_against_lapack_on_200_noise_free_samples():
    X, uv, R, t = pnp_cases.minimal_samples(200, seed=11)
    planted = np.hstack([R, t[:, None]]).reshape(12)
    worst_pose = worst_rep = worst_planted = 0.0
    for i in range(200):
        got = pnp_ref.epnp5(X[i], uv[i], detail=True)
        assert got is not None, i
        pose, _, rep = got
        lp, le = lapack_epnp5(X[i], uv[i])
        worst_pose = max(worst_pose, float(np.abs(np.array(pose) - lp).max()))
        worst_rep = max(worst_rep, abs(rep - le))
        worst_planted = max(worst_planted, float(np.abs(np.array(pose) - planted).max()))
    print("restatement vs LAPACK: pose", worst_pose, "rep_error", worst_rep, "| vs planted", worst_planted)
    assert worst_pose < POSE_TOL and worst_rep < REP_TOL and worst_planted < POSE_TOL


@pytest.mark.parametrize("seed", range(4))
def test_full_chain_on_planted_scenes(seed):
    X, px, cam, R, t = pnp_cases.planted_scene(seed, n=65)
    r = pnp_ref.register_set(X, px, tri_ref.cam_params(*cam), (640, 480), -8.0)
    assert r["status"] == 1 and r["n_inliers"] == 65 and r["mask"].all()            # all inliers found
    assert r["inlier_ratio"] == 64 / 65
    planted = np.hstack([R, t[:, None]]).reshape(12)
    err = float(np.abs(r["pose"] - planted).max())                                    # the refit's pose
    print("planted scene", seed, "refit pose error", err, "EPnP model", float(np.abs(r["ransac_pose"] - planted).max()),
          "subsets", len(r["drawn"]))
    assert err < SCENE_TOL and r["refit_start"] == 0
    Xn, pxn, _, _, _ = pnp_cases.planted_scene(seed, n=65, noise=0.5)
    rn = pnp_ref.register_set(Xn, pxn, tri_ref.cam_params(*cam), (640, 480), -8.0)
    assert rn["status"] == 1 and rn["n_inliers"] == 65


def test_exact_known_answers():
    X, px, cam, _, _ = pnp_cases.planted_scene(7, n=40)
    cam = tri_ref.cam_params(*cam)
    for n in (0, 3):
        r = pnp_ref.register_set(X[:n], px[:n], cam, (640, 480))
        assert r["status"] == 0 and r["inlier_ratio"] == -1.0 and np.isnan(r["ransac_pose"]).all() and len(r["mask"]) == n
    r = pnp_ref.register_set(X[:4], px[:4], cam, (640, 480))
    assert r["status"] == 2 and r["inlier_ratio"] == -1.0 and not r["mask"].any()
    r = pnp_ref.register_set(X[:5], px[:5], cam, (640, 480))
    assert r["status"] == 1 and r["drawn"] == [] and r["mask"].all() and r["inlier_ratio"] == 4 / 5
    assert r["refit_start"] == -1 and r["pose"].tobytes() == r["ransac_pose"].tobytes()          # no refit
    # the index-0 quirk
    r = pnp_ref.register_set(X, px, cam, (640, 480))
    assert r["mask"][0] and r["n_inliers"] == 40 and r["inlier_ratio"] == 39 / 40
    px2 = px.copy()
    px2[0] += 300.0
    r2 = pnp_ref.register_set(X, px2, cam, (640, 480))
    assert not r2["mask"][0] and r2["n_inliers"] == 39 and r2["inlier_ratio"] == 39 / 40
    # the 3-D points are rounded to float first: a change below the float's resolution changes nothing, a
    # coordinate that is no float gives another result than its double would
    r3 = pnp_ref.register_set(X * (1.0 + 1e-12), px2, cam, (640, 480))
    assert r3["ransac_pose"].tobytes() == r2["ransac_pose"].tobytes()
    Xd = X[:5] * (1.0 + 3e-8)
    assert (Xd.astype(F32).astype(F64) != Xd).any()
    uvn = np.stack(tri_ref.undistort(px[:5].astype(F32), cam), axis=1).astype(F64)
    assert pnp_ref.epnp5(Xd, uvn) != pnp_ref.epnp5(Xd.astype(F32).astype(F64), uvn)
    assert pnp_ref.register_set(Xd, px[:5], cam, (640, 480))["ransac_pose"].tolist() == pnp_ref.epnp5(Xd.astype(F32).astype(F64), uvn)


def test_planar_scenes_are_posed():
    """A coplanar sample has three control points (EPnP's case N = 1); exactly planar, tilted, with and without
    noise.  Tolerance: 10 x the restatement's largest error on the noise-free planes (measured 8.36e-7)."""
    worst = 0.0
    for seed in range(3):
        for tilt in (0.0, 0.3):
            X, _, cam, R, t = pnp_cases.planted_scene(seed, n=65)
            X[:, 2] = tilt * X[:, 0] - 0.2 * tilt * X[:, 1] + 0.5
            X = X.astype(F32).astype(F64)
            Xc = X @ R.T + t
            px = np.stack([Xc[:, 0] / Xc[:, 2] * 1200.0 + 320.0, Xc[:, 1] / Xc[:, 2] * 1200.0 + 240.0], axis=1)
            r = pnp_ref.register_set(X, px, tri_ref.cam_params(*cam), (640, 480), -8.0)
            assert r["status"] == 1 and r["n_inliers"] == 65, (seed, tilt)
            worst = max(worst, float(np.abs(r["ransac_pose"] - np.hstack([R, t[:, None]]).reshape(12)).max()))
            rn = pnp_ref.register_set(X, px + 0.5 * np.random.default_rng(seed).standard_normal(px.shape),
                                      tri_ref.cam_params(*cam), (640, 480), -8.0)
            assert rn["status"] == 1 and rn["n_inliers"] == 65, (seed, tilt)
    print("planar scenes: worst pose error", worst)
    assert worst < 8.4e-6


def test_refit_pieces():
    """Rodrigues against its finite differences and its inverse; a non-planar set of 5 inliers fails the DLT; a
    planar set starts from the EPnP model."""
    r = [0.1, -0.2, 0.05]
    R, dR = pnp_ref.rodrigues(r)
    for i in range(3):
        hi, lo = list(r), list(r)
        hi[i] += 1e-6
        lo[i] -= 1e-6
        fd = (np.array(pnp_ref.rodrigues(hi)[0]) - np.array(pnp_ref.rodrigues(lo)[0])) / 2e-6
        assert np.abs(fd - np.array(dR[i])).max() < 1e-9
    assert np.abs(np.array(pnp_ref.rodrigues_inv(R)) - r).max() < 1e-15
    assert pnp_ref.rodrigues([0.0, 0.0, 0.0])[0] == list(pnp_ref.EYE9)
    X, px, cam, _, _ = pnp_cases.planted_scene(2, n=12)
    cam = tri_ref.cam_params(*cam)
    pxb = px.copy()
    pxb[5:] += 400.0                                                                   # five inliers, seven far off
    rb = pnp_ref.register_set(X, pxb, cam, (640, 480))
    assert rb["status"] == 0 and rb["inlier_ratio"] == -1.0 and not rb["mask"].any() and rb["refit_start"] == -1
    Xp = X.copy()
    Xp[:, 2] = 0.5
    Rp, tp = pnp_cases.planted_pose()
    Xc = Xp @ Rp.T + tp
    pp = np.stack([Xc[:, 0] / Xc[:, 2] * 1200.0 + 320.0, Xc[:, 1] / Xc[:, 2] * 1200.0 + 240.0], axis=1)
    rp = pnp_ref.register_set(Xp, pp, cam, (640, 480))
    assert rp["status"] == 1 and rp["refit_start"] == 1 and rp["n_inliers"] == 12
    assert pnp_ref.tree_sum(np.arange(600.0).reshape(-1, 1))[0] == 600 * 599 / 2


def test_both_threshold_forms():
    assert pnp_ref.pixel_threshold(-8.0, (640, 480)) == F32(64.0)
    assert pnp_ref.pixel_threshold(-0.1, (640, 480)) == F32(float(F32(0.1)) ** 2)          # through the float parameter
    assert pnp_ref.pixel_threshold(0.004, (900, 500)) == F32(float(F32(900 * 0.004)) ** 2)
    assert pnp_ref.pixel_threshold(0.004, (500, 900)) == pnp_ref.pixel_threshold(0.004, (900, 500))
    # the same list under a loose and a tight positive threshold
    X, px, cam, _, _ = pnp_cases.planted_scene(3, n=30, noise=1.0)
    cam = tri_ref.cam_params(*cam)
    loose = pnp_ref.register_set(X, px, cam, (640, 480), 0.0125)       # 8 px
    tight = pnp_ref.register_set(X, px, cam, (640, 480), 0.0005)       # 0.32 px
    assert loose["n_inliers"] == 30 and tight["n_inliers"] < 30


def test_distinct_points():
    xyz = np.array([[1.0, 2, 3], [1.0, 2, 3], [-0.0, 0, 1], [0.0, 0, 1], [np.nan, 0, 1], [np.nan, 0, 1], [7.0, 8, 9]])
    oo = np.array([0, 2, 3, 4, 5, 6, 7, 8], np.int64)
    fk = np.array([4, 4, 9, 1, 1, 2, 2, -1], np.int32)
    fxy = np.array([[5, 6], [5, 6], [5, 6], [0, -0.0], [-0.0, 0], [1, 1], [1, 1], [np.nan, np.nan]], F32)
    p3, p2 = pnp_ref.distinct_3d2d(xyz, oo, fk, fxy)
    # one point for records 0-2 (equal coordinates at point indices 0 and 1), one for -0 / +0, both NaN records
    assert p3.shape == (4, 3) and p2.shape == (4, 2)
    assert p3[0].tolist() == [1, 2, 3] and p2[0].tolist() == [5, 6]
    assert p3[1].tolist() == [0, 0, 1] and np.signbit(p3[1, 0]) and p2[1].tolist() == [0, 0]     # the first appearance is kept
    assert np.isnan(p3[2:, 0]).all() and p2[2:].tolist() == [[1, 1], [1, 1]]
    # a different image point keeps the record
    fxy[1] = (5, 6.5)
    assert len(pnp_ref.distinct_3d2d(xyz, oo, fk, fxy)[0]) == 5
    e3, e2 = pnp_ref.distinct_3d2d(np.zeros((0, 3)), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), F32))
    assert e3.shape == (0, 3) and e2.shape == (0, 2)


def test_golden_file_pins_the_restatement_on_the_small_sets():
    g = np.load(os.path.join(HERE, "golden", "pnp_small.npz"))
    case = pnp_cases.small_case()
    assert g["names"].tolist() == case["names"] and g["thresholds"].tolist() == list(pnp_cases.THRESHOLDS)
    sub = pnp_cases.subset(case, pnp_cases.SMALL + ("nan",))
    for ti, thr in enumerate(pnp_cases.THRESHOLDS):
        r = pnp_ref.register_poses(*pnp_cases.args(sub), threshold=thr)
        for j, name in enumerate(sub["names"]):
            s = case["names"].index(name)
            for k in ("status", "pose", "ransac_pose", "n_inliers", "inlier_ratio", "refit_start"):
                assert r[k][j].tobytes() == g[f"t{ti}_{k}"][s].tobytes(), (thr, name, k)
            a, b = case["offsets"][s], case["offsets"][s + 1]
            assert r["mask"][sub["offsets"][j]:sub["offsets"][j + 1]].tobytes() == g[f"t{ti}_mask"][a:b].tobytes()
