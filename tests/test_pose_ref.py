"""CPU: pins tests/pose_ref.py, the restatement of SfM::findCameraPoseFromMatch.

The five-point solver is compared with an independent computation that shares nothing with it: numpy.linalg.svd
for the null space, dictionary polynomials for the constraints, the eigenvalues of the 10 x 10 action matrix
(Stewenius, Engels, Nister 2006) for the roots.  Each tolerance is ten times the maximum measured on this suite's
CPU run (the independent side is LAPACK, whose rounding differs between builds); measured values next to them.
"""
import os

import numpy as np
import pytest

import pose_cases
import pose_ref

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_MATCH = 6.6e-5      # measured 6.54e-06: restated solution vs the nearest independent one (max abs entry)
TOL_EPIPOLAR = 1.6e-15  # measured 1.53e-16: |x2^T E x1| on the sample
TOL_CUBIC = 2.2e-5      # measured 2.11e-06: max |2 E E^T E - tr(E E^T) E|
TOL_DET = 1.1e-5        # measured 1.08e-06: |det E|
TOL_PLANTED = 2.8e-7    # measured 2.73e-08: the planted E vs the nearest solution
TOL_POSE = 4.0e-7       # measured 3.94e-08: R, t / |t| of recoverPose on the solution nearest the planted E (max abs entry)


# ---------------------------------------------------------------------------- the independent solver

def _pmul(a, b):
    o = {}
    for ka, va in a.items():
        for kb, vb in b.items():
            k = (ka[0] + kb[0], ka[1] + kb[1], ka[2] + kb[2])
            o[k] = o.get(k, 0.0) + va * vb
    return o


def _padd(a, b, s=1.0):
    o = dict(a)
    for k, v in b.items():
        o[k] = o.get(k, 0.0) + s * v
    return o


GREVLEX = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
           (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def independent_five_point(q):
    x1 = np.c_[q[:, :2], np.ones(5)]
    x2 = np.c_[q[:, 2:], np.ones(5)]
    Q = np.stack([np.outer(x2[i], x1[i]).ravel() for i in range(5)])
    N = np.linalg.svd(Q)[2][5:]
    Ep = [[{(1, 0, 0): N[0][3 * i + j], (0, 1, 0): N[1][3 * i + j], (0, 0, 1): N[2][3 * i + j], (0, 0, 0): N[3][3 * i + j]}
           for j in range(3)] for i in range(3)]

    def mm(A, B):
        out = [[{} for _ in range(3)] for _ in range(3)]
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    out[i][j] = _padd(out[i][j], _pmul(A[i][k], B[k][j]))
        return out

    Et = [[Ep[j][i] for j in range(3)] for i in range(3)]
    EEt = mm(Ep, Et)
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    EEtE = mm(EEt, Ep)
    rows = [_padd({k: 2 * v for k, v in EEtE[i][j].items()}, _pmul(tr, Ep[i][j]), -1.0) for i in range(3) for j in range(3)]

    def minor(a, b, c, d):
        return _padd(_pmul(Ep[a[0]][a[1]], Ep[b[0]][b[1]]), _pmul(Ep[c[0]][c[1]], Ep[d[0]][d[1]]), -1.0)

    det = _padd(_padd(_pmul(Ep[0][0], minor((1, 1), (2, 2), (1, 2), (2, 1))),
                      _pmul(Ep[0][1], minor((1, 0), (2, 2), (1, 2), (2, 0))), -1.0),
                _pmul(Ep[0][2], minor((1, 0), (2, 1), (1, 1), (2, 0))))
    rows.append(det)
    A = np.array([[r.get(m, 0.0) for m in GREVLEX] for r in rows])
    M = np.linalg.solve(A[:, :10], A[:, 10:])
    At = np.zeros((10, 10))             # multiplication by x on the basis x2 xy xz y2 yz z2 x y z 1
    At[:6] = -M[:6]
    At[6, 0] = At[7, 1] = At[8, 2] = At[9, 6] = 1.0
    w, V = np.linalg.eig(At)
    out = []
    for k in range(10):
        if w[k].imag != 0:
            continue
        v = V[:, k].real
        x, y, z = v[6] / v[9], v[7] / v[9], v[8] / v[9]
        E = (x * N[0] + y * N[1] + z * N[2] + N[3]).reshape(3, 3)
        out.append(E / np.linalg.norm(E))
    return out


def _sign_dist(E, F):
    return min(np.abs(E - F).max(), np.abs(E + F).max())


@pytest.fixture(scope="module")
def minimal():
    samples, P, R, t, E0 = pose_cases.minimal_samples(200, seed=11)
    mine = [[np.array(E).reshape(3, 3) for E in pose_ref.five_point(q)] for q in samples]
    return samples, P, R, t, E0, mine


def test_same_number_of_real_solutions_on_every_sample(minimal):
    samples, _, _, _, _, mine = minimal
    assert len(samples) == 200
    worst = 0.0
    for q, sols in zip(samples, mine):
        ind = independent_five_point(q)
        assert len(sols) == len(ind) and 1 <= len(sols) <= 10
        for E in sols:
            worst = max(worst, min(_sign_dist(E, F) for F in ind))
    print("match", worst)
    assert worst <= TOL_MATCH


def test_solutions_satisfy_the_constraints(minimal):
    samples, _, _, _, _, mine = minimal
    epi = cubic = det = 0.0
    for q, sols in zip(samples, mine):
        x1 = np.c_[q[:, :2], np.ones(5)]
        x2 = np.c_[q[:, 2:], np.ones(5)]
        for E in sols:
            assert abs(np.linalg.norm(E) - 1.0) < 1e-15 * 8
            epi = max(epi, np.abs(np.einsum("ni,ij,nj->n", x2, E, x1)).max())
            cubic = max(cubic, np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max())
            det = max(det, abs(np.linalg.det(E)))
    print("epipolar", epi, "cubic", cubic, "det", det)
    assert epi <= TOL_EPIPOLAR and cubic <= TOL_CUBIC and det <= TOL_DET


def test_planted_pose_comes_back(minimal):
    samples, P, R, t, E0, mine = minimal
    worst = max(min(_sign_dist(E, E0) for E in sols) for sols in mine)
    print("planted", worst)
    assert worst <= TOL_PLANTED
    worst_pose = 0.0
    for sols in mine:
        E = min(sols, key=lambda E: _sign_dist(E, E0))
        cands = pose_ref.candidates(list(E.reshape(9)))
        good = [int(np.count_nonzero(pose_ref.cheirality(c, P[:, 0], P[:, 1], P[:, 2], P[:, 3]))) for c in cands]
        w = pose_ref.choose(good)
        assert good[w] == len(P) and sorted(good)[:3] == [0, 0, 0]       # every cheirality bit, only the winner's
        Pw = np.array(cands[w]).reshape(3, 4)
        worst_pose = max(worst_pose, np.abs(Pw[:, :3] - R).max(), np.abs(Pw[:, 3] - t).max())
    print("pose", worst_pose)
    assert worst_pose <= TOL_POSE


# ---------------------------------------------------------------------------- exact known answers

def _pair(case, name, thr=-1.0, **kw):
    p = case["names"].index(name)
    L, R = case["pairs"][p]
    a, b = case["offsets"][p], case["offsets"][p + 1]
    m = case["matches"][a:b]
    cams = [pose_ref.cam_params(K, d) for K, d in case["cameras"]]
    return pose_ref.pose_pair(case["kps"][L][m["queryIdx"]], case["kps"][R][m["trainIdx"]], cams[case["shot_camera"][L]],
                              cams[case["shot_camera"][R]], thr, **kw)


@pytest.fixture(scope="module")
def case():
    return pose_cases.small_case()


def test_fewer_than_five_matches_and_no_model_have_status_0(case):
    for name in ("len4", "repeated"):
        r = _pair(case, name)
        assert r["status"] == 0 and not r["mask"].any() and r["n_ransac"] == 0 and r["n_inliers"] == 0
        assert np.isnan(r["E"]).all() and np.isnan(r["pose"]).all()
    assert pose_ref.five_point(np.tile([[0.1, 0.2, 0.3, 0.4]], (5, 1))) == []


def test_five_matches_draw_nothing(case):
    r = _pair(case, "len5")
    assert r["status"] == 1 and r["drawn"] == [] and r["n_ransac"] == 5


def _independent_subsets(n, k):
    state, out = (1 << 64) - 1, []
    for _ in range(k):
        idx = []
        while len(idx) < 5:
            state = (state & 0xFFFFFFFF) * 4164903690 + (state >> 32)
            v = (state & 0xFFFFFFFF) % n
            if v not in idx:
                idx.append(v)
        out.append(idx)
    return out


def test_first_subsets_of_the_rng_stream():
    """cv::RNG((uint64)-1), uniform(0, n) = next() % n, a repeated index redrawn."""
    first = {6: [[3, 4, 2, 5, 0], [1, 4, 0, 2, 3], [2, 0, 4, 3, 1]],
             65: [[35, 9, 50, 43, 51], [37, 46, 45, 43, 25], [35, 24, 21, 44, 58]]}
    for n, exp in first.items():
        rng = pose_ref.Rng()
        assert [pose_ref.get_subset(rng, n) for _ in range(3)] == exp == _independent_subsets(n, 3)
    assert _pair(pose_cases.small_case(), "len6")["drawn"][0] == first[6][0]


def test_cascade_on_hand_made_counts():
    assert pose_ref.choose([3, 3, 1, 0]) == 0
    assert pose_ref.choose([1, 3, 3, 0]) == 1
    assert pose_ref.choose([0, 1, 2, 2]) == 2
    assert pose_ref.choose([0, 0, 0, 1]) == 3
    assert pose_ref.choose([2, 2, 2, 2]) == 0
    assert pose_ref.choose([1, 2, 3, 3]) == 2
    assert pose_ref.choose([0, 0, 0, 0]) == 0


def test_threshold_never_looks_at_the_right_width():
    assert pose_ref.pixel_threshold(-0.25, (640, 480), (900, 500)) == 0.25
    assert pose_ref.pixel_threshold(0.002, (640, 480), (900, 500)) == 640 * 0.002     # not 900 * 0.002
    assert pose_ref.pixel_threshold(0.002, (900, 500), (640, 480)) == 900 * 0.002     # the left width counts
    assert pose_ref.pixel_threshold(0.002, (300, 200), (900, 500)) == 500 * 0.002


def test_update_num_iters():
    assert pose_ref.update_num_iters(0.999, 0.0, 1000) == 0
    assert pose_ref.update_num_iters(0.999, 1.0, 1000) == 1000
    assert pose_ref.update_num_iters(0.999, 0.5, 1000) == 218     # log(0.001) / log(1 - 0.5^5) = 217.6


def test_golden_file_pins_the_restatement(case):
    """tests/golden/pose_small.npz (tests/golden/make_pose_golden.py) on the small pairs and the noise pair."""
    g = np.load(os.path.join(HERE, "golden", "pose_small.npz"))
    for name in pose_cases.SMALL + ("nan",):
        p = case["names"].index(name)
        a, b = case["offsets"][p], case["offsets"][p + 1]
        r = _pair(case, name)
        assert r["status"] == g["t0_status"][p]
        assert r["E"].tobytes() == g["t0_E"][p].tobytes() and r["pose"].tobytes() == g["t0_pose"][p].tobytes()
        assert np.array_equal(r["mask"], g["t0_mask"][a:b].astype(bool))
        assert (r["n_ransac"], r["n_inliers"]) == (g["t0_n_ransac_inliers"][p], g["t0_n_inliers"][p])
    r = pose_ref.relative_poses(*pose_cases.args(pose_cases.noise_case()), threshold=-1.0,
                                max_iters=pose_cases.NOISE_MAX_ITERS)
    for k in ("status", "E", "pose", "mask", "n_ransac_inliers", "n_inliers", "matches", "pair_offsets"):
        assert r[k].tobytes() == g[f"noise_{k}"].tobytes(), k
    assert g["t0_pair_offsets"][-1] == np.count_nonzero(g["t0_mask"]) == len(g["t0_matches"])
