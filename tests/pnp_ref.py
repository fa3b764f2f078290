"""numpy restatement of SfM::findCameraPoseFrom3d2dMatch (SfM.cpp:453-489) — the
specification csrc/pnp_math.hpp and csrc/pnp.hip are held to, bit for bit.

ShotMatches3d2d::getDistinct3d2dPoints (Scene.cpp:264-278), cv::solvePnPRansac (EPnP RANSAC, the iterative refit on
the inliers), and the inlier ratio of SfM.cpp:479, as OpenCV 4.5.1 runs them, with EPnP's cvSVD / cvInvert / cvSolve
replaced by deterministic, libm-free routines (§8i):
  eigenvectors    of the symmetric 3x3 and 12x12 by cyclic two-sided Jacobi rotations in row-major pair order;
  control matrix  (pseudo-)inverted through the 3x3 eigenpairs, a direction without extent truncated;
  least squares   (6 x 3, 6 x 4, 6 x 5 and the 6 x 4 of Gauss-Newton) by epnp's own Householder qr_solve;
  orientation     the 3x3 SVD is the one-sided Jacobi of tri_ref / pose_ref with a genuine third column of U.
Every step is one correctly rounded IEEE + - * / sqrt on float64 (float32 where named); scalar code is Python
float arithmetic, the per-point parts are elementwise numpy.  The RANSAC stage takes nothing from libm but sqrt and
the log of RANSACUpdateNumIters; the final solvePnP(ITERATIVE) refit (last section) also needs sin, cos and acos,
so its pose is compared within a tolerance and not as bits.
"""
import math

import numpy as np

from tri_ref import F32, F64, EPS, MAX_SWEEPS, cam_params, project, undistort
from pose_ref import Rng, get_subset, update_num_iters, _div, _finite, _det3

MODEL_POINTS = 5
CONFIDENCE = 0.99             # solvePnPRansac's default
MAX_ITERS = 100               # iterationsCount
EIG_SWEEPS = 30
GN_STEPS = 5
# Float coordinates carry a relative rounding of 2^-24, which gives a flat sample an eigenvalue ratio of up to about
# 2^-48 = 4e-15; 1e-12 is 300 times that, and a sample whose thickness is 1e-6 of its extent is still kept.
PLANE_EPS = 1e-12
INF = float("inf")
QNAN = F64(np.nan)


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


# ---------------------------------------------------------------------------- linear algebra

def _si(n, i, j):
    """Index of (i, j) in the packed upper triangle of a symmetric n x n."""
    if i > j:
        i, j = j, i
    return i * n - (i * (i - 1)) // 2 + (j - i)


def jacobi_eig(A, n):
    """Cyclic Jacobi on the packed symmetric A (n (n + 1) / 2, overwritten: its diagonal becomes the
    eigenvalues).  -> Vt (n x n flat): row j is the eigenvector of A[_si(n, j, j)].  Pairs (p, q), p < q, in
    row-major order; a pair is skipped when |a_pq| <= EPS * (the largest |diagonal| of the input); at most
    EIG_SWEEPS sweeps."""
    Vt = [1.0 if i == k else 0.0 for i in range(n) for k in range(n)]
    big = 0.0
    for i in range(n):
        v = abs(A[_si(n, i, i)])
        if v > big:
            big = v
    tol = float(EPS) * big
    for _ in range(EIG_SWEEPS):
        changed = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                ipq = _si(n, p, q)
                apq = A[ipq]
                if abs(apq) <= tol:
                    continue
                ipp, iqq = _si(n, p, p), _si(n, q, q)
                app, aqq = A[ipp], A[iqq]
                theta = _div(aqq - app, 2.0 * apq)
                t = _div(1.0, abs(theta) + _sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = _div(1.0, _sqrt(t * t + 1.0))
                s = t * c
                for k in range(n):
                    if k == p or k == q:
                        continue
                    ikp, ikq = _si(n, k, p), _si(n, k, q)
                    akp, akq = A[ikp], A[ikq]
                    A[ikp] = c * akp - s * akq
                    A[ikq] = s * akp + c * akq
                A[ipp] = app - t * apq
                A[iqq] = aqq + t * apq
                A[ipq] = 0.0
                for k in range(n):
                    vp, vq = Vt[n * p + k], Vt[n * q + k]
                    Vt[n * p + k] = c * vp - s * vq
                    Vt[n * q + k] = s * vp + c * vq
                changed = True
        if not changed:
            break
    return Vt


def qr_solve(A, b, nr, nc):
    """epnp::qr_solve: least squares of the nr x nc system (A flat row-major, A and b overwritten) by
    Householder reflections, column by column.  -> x (nc) or None when a column is zero."""
    A1, A2 = [0.0] * nc, [0.0] * nc
    for k in range(nc):
        eta = abs(A[k * nc + k])
        for i in range(k + 1, nr):
            v = abs(A[i * nc + k])
            if v > eta:
                eta = v
        if not eta > 0.0:                      # zero (or NaN) column
            return None
        inv_eta = 1.0 / eta
        sm = 0.0
        for i in range(k, nr):
            A[i * nc + k] = A[i * nc + k] * inv_eta
            sm = sm + A[i * nc + k] * A[i * nc + k]
        sigma = _sqrt(sm)
        if A[k * nc + k] < 0.0:
            sigma = -sigma
        A[k * nc + k] = A[k * nc + k] + sigma
        A1[k] = sigma * A[k * nc + k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            sm = 0.0
            for i in range(k, nr):
                sm = sm + A[i * nc + k] * A[i * nc + j]
            tau = _div(sm, A1[k])
            for i in range(k, nr):
                A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau = tau + A[i * nc + j] * b[i]
        tau = _div(tau, A1[j])
        for i in range(j, nr):
            b[i] = b[i] - tau * A[i * nc + j]
    x = [0.0] * nc
    x[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        sm = 0.0
        for j in range(i + 1, nc):
            sm = sm + A[i * nc + j] * x[j]
        x[i] = _div(b[i] - sm, A2[i])
    return x


def svd3_full(M):
    """M (9, row-major) -> U (3x3), Vt (3x3), M = U diag(w) Vt: pose_ref.svd3's one-sided Jacobi on the rows of
    M^T, rows sorted by descending norm, the columns of U the normalised rows; the third is the cross product of the
    first two when its singular value is not above EPS times the largest (rank 2: coplanar points)."""
    At = [[M[3 * k + i] for k in range(3)] for i in range(3)]
    V = [[1.0 if i == k else 0.0 for k in range(3)] for i in range(3)]
    W = [_dot3(At[i], At[i]) for i in range(3)]
    eps = float(EPS)
    for _ in range(MAX_SWEEPS):
        changed = False
        for i, j in ((0, 1), (0, 2), (1, 2)):
            p = _dot3(At[i], At[j])
            if abs(p) <= eps * _sqrt(W[i] * W[j]):
                continue
            p = 2.0 * p
            beta = W[i] - W[j]
            gamma = _sqrt(p * p + beta * beta)
            if beta < 0:
                s = _sqrt(_div((gamma - beta) * 0.5, gamma))
                c = _div(p, gamma * s * 2.0)
            else:
                c = _sqrt(_div(gamma + beta, gamma * 2.0))
                s = _div(p, gamma * c * 2.0)
            for Mx in (At, V):
                for k in range(3):
                    t0 = c * Mx[i][k] + s * Mx[j][k]
                    t1 = c * Mx[j][k] - s * Mx[i][k]
                    Mx[i][k], Mx[j][k] = t0, t1
            W[i] = _dot3(At[i], At[i])
            W[j] = _dot3(At[j], At[j])
            changed = True
        if not changed:
            break
    W = [_sqrt(_dot3(At[i], At[i])) for i in range(3)]
    for i in range(2):                      # selection sort, descending
        j = i
        for k in range(i + 1, 3):
            if W[j] < W[k]:
                j = k
        if j != i:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            V[i], V[j] = V[j], V[i]
    u = [[_div(At[c][r], W[c]) for r in range(3)] for c in range(2)]
    if W[2] > float(EPS) * W[0]:
        u.append([_div(At[2][r], W[2]) for r in range(3)])
    else:                                   # rank 2 (coplanar points): completed by the cross product
        u.append([u[0][1] * u[1][2] - u[0][2] * u[1][1], u[0][2] * u[1][0] - u[0][0] * u[1][2],
                  u[0][0] * u[1][1] - u[0][1] * u[1][0]])
    U = [[u[c][r] for c in range(3)] for r in range(3)]
    return U, V


# ---------------------------------------------------------------------------- EPnP on five points

COLS = ((0, 1, 3, 6), (0, 1, 2), (0, 1, 2, 3, 4))       # columns of L_6x10 of the three beta approximations
PAIR6 = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def control_points(pw):
    """-> (cws 4 x 3, PW0 5 x 3, rows of the control matrix's pseudo-inverse, whether the sample has
    extent in all three directions) or None: the centroid and the three
    principal directions of PW0^T PW0, scaled by sqrt(lambda / n), largest eigenvalue first.  A direction whose
    eigenvalue is not above PLANE_EPS times the largest (a coplanar or collinear sample) is truncated."""
    c0 = [_div((((pw[0][j] + pw[1][j]) + pw[2][j]) + pw[3][j]) + pw[4][j], 5.0) for j in range(3)]
    d = [[pw[i][j] - c0[j] for j in range(3)] for i in range(5)]
    S = []
    for a in range(3):
        for b in range(a, 3):
            sm = 0.0
            for i in range(5):
                sm = sm + d[i][a] * d[i][b]
            S.append(sm)
    Vt = jacobi_eig(S, 3)
    lam = [S[0], S[3], S[5]]
    order = []
    for _ in range(3):                      # descending; the first largest wins, a NaN never does
        best, bi = -INF, -1
        for i in range(3):
            if i not in order and lam[i] > best:
                best, bi = lam[i], i
        if bi < 0:
            return None
        order.append(bi)
    cws, ci = [c0], []
    for m in range(3):
        lm = lam[order[m]]
        k = _sqrt(_div(lm, 5.0))
        v = [Vt[3 * order[m] + j] for j in range(3)]
        if lm > PLANE_EPS * lam[order[0]]:
            cws.append([c0[j] + k * v[j] for j in range(3)])
            ci.append([_div(v[j], k) for j in range(3)])
        else:                               # no extent in this direction: the control point is the centroid
            cws.append(list(c0))
            ci.append([0.0, 0.0, 0.0])
    return cws, d, ci, lam[order[2]] > PLANE_EPS * lam[order[0]]


def barycentric(ci, d):
    """alphas (5 x 4).  The control matrix has the columns k_m v_m with orthonormal v_m, so row m of its
    (pseudo-)inverse is v_m / k_m, and zero for a direction without extent."""
    al = []
    for i in range(5):
        a = [_dot3(ci[j], d[i]) for j in range(3)]
        al.append([((1.0 - a[0]) - a[1]) - a[2], a[0], a[1], a[2]])
    return al


def mtm(al, uv):
    """The 10 x 12 M of fill_M with fu = fv = 1, uc = vc = 0, and the packed upper triangle of M^T M."""
    M = []
    for i in range(5):
        r1, r2 = [], []
        for k in range(4):
            r1 += [al[i][k], 0.0, al[i][k] * (0.0 - uv[i][0])]
            r2 += [0.0, al[i][k], al[i][k] * (0.0 - uv[i][1])]
        M += [r1, r2]
    S = []
    for a in range(12):
        for b in range(a, 12):
            sm = 0.0
            for r in range(10):
                sm = sm + M[r][a] * M[r][b]
            S.append(sm)
    return S


def smallest4(S, Vt, n=12):
    """Rows of Vt of the four smallest eigenvalues among the first n, ascending (the first smallest wins)."""
    lam = [S[_si(12, i, i)] for i in range(12)]
    order = []
    for _ in range(4):
        best, bi = INF, -1
        for i in range(n):
            if i not in order and lam[i] < best:
                best, bi = lam[i], i
        if bi < 0:
            return None
        order.append(bi)
    return [[Vt[12 * i + k] for k in range(12)] for i in order]


def l_6x10(v):
    L = []
    for a, b in PAIR6:
        dv = [[v[i][3 * a + k] - v[i][3 * b + k] for k in range(3)] for i in range(4)]
        L.append([_dot3(dv[0], dv[0]), 2.0 * _dot3(dv[0], dv[1]), _dot3(dv[1], dv[1]), 2.0 * _dot3(dv[0], dv[2]),
                  2.0 * _dot3(dv[1], dv[2]), _dot3(dv[2], dv[2]), 2.0 * _dot3(dv[0], dv[3]), 2.0 * _dot3(dv[1], dv[3]),
                  2.0 * _dot3(dv[2], dv[3]), _dot3(dv[3], dv[3])])
    return L


def _dist2(p, q):
    a, b, c = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return (a * a + b * b) + c * c


def betas_approx(L, rho, which):
    """find_betas_approx_1 / _2 / _3 -> 4 betas or None."""
    cols = COLS[which]
    nc = len(cols)
    x = qr_solve([L[r][c] for r in range(6) for c in cols], list(rho), 6, nc)
    if x is None:
        return None
    if which == 0:
        if x[0] < 0:
            b0 = _sqrt(-x[0])
            return [b0, _div(-x[1], b0), _div(-x[2], b0), _div(-x[3], b0)]
        b0 = _sqrt(x[0])
        return [b0, _div(x[1], b0), _div(x[2], b0), _div(x[3], b0)]
    if x[0] < 0:
        b0 = _sqrt(-x[0])
        b1 = _sqrt(-x[2]) if x[2] < 0 else 0.0
    else:
        b0 = _sqrt(x[0])
        b1 = _sqrt(x[2]) if x[2] > 0 else 0.0
    if x[1] < 0:
        b0 = -b0
    return [b0, b1, 0.0 if which == 1 else _div(x[3], b0), 0.0]


def gauss_newton(L, rho, b):
    """Five Gauss-Newton steps on the betas; None when a step's system has a zero column."""
    b = list(b)
    for _ in range(GN_STEPS):
        A, r = [], []
        for i in range(6):
            l = L[i]
            A += [((2.0 * l[0] * b[0] + l[1] * b[1]) + l[3] * b[2]) + l[6] * b[3],
                  ((l[1] * b[0] + 2.0 * l[2] * b[1]) + l[4] * b[2]) + l[7] * b[3],
                  ((l[3] * b[0] + l[4] * b[1]) + 2.0 * l[5] * b[2]) + l[8] * b[3],
                  ((l[6] * b[0] + l[7] * b[1]) + l[8] * b[2]) + 2.0 * l[9] * b[3]]
            r.append(rho[i] - (((((((((l[0] * b[0] * b[0] + l[1] * b[0] * b[1]) + l[2] * b[1] * b[1]) + l[3] * b[0] * b[2])
                                     + l[4] * b[1] * b[2]) + l[5] * b[2] * b[2]) + l[6] * b[0] * b[3]) + l[7] * b[1] * b[3])
                                 + l[8] * b[2] * b[3]) + l[9] * b[3] * b[3]))
        x = qr_solve(A, r, 6, 4)
        if x is None:
            return None
        b = [b[k] + x[k] for k in range(4)]
    return b


def beta_planar(v0, rho):
    """The one beta of a coplanar sample (EPnP's case N = 1 on the three control points that span the plane):
    sum(|v_a - v_b| |c_a - c_b|) / sum(|v_a - v_b|^2) over the pairs (0, 1), (0, 2), (1, 2)."""
    num, den = 0.0, 0.0
    for r in (0, 1, 3):
        a, b = PAIR6[r]
        dv = [v0[3 * a + k] - v0[3 * b + k] for k in range(3)]
        q = _dot3(dv, dv)
        num = num + _sqrt(q) * _sqrt(rho[r])
        den = den + q
    return [_div(num, den), 0.0, 0.0, 0.0]


def r_and_t(v, b, al, pw, d, c0, uv):
    """compute_R_and_t: -> (R 9, t 3, the mean reprojection error)."""
    ccs = [[((b[0] * v[0][3 * j + k] + b[1] * v[1][3 * j + k]) + b[2] * v[2][3 * j + k]) + b[3] * v[3][3 * j + k]
            for k in range(3)] for j in range(4)]
    pcs = [[((al[i][0] * ccs[0][j] + al[i][1] * ccs[1][j]) + al[i][2] * ccs[2][j]) + al[i][3] * ccs[3][j]
            for j in range(3)] for i in range(5)]
    if pcs[0][2] < 0.0:
        pcs = [[-x for x in p] for p in pcs]
    pc0 = [_div((((pcs[0][j] + pcs[1][j]) + pcs[2][j]) + pcs[3][j]) + pcs[4][j], 5.0) for j in range(3)]
    abt = []
    for j in range(3):
        for k in range(3):
            sm = 0.0
            for i in range(5):
                sm = sm + (pcs[i][j] - pc0[j]) * d[i][k]
            abt.append(sm)
    U, Vt = svd3_full(abt)
    R = [[(U[i][0] * Vt[0][j] + U[i][1] * Vt[1][j]) + U[i][2] * Vt[2][j] for j in range(3)] for i in range(3)]
    if _det3(R) < 0:
        R[2] = [-x for x in R[2]]
    t = [pc0[i] - _dot3(R[i], c0) for i in range(3)]
    sm = 0.0
    for i in range(5):
        iz = _div(1.0, _dot3(R[2], pw[i]) + t[2])
        du = uv[i][0] - (_dot3(R[0], pw[i]) + t[0]) * iz
        dv = uv[i][1] - (_dot3(R[1], pw[i]) + t[1]) * iz
        sm = sm + _sqrt(du * du + dv * dv)
    return [x for r in R for x in r], t, _div(sm, 5.0)


def epnp5(pw, uv, detail=False):
    """epnp::compute_pose on five points.  pw: 5 x 3 (the float-rounded 3-D points), uv: 5 x 2 (normalised image
    points).  -> the pose, 12 floats hconcat(R, t) row-major, or None.  detail: -> (pose, N, rep_error)."""
    pw = [[float(x) for x in p] for p in pw]
    uv = [[float(x) for x in p] for p in uv]
    cp = control_points(pw)
    if cp is None:
        return None
    cws, d, ci, full = cp
    al = barycentric(ci, d)
    S = mtm(al, uv)
    Vt = jacobi_eig(S, 12)
    # A coplanar sample has three control points: the fourth's columns of M are exactly zero, the rotations never
    # touch them, and its unit eigenvectors (indices 9-11) are left out.
    v = smallest4(S, Vt, 12 if full else 9)
    if v is None:
        return None
    rho = [_dist2(cws[a], cws[b]) for a, b in PAIR6]
    res = []
    if full:
        L = l_6x10(v)
    for which in range(3):
        if full:
            b = betas_approx(L, rho, which)
            if b is not None:
                b = gauss_newton(L, rho, b)
        else:
            b = beta_planar(v[0], rho) if which == 0 else None
        if b is None:
            res.append((None, INF))
            continue
        R, t, e = r_and_t(v, b, al, pw, d, cws[0], uv)
        pose = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
        ok = all(_finite(x) for x in pose) and _finite(e)
        res.append((pose, e if ok else INF))
    N = 0
    if res[1][1] < res[0][1]:
        N = 1
    if res[2][1] < res[N][1]:
        N = 2
    if not res[N][1] < INF:
        return None
    return (res[N][0], N + 1, res[N][1]) if detail else res[N][0]


# ---------------------------------------------------------------------------- RANSAC

@np.errstate(all="ignore")
def reprojection_error(pose, X32, pt, cam):
    """PnPRansacCallback::computeError: projectPoints (double, rounded to float) against the float image points;
    the difference and dx dx + dy dy in float."""
    u, v = project(X32[:, 0], X32[:, 1], X32[:, 2], pose, cam)
    du = (u - pt[:, 0]).astype(F32)
    dv = (v - pt[:, 1]).astype(F32)
    return (du * du + dv * dv).astype(F32)


def sample_pose(X32, pt, cam, idx):
    """PnPRansacCallback::runKernel: undistortPoints of the five image points, then EPnP."""
    x, y = undistort(pt[idx], cam)
    return epnp5(X32[idx].astype(F64), np.stack([x, y], axis=1).astype(F64))


def pixel_threshold(threshold, size):
    """ransacReprojectionPoseThreshold: < 0 pixels, > 0 a fraction of max(width, height); through the float
    parameter of solvePnPRansac.  -> the float the errors are compared with, (float)(thr * thr)."""
    thr = -float(threshold) if threshold < 0 else float(max(int(size[0]), int(size[1]))) * float(threshold)
    thr = float(F32(thr))
    return F32(thr * thr)


def ransac(X32, pt, cam, t, confidence=CONFIDENCE, max_iters=MAX_ITERS):
    """RANSACPointSetRegistrator::run, modelPoints = 5, n > 5.  -> (pose or None, mask, subsets drawn)."""
    n = len(X32)
    mask = np.zeros(n, bool)
    rng = Rng()
    niters, max_good, best = max(max_iters, 1), 0, None
    drawn = []
    it = 0
    while it < niters:
        idx = get_subset(rng, n)
        if idx is None:
            if it == 0:
                return None, mask, drawn
            break
        drawn.append(idx)
        pose = sample_pose(X32, pt, cam, idx)
        if pose is not None:
            good = int(np.count_nonzero(reprojection_error(pose, X32, pt, cam) <= t))
            if good > max(max_good, MODEL_POINTS - 1):
                best, max_good = pose, good
                niters = update_num_iters(confidence, (n - good) / n, niters)
        it += 1
    if best is None:
        return None, mask, drawn
    return best, reprojection_error(best, X32, pt, cam) <= t, drawn


def register_set(p3, p2, cam, size, threshold=-8.0, confidence=CONFIDENCE, max_iters=MAX_ITERS):
    """One candidate set: p3 (n x 3) float64, p2 (n x 2) float64, as getDistinct3d2dPoints delivers them.
    -> dict(status, pose (12, after the refit), ransac_pose (12), mask, n_inliers, inlier_ratio, refit_start, drawn).
    status 0: no pose (fewer than 4 points, no model); 1: a pose; 2: exactly 4 points (P3P: the host's)."""
    n = len(p3)
    out = dict(status=0, pose=np.full(12, QNAN), ransac_pose=np.full(12, QNAN), mask=np.zeros(n, bool), n_inliers=0,
               inlier_ratio=-1.0, refit_start=-1, drawn=[])
    if n < 4:
        return out
    if n == 4:
        out["status"] = 2
        return out
    X32 = np.ascontiguousarray(p3, F64).reshape(-1, 3).astype(F32)      # solvePnPRansac: both to float first
    pt = np.ascontiguousarray(p2, F64).reshape(-1, 2).astype(F32)
    if n == MODEL_POINTS:
        pose = sample_pose(X32, pt, cam, list(range(5)))
        mask = np.ones(5, bool)
    else:
        pose, mask, out["drawn"] = ransac(X32, pt, cam, pixel_threshold(threshold, size), confidence, max_iters)
    if pose is None:
        return out
    final, start = pose, -1                 # 5 points: no refit
    if n > MODEL_POINTS:
        rf = refit(X32, pt, mask, cam, pose)
        if rf is None:
            return out                       # a failing refit: no pose
        final, start = rf
    ni = int(np.count_nonzero(mask))
    # SfM.cpp:479 counts the non-zero entries of the inlier *index* list: index 0 is never counted
    out.update(status=1, pose=np.array(final, F64), ransac_pose=np.array(pose, F64), refit_start=start, mask=mask, n_inliers=ni,
               inlier_ratio=float(F64(ni - int(mask[0])) / F64(n)))
    return out


def register_poses(points3d, points2d, set_offsets, set_shot, cameras, shot_camera, shot_size, threshold=-8.0,
                   confidence=CONFIDENCE, max_iters=MAX_ITERS):
    """The whole call of sfmx_register_poses: dict of the ABI's output arrays."""
    p3 = np.asarray(points3d, F64).reshape(-1, 3)
    p2 = np.asarray(points2d, F64).reshape(-1, 2)
    off = np.asarray(set_offsets, np.int64)
    cams = [cam_params(K, d) for K, d in cameras]
    size = np.asarray(shot_size, np.int32).reshape(-1, 2)
    ns = len(off) - 1
    out = dict(status=np.zeros(ns, np.int32), pose=np.full((ns, 12), QNAN), ransac_pose=np.full((ns, 12), QNAN),
               mask=np.zeros(len(p3), np.uint8), n_inliers=np.zeros(ns, np.int32), inlier_ratio=np.full(ns, -1.0),
               refit_start=np.full(ns, -1, np.int32))
    for s in range(ns):
        a, b = int(off[s]), int(off[s + 1])
        sh = int(set_shot[s])
        r = register_set(p3[a:b], p2[a:b], cams[shot_camera[sh]], size[sh], threshold, confidence, max_iters)
        out["status"][s] = r["status"]
        out["ransac_pose"][s] = r["ransac_pose"]
        out["pose"][s] = r["pose"]
        out["refit_start"][s] = r["refit_start"]
        out["mask"][a:b] = r["mask"]
        out["n_inliers"][s] = r["n_inliers"]
        out["inlier_ratio"][s] = r["inlier_ratio"]
    return out


# ---------------------------------------------------------------------------- getDistinct3d2dPoints

def distinct_3d2d(cloud_xyz, origin_offsets, found_keypoint, found_xy):
    """f4's per-origin-record output -> the distinct (Point3d, Point2d) list (xyz n x 3, xy n x 2), in
    first-appearance order over the point-major records.  A record with a match (found_keypoint >= 0) is dropped
    iff an earlier kept record has == coordinates in all five doubles (-0 == +0; a NaN never equals anything)."""
    xyz = np.asarray(cloud_xyz, F64).reshape(-1, 3)
    off = np.asarray(origin_offsets, np.int64)
    kp = np.asarray(found_keypoint, np.int32).reshape(-1)
    xy = np.asarray(found_xy, F64).reshape(-1, 2)
    rows, seen = [], {}
    for p in range(len(xyz)):
        for r in range(int(off[p]), int(off[p + 1])):
            if kp[r] < 0:
                continue
            row = (float(xyz[p, 0]), float(xyz[p, 1]), float(xyz[p, 2]), float(xy[r, 0]), float(xy[r, 1]))
            if any(v != v for v in row):
                rows.append(row)                 # never equal to anything, itself included
                continue
            key = tuple(v + 0.0 for v in row)    # -0.0 + 0.0 == +0.0: one key for both zeros
            if key in seen:
                continue
            seen[key] = True
            rows.append(row)
    a = np.array(rows, F64).reshape(-1, 5)
    return np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3:])


# ---------------------------------------------------------------------------- the refit: solvePnP(ITERATIVE)

NT = 256                      # slots of the fixed summation tree (the kernel's threads)
LM_ITERS = 20
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
POW10 = {k: float("1e%d" % k) for k in range(-16, 17)}


def _sin(x):
    return math.sin(x)


def _cos(x):
    return math.cos(x)


def _acos(x):
    return math.acos(x)


def tree_sum(v):
    """v (n x k) -> (k): slot s adds rows s, s + NT, ... in order from 0.0, then the slots are folded in halves
    (128, 64, ... 1): the order of the kernel's sums over a set."""
    v = np.asarray(v, F64)
    n, k = v.shape
    rows = (n + NT - 1) // NT
    pad = np.zeros((max(rows, 1) * NT, k))
    pad[:n] = v
    acc = np.zeros((NT, k))
    for r in range(rows):
        acc = acc + pad[r * NT:(r + 1) * NT]
    s = NT // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0].copy()


@np.errstate(all="ignore")
def undistort64(pt, cam):
    """cvUndistortPoints into CV_64F, as cvFindExtrinsicCameraParams2 calls it: tri_ref.undistort without the
    rounding to float."""
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    k1, k2, p1, p2, k3 = cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"]
    ifx, ify = F64(1.0) / fx, F64(1.0) / fy
    x = (pt[:, 0].astype(F64) - cx) * ifx
    y = (pt[:, 1].astype(F64) - cy) * ify
    x0, y0 = x, y
    live = np.ones(len(x), bool)
    for _ in range(5):
        r2 = x * x + y * y
        icdist = F64(1.0) / (F64(1.0) + ((k3 * r2 + k2) * r2 + k1) * r2)
        neg = live & (icdist < 0)
        dX = F64(2.0) * p1 * x * y + p2 * (r2 + F64(2.0) * x * x)
        dY = p1 * (r2 + F64(2.0) * y * y) + F64(2.0) * p2 * x * y
        nx = (x0 - dX) * icdist
        ny = (y0 - dY) * icdist
        upd = live & ~neg
        x = np.where(neg, x0, np.where(upd, nx, x))
        y = np.where(neg, y0, np.where(upd, ny, y))
        live = upd
    return x, y


EYE9 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
GEN = ((0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0),
       (0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0))


def rodrigues(r):
    """cvRodrigues2, vector -> matrix with its Jacobian: (R 9, dR 3 x 9)."""
    theta = _sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if not theta >= DBL_EPSILON:
        return list(EYE9), [list(g) for g in GEN]
    c, s = _cos(theta), _sin(theta)
    c1 = 1.0 - c
    it = 1.0 / theta
    x, y, z = r[0] * it, r[1] * it, r[2] * it
    rrt = (x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z)
    rx = (0.0, -z, y, z, 0.0, -x, -y, x, 0.0)
    R = [(c * EYE9[k] + c1 * rrt[k]) + s * rx[k] for k in range(9)]
    drrt = ((x + x, y, z, y, 0.0, 0.0, z, 0.0, 0.0), (0.0, x, 0.0, x, y + y, z, 0.0, z, 0.0),
            (0.0, 0.0, x, 0.0, 0.0, y, x, y, z + z))
    dR = []
    for i, ri in enumerate((x, y, z)):
        a0, a1, a2, a3, a4 = -s * ri, (s - 2.0 * c1 * it) * ri, c1 * it, (c - s * it) * ri, s * it
        dR.append([(((a0 * EYE9[k] + a1 * rrt[k]) + a2 * drrt[i][k]) + a3 * rx[k]) + a4 * GEN[i][k] for k in range(9)])
    return R, dR


def rodrigues_inv(R):
    """cvRodrigues2, matrix -> vector (without its re-orthonormalisation: R comes from an SVD or from EPnP)."""
    rx, ry, rz = R[7] - R[5], R[2] - R[6], R[3] - R[1]
    s = _sqrt(((rx * rx + ry * ry) + rz * rz) * 0.25)
    c = ((R[0] + R[4]) + R[8] - 1.0) * 0.5
    c = 1.0 if c > 1.0 else (-1.0 if c < -1.0 else c)
    theta = _acos(c)
    if s < 1e-5:
        if c > 0:
            return [0.0, 0.0, 0.0]
        t = (R[0] + 1.0) * 0.5
        rx = _sqrt(t if t > 0.0 else 0.0)
        t = (R[4] + 1.0) * 0.5
        ry = _sqrt(t if t > 0.0 else 0.0) * (-1.0 if R[1] < 0 else 1.0)
        t = (R[8] + 1.0) * 0.5
        rz = _sqrt(t if t > 0.0 else 0.0) * (-1.0 if R[2] < 0 else 1.0)
        if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[5] > 0) != (ry * rz > 0):
            rz = -rz
        theta = _div(theta, _sqrt((rx * rx + ry * ry) + rz * rz))
        return [rx * theta, ry * theta, rz * theta]
    vth = (1.0 / (2.0 * s)) * theta
    return [rx * vth, ry * vth, rz * vth]


@np.errstate(all="ignore")
def residuals(param, M, pt, w, cam):
    """cvProjectPoints2 with dp/dr, dp/dt at param = (rvec, tvec), reduced over the set: w is the inlier mask (another point
    contributes 0.0).  -> 28 sums: JtJ (upper triangle, 21, row-major), JtErr (6), |err|^2."""
    R, dR = rodrigues(param[:3])
    R = [F64(v) for v in R]
    t = [F64(v) for v in param[3:]]
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    k1, k2, p1, p2, k3 = cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"]
    X0, X1, X2 = M[:, 0], M[:, 1], M[:, 2]
    X = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0]
    Y = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1]
    Z = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2]
    z = np.where(Z != 0, F64(1.0) / Z, F64(1.0))
    x, y = X * z, Y * z
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    a1 = F64(2.0) * x * y
    a2 = r2 + F64(2.0) * x * x
    a3 = r2 + F64(2.0) * y * y
    cdist = ((F64(1.0) + k1 * r2) + k2 * r4) + k3 * r6
    xd = (x * cdist + p1 * a1) + p2 * a2
    yd = (y * cdist + p1 * a3) + p2 * a1
    eu = (xd * fx + cx) - pt[:, 0]
    ev = (yd * fy + cy) - pt[:, 1]
    dcd = (k1 + F64(2.0) * k2 * r2) + F64(3.0) * k3 * r4
    xdx = ((cdist + F64(2.0) * x * x * dcd) + F64(2.0) * p1 * y) + F64(6.0) * p2 * x
    xdy = (F64(2.0) * x * y * dcd + F64(2.0) * p1 * x) + F64(2.0) * p2 * y
    ydx = (F64(2.0) * x * y * dcd + F64(2.0) * p1 * x) + F64(2.0) * p2 * y
    ydy = ((cdist + F64(2.0) * y * y * dcd) + F64(6.0) * p1 * y) + F64(2.0) * p2 * x
    xz, yz = -(x * z), -(y * z)
    uP = [fx * (xdx * z), fx * (xdy * z), fx * (xdx * xz + xdy * yz)]
    vP = [fy * (ydx * z), fy * (ydy * z), fy * (ydx * xz + ydy * yz)]
    Ju, Jv = [], []
    for i in range(3):
        D = [F64(v) for v in dR[i]]
        q0 = (D[0] * X0 + D[1] * X1) + D[2] * X2
        q1 = (D[3] * X0 + D[4] * X1) + D[5] * X2
        q2 = (D[6] * X0 + D[7] * X1) + D[8] * X2
        Ju.append((uP[0] * q0 + uP[1] * q1) + uP[2] * q2)
        Jv.append((vP[0] * q0 + vP[1] * q1) + vP[2] * q2)
    Ju += uP
    Jv += vP
    cols = []
    for a in range(6):
        for b in range(a, 6):
            cols.append(Ju[a] * Ju[b] + Jv[a] * Jv[b])
    for a in range(6):
        cols.append(Ju[a] * eu + Jv[a] * ev)
    cols.append(eu * eu + ev * ev)
    return tree_sum(np.where(w[:, None], np.stack(cols, axis=1), F64(0.0)))


def solve6(A, b):
    """Gaussian elimination with partial pivoting of the 6 x 6 system (A: list of rows); None on a zero pivot."""
    A = [list(r) + [b[i]] for i, r in enumerate(A)]
    for k in range(6):
        best, pr = 0.0, -1
        for r in range(k, 6):
            v = abs(A[r][k])
            if v > best:
                best, pr = v, r
        if pr < 0:
            return None
        A[k], A[pr] = A[pr], A[k]
        for r in range(k + 1, 6):
            f = _div(A[r][k], A[k][k])
            for c in range(k + 1, 7):
                A[r][c] = A[r][c] - f * A[k][c]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        sm = A[i][6]
        for j in range(i + 1, 6):
            sm = sm - A[i][j] * x[j]
        x[i] = _div(sm, A[i][i])
    return x


def lev_marq(param, M, pt, w, cam):
    """CvLevMarq as cvFindExtrinsicCameraParams2 drives it: at most 20 iterations, FLT_EPSILON on the relative
    step, lambda = 10^k from k = -3 inside [-16, 16], the diagonal of JtJ scaled by 1 + lambda."""
    lg, iters = -3, 0
    prev_norm = 0.0
    while True:
        S = residuals(param, M, pt, w, cam)
        JtJ = [[0.0] * 6 for _ in range(6)]
        k = 0
        for a in range(6):
            for b in range(a, 6):
                JtJ[a][b] = JtJ[b][a] = float(S[k])
                k += 1
        JtE = [float(v) for v in S[21:27]]
        prev = list(param)
        if iters == 0:
            prev_norm = _sqrt(float(S[27]))

        def step():
            lam = POW10[lg]
            A = [[JtJ[a][b] * (1.0 + lam) if a == b else JtJ[a][b] for b in range(6)] for a in range(6)]
            dx = solve6(A, JtE)
            return None if dx is None else [prev[i] - dx[i] for i in range(6)]

        param = step()
        if param is None:
            return None
        while True:
            norm = _sqrt(float(residuals(param, M, pt, w, cam)[27]))
            if norm > prev_norm:
                lg += 1
                if lg <= 16:
                    param = step()
                    if param is None:
                        return None
                    continue
            break
        lg = max(lg - 1, -16)
        iters += 1
        num = _sqrt(sum3sq([param[i] - prev[i] for i in range(6)]))
        den = _sqrt(sum3sq(prev))
        if iters >= LM_ITERS or _div(num, den) < FLT_EPSILON:
            return param
        prev_norm = norm


def sum3sq(v):
    s = 0.0
    for x in v:
        s = s + x * x
    return s


def planar_cov(S):
    """The planarity test on the packed 3 x 3 covariance S (overwritten): eigenvalues descending, W[2] / W[1] < 1e-3;
    a NaN eigenvalue is not planar."""
    jacobi_eig(S, 3)
    W = [S[0], S[3], S[5]]
    if not all(v == v for v in W):
        return False
    W = sorted(W, reverse=True)
    return _div(W[2], W[1]) < 1e-3


def dlt_start(LL):
    """The DLT start from the packed 12 x 12 L^T L (overwritten): the eigenvector of the smallest eigenvalue (the
    first smallest, a NaN never) as 3 x 4, negated when det of its 3 x 3 part is negative, R = U V^T of that part's
    SVD, t scaled by |R|_F / |RR|_F.  -> (R 9, t 3) or None."""
    Vt = jacobi_eig(LL, 12)
    best, bi = INF, -1
    for i in range(12):
        lam = LL[_si(12, i, i)]
        if lam < best:
            best, bi = lam, i
    if bi < 0:
        return None
    P = [Vt[12 * bi + k] for k in range(12)]
    RR = [P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]]
    if _det3([RR[0:3], RR[3:6], RR[6:9]]) < 0:
        P = [-x for x in P]
        RR = [-x for x in RR]
    U, Vt3 = svd3_full(RR)
    R = [(U[i][0] * Vt3[0][j] + U[i][1] * Vt3[1][j]) + U[i][2] * Vt3[2][j] for i in range(3) for j in range(3)]
    sc = _div(_sqrt(sum3sq(R)), _sqrt(sum3sq(RR)))
    t = [P[3] * sc, P[7] * sc, P[11] * sc]
    if not all(_finite(x) for x in R + t):
        return None
    return R, t


def inlier_sums(X32, pt, mask, cam):
    """The refit's sums over the inliers in the fixed tree order: (the packed 3 x 3 covariance, the packed 12 x 12
    L^T L of the DLT)."""
    M = X32.astype(F64)
    wc = np.asarray(mask, bool)[:, None]
    with np.errstate(all="ignore"):
        Mc = tree_sum(np.where(wc, M, F64(0.0))) / F64(int(np.count_nonzero(wc)))
        d = M - Mc
        S = tree_sum(np.where(wc, np.stack([d[:, a] * d[:, b] for a in range(3) for b in range(a, 3)], axis=1), F64(0.0)))
        xn, yn = undistort64(pt, cam)
        one, zero = np.ones(len(M)), np.zeros(len(M))
        r1 = [M[:, 0], M[:, 1], M[:, 2], one, zero, zero, zero, zero, -xn * M[:, 0], -xn * M[:, 1], -xn * M[:, 2], -xn]
        r2 = [zero, zero, zero, zero, M[:, 0], M[:, 1], M[:, 2], one, -yn * M[:, 0], -yn * M[:, 1], -yn * M[:, 2], -yn]
        LL = tree_sum(np.where(wc, np.stack([r1[a] * r1[b] + r2[a] * r2[b] for a in range(12) for b in range(a, 12)], axis=1), F64(0.0)))
    return [float(v) for v in S], [float(v) for v in LL]


@np.errstate(all="ignore")
def refit(X32, pt, mask, cam, ransac_pose):
    """solvePnP(SOLVEPNP_ITERATIVE) on the inliers (cvFindExtrinsicCameraParams2).
    -> (pose 12, refit_start: 0 DLT, 1 the RANSAC's EPnP model) or None."""
    M = X32.astype(F64)
    w = np.asarray(mask, bool)
    m = int(np.count_nonzero(w))
    S, LL = inlier_sums(X32, pt, mask, cam)
    planar = planar_cov(S)
    if planar:
        R = [ransac_pose[k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10)]
        t = [ransac_pose[3], ransac_pose[7], ransac_pose[11]]
        if not all(_finite(x) for x in R + t):
            return None
    else:
        if m < 6:
            return None                      # OpenCV's DLT needs 6 points
        st = dlt_start(LL)
        if st is None:
            return None
        R, t = st
    param = lev_marq(rodrigues_inv(R) + t, M, pt.astype(F64), w, cam)
    if param is None or not all(_finite(x) for x in param):
        return None
    R, _ = rodrigues(param[:3])
    return [R[0], R[1], R[2], param[3], R[3], R[4], R[5], param[4], R[6], R[7], R[8], param[5]], 1 if planar else 0
