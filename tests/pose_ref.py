"""numpy restatement of SfM::findCameraPoseFromMatch (SfM.cpp:491-540) — the specification
csrc/pose_math.hpp and csrc/pose.hip are held to, bit for bit.

cv::findEssentialMat(left, right, K_L, dist_L, K_R, dist_R, RANSAC, 0.999, thr, mask), cv::recoverPose(E, left,
right, K_L, R, t, mask) and the reduction of the match list to the surviving inliers, as OpenCV 4.5.1 runs them,
with the five-point solver's SVD and solvePoly replaced by a deterministic, libm-free route (§8h):
  null space      Gauss-Jordan elimination of the 5x9 epipolar system with complete pivoting;
  constraints     the 10x20 matrix by polynomial products in a fixed accumulation order, reduced by Gauss-Jordan
                  elimination with partial pivoting;
  real roots      of the tenth-degree polynomial by bracketing between the roots of its derivative (recursively,
                  inside the Cauchy bound) and bisection to neighbouring doubles (at most 128 halvings);
  E               x, y from the cross product of two rows of B(z), E = xX + yY + zZ + W over its Frobenius norm.
Every step is one correctly rounded IEEE + - * / sqrt on float64 (float32 where named); scalar code is Python
float arithmetic (IEEE double), the per-match parts are elementwise numpy.  Nothing comes from libm but sqrt and
the log of RANSACUpdateNumIters.
"""
import math

import numpy as np

from tri_ref import F32, F64, EPS, MAX_SWEEPS, cam_params, dlt_matrix, jacobi_null, undistort

MODEL_POINTS = 5
MAX_ATTEMPTS = 10000
CONFIDENCE = 0.999            # SfM.cpp:524
MAX_ITERS = 1000              # RANSACPointSetRegistrator's default
DISTANCE_THRESH = 50.0        # recoverPose's distanceThresh
MAX_HALVINGS = 128
DBL_MIN = 2.2250738585072014e-308
INF = float("inf")

# monomials in x, y, z: degree <= 1, <= 2 and <= 3 (the column order of the constraint matrix)
M1 = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
M2 = ((2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
M3 = ((3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
      (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0))


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


MUL11 = [[M2.index(_add(a, b)) for b in M1] for a in M1]      # (degree 1) x (degree 1) -> index in M2
MUL21 = [[M3.index(_add(a, b)) for b in M1] for a in M2]      # (degree 2) x (degree 1) -> index in M3


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def _finite(v):
    return abs(v) < INF          # false for NaN


# ---------------------------------------------------------------------------- the five-point solver

def null_space(q):
    """q: 5 x (x1, y1, x2, y2).  -> the basis X, Y, Z, W (4 x 9) of the null space of the epipolar system
    x2^T E x1 = 0 (E row-major), or None when a pivot is zero."""
    a = [[x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0] for x1, y1, x2, y2 in q]
    perm = list(range(9))
    for k in range(5):
        best, pr, pc = 0.0, -1, -1
        for r in range(k, 5):
            for c in range(k, 9):
                v = abs(a[r][c])
                if v > best:                      # strict: the first largest wins, a NaN never does
                    best, pr, pc = v, r, c
        if not best > 0.0:
            return None
        a[k], a[pr] = a[pr], a[k]
        for r in range(5):
            a[r][k], a[r][pc] = a[r][pc], a[r][k]
        perm[k], perm[pc] = perm[pc], perm[k]
        p = a[k][k]
        for c in range(k + 1, 9):
            a[k][c] = a[k][c] / p
        for r in range(5):
            if r != k:
                f = a[r][k]
                for c in range(k + 1, 9):
                    a[r][c] = a[r][c] - f * a[k][c]
    N = [[0.0] * 9 for _ in range(4)]
    for j in range(4):
        for i in range(5):
            N[j][perm[i]] = -a[i][5 + j]
        N[j][perm[5 + j]] = 1.0
    return N


def _mul11(out, a, b, sub=False):
    for i in range(4):
        for j in range(4):
            k = MUL11[i][j]
            out[k] = out[k] - a[i] * b[j] if sub else out[k] + a[i] * b[j]


def _mul21(out, a, b, sub=False):
    for i in range(10):
        for j in range(4):
            k = MUL21[i][j]
            out[k] = out[k] - a[i] * b[j] if sub else out[k] + a[i] * b[j]


SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))        # index of (E E^T)[i][k] among its six distinct entries


def constraint_matrix(N):
    """The 10 x 20 coefficients (columns M3) of 2 E E^T E - tr(E E^T) E (rows 0-8) and det E (row 9) for
    E = xX + yY + zZ + W."""
    lin = [[N[0][e], N[1][e], N[2][e], N[3][e]] for e in range(9)]      # entry e of E as a polynomial over M1
    eet = []
    for i in range(3):
        for k in range(i, 3):
            o = [0.0] * 10
            for m in range(3):
                _mul11(o, lin[3 * i + m], lin[3 * k + m])
            eet.append(o)
    tr = [(eet[0][m] + eet[3][m]) + eet[5][m] for m in range(10)]
    A = []
    for i in range(3):
        for j in range(3):
            row = [0.0] * 20
            for k in range(3):
                _mul21(row, eet[SYM[i][k]], lin[3 * k + j])
            row = [2.0 * v for v in row]
            _mul21(row, tr, lin[3 * i + j], sub=True)
            A.append(row)
    row = [0.0] * 20
    for c, (a0, a1, b0, b1) in enumerate(((4, 8, 5, 7), (3, 8, 5, 6), (3, 7, 4, 6))):
        minor = [0.0] * 10
        _mul11(minor, lin[a0], lin[a1])
        _mul11(minor, lin[b0], lin[b1], sub=True)
        _mul21(row, minor, lin[c], sub=(c == 1))
    A.append(row)
    return A


def reduce_matrix(A):
    """Gauss-Jordan elimination of the first 10 columns, partial pivoting; False when a pivot is zero."""
    for k in range(10):
        best, pr = 0.0, -1
        for r in range(k, 10):
            v = abs(A[r][k])
            if v > best:
                best, pr = v, r
        if not best > 0.0:
            return False
        A[k], A[pr] = A[pr], A[k]
        p = A[k][k]
        for c in range(k + 1, 20):
            A[k][c] = A[k][c] / p
        for r in range(10):
            if r != k:
                f = A[r][k]
                for c in range(k + 1, 20):
                    A[r][c] = A[r][c] - f * A[k][c]
    return True


def b_matrix(A):
    """Rows (4 - z 5), (6 - z 7), (8 - z 9) of the reduced matrix: B(z) (x, y, 1)^T = 0.
    -> 3 x (bx[0..3], by[0..3], bc[0..4]), ascending powers of z."""
    B = []
    for p, q in ((4, 5), (6, 7), (8, 9)):
        bx = [A[p][12], A[p][11] - A[q][12], A[p][10] - A[q][11], -A[q][10]]
        by = [A[p][15], A[p][14] - A[q][15], A[p][13] - A[q][14], -A[q][13]]
        bc = [A[p][19], A[p][18] - A[q][19], A[p][17] - A[q][18], A[p][16] - A[q][17], -A[q][16]]
        B.append((bx, by, bc))
    return B


def _conv(out, a, b, sub=False):
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] = out[i + j] - a[i] * b[j] if sub else out[i + j] + a[i] * b[j]


def det_poly(B):
    """det B(z): 11 coefficients, ascending."""
    (bx0, by0, bc0), (bx1, by1, bc1), (bx2, by2, bc2) = B
    p1, p2, p3 = [0.0] * 8, [0.0] * 8, [0.0] * 7
    _conv(p1, by1, bc2)
    _conv(p1, by2, bc1, sub=True)
    _conv(p2, bx1, bc2)
    _conv(p2, bx2, bc1, sub=True)
    _conv(p3, bx1, by2)
    _conv(p3, bx2, by1, sub=True)
    c = [0.0] * 11
    _conv(c, bx0, p1)
    _conv(c, by0, p2, sub=True)
    _conv(c, bc0, p3)
    return c


def _horner(c, d, z):
    v = c[d]
    for i in range(d - 1, -1, -1):
        v = v * z + c[i]
    return v


def real_roots(c):
    """The real roots of the degree-10 polynomial c (ascending coefficients), ascending; [] when the leading
    coefficient is zero or a coefficient or the Cauchy bound is not finite."""
    for v in c:
        if not _finite(v):
            return []
    if c[10] == 0.0:
        return []
    m = 0.0
    for i in range(10):
        v = abs(c[i] / c[10])
        if v > m:
            m = v
    R = 1.0 + m
    if not R < 1e300:
        return []
    dp = [None] * 11                          # dp[d]: the (10 - d)th derivative, degree d
    dp[10] = list(c)
    for d in range(10, 1, -1):
        dp[d - 1] = [dp[d][i + 1] * float(i + 1) for i in range(d)]
    roots = []
    for d in range(1, 11):
        pts = [-R] + roots + [R]
        new = []
        fa = _horner(dp[d], d, pts[0])
        for s in range(len(pts) - 1):
            lo, hi = pts[s], pts[s + 1]
            fb = _horner(dp[d], d, hi)
            neg = fa < 0.0
            if neg != (fb < 0.0):
                for _ in range(MAX_HALVINGS):
                    mid = 0.5 * (lo + hi)
                    if not (lo < mid and mid < hi):
                        break
                    fm = _horner(dp[d], d, mid)
                    if (fm < 0.0) == neg:
                        lo = mid
                    else:
                        hi = mid
                new.append(0.5 * (lo + hi))
            fa = fb
        roots = new
    return roots


def models_from_roots(N, B, roots):
    """Per root z: (x, y, 1) ~ the cross product of two rows of B(z) with the largest third component,
    E = xX + yY + zZ + W over its Frobenius norm; a model with a non-finite entry is dropped."""
    out = []
    for z in roots:
        r = [(_horner(bx, 3, z), _horner(by, 3, z), _horner(bc, 4, z)) for bx, by, bc in B]
        best, cx, cy, cz = -1.0, 0.0, 0.0, 0.0
        for a, b in ((0, 1), (0, 2), (1, 2)):
            c0 = r[a][1] * r[b][2] - r[a][2] * r[b][1]
            c1 = r[a][2] * r[b][0] - r[a][0] * r[b][2]
            c2 = r[a][0] * r[b][1] - r[a][1] * r[b][0]
            if abs(c2) > best:
                best, cx, cy, cz = abs(c2), c0, c1, c2
        x, y = _div(cx, cz), _div(cy, cz)
        E = [((x * N[0][e] + y * N[1][e]) + z * N[2][e]) + N[3][e] for e in range(9)]
        s = 0.0
        for e in range(9):
            s = s + E[e] * E[e]
        nrm = math.sqrt(s) if s >= 0.0 else math.nan
        E = [_div(v, nrm) for v in E]
        if all(_finite(v) for v in E):
            out.append(E)
    return out


def five_point(q):
    """EMEstimatorCallback::runKernel on 5 correspondences (x1, y1, x2, y2): 0-10 essential matrices (9 floats,
    row-major, unit Frobenius norm) in ascending order of the root z."""
    N = null_space([[float(v) for v in row] for row in q])
    if N is None:
        return []
    A = constraint_matrix(N)
    if not reduce_matrix(A):
        return []
    B = b_matrix(A)
    return models_from_roots(N, B, real_roots(det_poly(B)))


# ---------------------------------------------------------------------------- RANSAC

@np.errstate(all="ignore")
def sampson_error(E, P):
    """EMEstimatorCallback::computeError: P (n x 4) float64 -> float32 errors."""
    x1, y1, x2, y2 = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    E = [F64(v) for v in E]
    e0 = (E[0] * x1 + E[1] * y1) + E[2]
    e1 = (E[3] * x1 + E[4] * y1) + E[5]
    e2 = (E[6] * x1 + E[7] * y1) + E[8]
    t0 = (E[0] * x2 + E[3] * y2) + E[6]
    t1 = (E[1] * x2 + E[4] * y2) + E[7]
    s = (x2 * e0 + y2 * e1) + e2
    return ((s * s) / (((e0 * e0 + e1 * e1) + t0 * t0) + t1 * t1)).astype(F32)


class Rng:
    """cv::RNG"""

    def __init__(self, state=(1 << 64) - 1):
        self.state = state

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & ((1 << 64) - 1)
        return self.state & 0xFFFFFFFF

    def uniform(self, n):
        return self.next() % n


def get_subset(rng, count):
    """RANSACPointSetRegistrator::getSubset without checkSubset: 5 distinct indices, a repeated one is redrawn;
    None after MAX_ATTEMPTS values without five distinct ones (the bound that stands for maxAttempts)."""
    idx = []
    for _ in range(MAX_ATTEMPTS):
        v = rng.uniform(count)
        if v not in idx:
            idx.append(v)
            if len(idx) == MODEL_POINTS:
                return idx
    return None


def update_num_iters(p, ep, max_iters):
    """RANSACUpdateNumIters with modelPoints = 5 (oracle/homography_oracle.cpp:293-304)."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    q = 1.0 - ep
    q2 = q * q
    denom = 1.0 - q2 * q2 * q
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(np.rint(num / denom))


def ransac(P, thr, confidence=CONFIDENCE, max_iters=MAX_ITERS):
    """P: (n x 4) float64 normalised correspondences, thr: the normalised threshold.
    -> (E or None, mask (n) bool, subsets drawn)."""
    n = len(P)
    mask = np.zeros(n, bool)
    if n < MODEL_POINTS:
        return None, mask, []
    t = F32(thr * thr)
    rng = Rng()
    niters, max_good, best = max(max_iters, 1), 0, None
    drawn = []
    it = 0
    while it < niters:
        if n > MODEL_POINTS:
            idx = get_subset(rng, n)
            if idx is None:
                if it == 0:
                    return None, mask, drawn
                break
            drawn.append(idx)
        else:
            idx = list(range(MODEL_POINTS))
        for E in five_point(P[idx]):
            good = int(np.count_nonzero(sampson_error(E, P) <= t))
            if good > max(max_good, MODEL_POINTS - 1):
                best, max_good = E, good
                niters = update_num_iters(confidence, (n - good) / n, niters)
        it += 1
        if n == MODEL_POINTS:
            break                     # the same sample again: nothing can change
    if best is None:
        return None, mask, drawn
    return best, sampson_error(best, P) <= t, drawn


# ---------------------------------------------------------------------------- recoverPose

def _sum3(a, b, c):
    return (a + b) + c


def svd3(E):
    """E (9, row-major) -> U (3x3), Vt (3x3): one-sided Jacobi on the rows of At = E^T (the rotation of
    tri_ref.jacobi_null), rows sorted by descending norm; U's columns 0, 1 are the normalised rows of At, column 2
    their cross product (E has rank 2)."""
    At = [[E[3 * k + i] for k in range(3)] for i in range(3)]
    V = [[1.0 if i == k else 0.0 for k in range(3)] for i in range(3)]
    W = [_sum3(*[At[i][k] * At[i][k] for k in range(3)]) for i in range(3)]
    eps = float(EPS)
    for _ in range(MAX_SWEEPS):
        changed = False
        for i, j in ((0, 1), (0, 2), (1, 2)):
            p = _sum3(*[At[i][k] * At[j][k] for k in range(3)])
            if abs(p) <= eps * math.sqrt(W[i] * W[j]):
                continue
            p = 2.0 * p
            beta = W[i] - W[j]
            gamma = math.sqrt(p * p + beta * beta)
            if beta < 0:
                s = math.sqrt(((gamma - beta) * 0.5) / gamma)
                c = p / (gamma * s * 2.0)
            else:
                c = math.sqrt((gamma + beta) / (gamma * 2.0))
                s = p / (gamma * c * 2.0)
            for M in (At, V):
                for k in range(3):
                    t0 = c * M[i][k] + s * M[j][k]
                    t1 = c * M[j][k] - s * M[i][k]
                    M[i][k], M[j][k] = t0, t1
            W[i] = _sum3(*[v * v for v in At[i]])
            W[j] = _sum3(*[v * v for v in At[j]])
            changed = True
        if not changed:
            break
    W = [math.sqrt(_sum3(*[v * v for v in At[i]])) for i in range(3)]
    for i in range(2):                      # selection sort, descending
        j = i
        for k in range(i + 1, 3):
            if W[j] < W[k]:
                j = k
        if j != i:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            V[i], V[j] = V[j], V[i]
    u0 = [_div(v, W[0]) for v in At[0]]
    u1 = [_div(v, W[1]) for v in At[1]]
    u2 = [u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]]
    U = [[u0[r], u1[r], u2[r]] for r in range(3)]
    return U, V


def _det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])) \
        + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])


def decompose(E):
    """cv::decomposeEssentialMat: -> R1, R2 (3x3 lists), t (3)."""
    U, Vt = svd3(E)
    if _det3(U) < 0:
        U = [[-v for v in r] for r in U]
    if _det3(Vt) < 0:
        Vt = [[-v for v in r] for r in Vt]
    R1 = [[((-U[r][1]) * Vt[0][c] + U[r][0] * Vt[1][c]) + U[r][2] * Vt[2][c] for c in range(3)] for r in range(3)]
    R2 = [[(U[r][1] * Vt[0][c] + (-U[r][0]) * Vt[1][c]) + U[r][2] * Vt[2][c] for c in range(3)] for r in range(3)]
    return R1, R2, [U[0][2], U[1][2], U[2][2]]


def candidates(E):
    """The four [R|t] of recoverPose, 12 floats each: [R1|t], [R2|t], [R1|-t], [R2|-t]."""
    R1, R2, t = decompose(E)
    out = []
    for R, s in ((R1, 1.0), (R2, 1.0), (R1, -1.0), (R2, -1.0)):
        out.append([v for r in range(3) for v in (R[r][0], R[r][1], R[r][2], t[r] if s > 0 else -t[r])])
    return out


P0 = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


@np.errstate(all="ignore")
def cheirality(P1, x1, y1, x2, y2):
    """triangulatePoints([I|0], P1) on float64 points (f5's DLT without the float rounding) and recoverPose's
    four tests -> bool mask."""
    h, _ = jacobi_null(dlt_matrix(P0, P1, x1, y1, x2, y2))
    P1 = [F64(v) for v in P1]
    m = (h[:, 2] * h[:, 3]) > 0
    X, Y, Z = h[:, 0] / h[:, 3], h[:, 1] / h[:, 3], h[:, 2] / h[:, 3]
    m &= Z < DISTANCE_THRESH
    Z2 = ((P1[8] * X + P1[9] * Y) + P1[10] * Z) + P1[11]
    m &= Z2 > 0
    m &= Z2 < DISTANCE_THRESH
    return m


def choose(g):
    """recoverPose's >= cascade over the four counts -> the candidate's index."""
    if g[0] >= g[1] and g[0] >= g[2] and g[0] >= g[3]:
        return 0
    if g[1] >= g[0] and g[1] >= g[2] and g[1] >= g[3]:
        return 1
    if g[2] >= g[0] and g[2] >= g[1] and g[2] >= g[3]:
        return 2
    return 3


def recover_pose(E, l, r, camL, mask):
    """l, r: raw (n x 2) float32 keypoints, both normalised with the LEFT camera matrix (as the reference passes
    them).  -> (pose 12 floats, mask after the cheirality tests, the four counts)."""
    with np.errstate(all="ignore"):
        x1 = (l[:, 0].astype(F64) - camL["cx"]) / camL["fx"]
        y1 = (l[:, 1].astype(F64) - camL["cy"]) / camL["fy"]
        x2 = (r[:, 0].astype(F64) - camL["cx"]) / camL["fx"]
        y2 = (r[:, 1].astype(F64) - camL["cy"]) / camL["fy"]
    cands = candidates(E)
    masks = [cheirality(P, x1, y1, x2, y2) & mask for P in cands]
    good = [int(np.count_nonzero(m)) for m in masks]
    w = choose(good)
    return cands[w], masks[w], good


# ---------------------------------------------------------------------------- the call

def pixel_threshold(threshold, size_l, size_r):
    """SfM.cpp:515-521: < 0 pixels, > 0 a fraction of max(leftW, leftH, rightH, rightH) (never the right width)."""
    if threshold < 0:
        return -float(threshold)
    return float(max(size_l[0], size_l[1], size_r[1], size_r[1])) * float(threshold)


@np.errstate(all="ignore")
def prepare(l, r, camL, camR):
    """The two-camera findEssentialMat overload up to the RANSAC's points.
    -> (P (n x 4) float64, the mean focal length (fx + fy) / 2)."""
    fx, fy = (camL["fx"] + camR["fx"]) * F64(0.5), (camL["fy"] + camR["fy"]) * F64(0.5)
    cx, cy = (camL["cx"] + camR["cx"]) * F64(0.5), (camL["cy"] + camR["cy"]) * F64(0.5)
    cols = []
    for pt, cam in ((l, camL), (r, camR)):
        x, y = undistort(pt, cam)
        u = (fx * x.astype(F64) + cx).astype(F32)
        v = (fy * y.astype(F64) + cy).astype(F32)
        cols += [(u.astype(F64) - cx) / fx, (v.astype(F64) - cy) / fy]
    return np.stack(cols, axis=1), (fx + fy) / F64(2.0)


def pose_pair(l, r, camL, camR, thr_px, confidence=CONFIDENCE, max_iters=MAX_ITERS):
    """findCameraPoseFromMatch on one pair's aligned keypoints.
    -> dict(status, E (9), pose (12), mask, n_ransac, n_inliers, counts, drawn)."""
    n = len(l)
    nan9, nan12 = np.full(9, np.nan), np.full(12, np.nan)
    fail = dict(status=0, E=nan9, pose=nan12, mask=np.zeros(n, bool), n_ransac=0, n_inliers=0, counts=None, drawn=[])
    if n < MODEL_POINTS:
        return fail
    P, f = prepare(l, r, camL, camR)
    E, mask, drawn = ransac(P, float(F64(thr_px) / f), confidence, max_iters)
    fail["drawn"] = drawn
    if E is None:
        return fail
    pose, m2, counts = recover_pose(E, l, r, camL, mask)
    return dict(status=1, E=np.array(E), pose=np.array(pose), mask=m2, n_ransac=int(np.count_nonzero(mask)),
                n_inliers=int(np.count_nonzero(m2)), counts=counts, drawn=drawn)


def relative_poses(keypoints, cameras, shot_camera, shot_size, pairs, matches, offsets, threshold=-1.0,
                   confidence=CONFIDENCE, max_iters=MAX_ITERS):
    """The whole call of sfmx_relative_poses: dict of the ABI's output arrays."""
    kps = [np.ascontiguousarray(k, F32).reshape(-1, 2) for k in keypoints]
    cams = [cam_params(K, d) for K, d in cameras]
    size = np.asarray(shot_size, np.int32).reshape(-1, 2)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    off = np.asarray(offsets, np.int64)
    n, npair = int(off[-1]), len(pairs)
    out = dict(status=np.zeros(npair, np.int32), E=np.full((npair, 9), np.nan), pose=np.full((npair, 12), np.nan),
               mask=np.zeros(n, np.uint8), n_ransac_inliers=np.zeros(npair, np.int32),
               n_inliers=np.zeros(npair, np.int32))
    for p, (L, R) in enumerate(pairs):
        a, b = int(off[p]), int(off[p + 1])
        if b == a:
            continue
        q, t = matches["queryIdx"][a:b], matches["trainIdx"][a:b]
        if q.min() < 0 or q.max() >= len(kps[L]) or t.min() < 0 or t.max() >= len(kps[R]):
            raise ValueError("match index outside its image's keypoints")
        res = pose_pair(kps[L][q], kps[R][t], cams[shot_camera[L]], cams[shot_camera[R]],
                        pixel_threshold(threshold, size[L], size[R]), confidence, max_iters)
        out["status"][p] = res["status"]
        out["E"][p], out["pose"][p] = res["E"], res["pose"]
        out["mask"][a:b] = res["mask"]
        out["n_ransac_inliers"][p], out["n_inliers"][p] = res["n_ransac"], res["n_inliers"]
    keep = out["mask"].astype(bool)
    ck = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    out["matches"] = matches[keep]
    out["pair_offsets"] = ck[off]
    out["E"] = np.where(np.isnan(out["E"]), F64(np.nan), out["E"])
    out["pose"] = np.where(np.isnan(out["pose"]), F64(np.nan), out["pose"])
    return out
