"""numpy restatement of SfM::triangulateMatch (SfM.cpp:383-451) — the specification
csrc/triangulate.hip is held to, bit for bit (triangulation section).

Every step is one correctly rounded IEEE + - * / sqrt on float64 (float32 where
a float rounding is named), elementwise over the matches of a pair; nothing
comes from libm.  Expressions are written with the same association as the
kernel's.  OpenCV 4.5.1 semantics of undistortPoints (5 iterations),
triangulatePoints (one-sided Jacobi SVD, hypot restated as sqrt(p*p + b*b)),
convertPointsFromHomogeneous and projectPoints.
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS = F64(10.0) * np.finfo(np.float64).eps     # 10 * DBL_EPSILON
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
MAX_SWEEPS = 30
MAX_REPROJECTION_ERROR = 10.0                   # SfM.h:55


def cam_params(K, dist):
    K = np.asarray(K, F64).reshape(9)
    d = np.asarray(dist, F64).reshape(5)
    return dict(fx=K[0], fy=K[4], cx=K[2], cy=K[5], k1=d[0], k2=d[1], p1=d[2], p2=d[3], k3=d[4])


def undistort(pt, cam):
    """cv::undistortPoints(pts, K, dist), TermCriteria(COUNT, 5): (n x 2) float32 -> two float32 arrays."""
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
    return x.astype(F32), y.astype(F32)


def _sum4(a, b, c, d):
    return ((a + b) + c) + d


@np.errstate(all="ignore")
def jacobi_null(A):
    """A: (n, 4, 4) float64 -> (row 3 of V after the descending sort as (n, 4) float64, sweeps per system)."""
    n = A.shape[0]
    At = [[A[:, k, i].copy() for k in range(4)] for i in range(4)]     # rows of At = columns of A
    V = [[np.full(n, 1.0 if i == k else 0.0) for k in range(4)] for i in range(4)]
    W = [_sum4(*[At[i][k] * At[i][k] for k in range(4)]) for i in range(4)]
    sweeps = np.zeros(n, np.int32)
    live = np.ones(n, bool)
    for _ in range(MAX_SWEEPS):
        changed = np.zeros(n, bool)
        for i, j in PAIRS:
            p = _sum4(*[At[i][k] * At[j][k] for k in range(4)])
            rot = live & ~(np.abs(p) <= EPS * np.sqrt(W[i] * W[j]))
            p = F64(2.0) * p
            beta = W[i] - W[j]
            gamma = np.sqrt(p * p + beta * beta)
            s_n = np.sqrt(((gamma - beta) * F64(0.5)) / gamma)
            c_n = p / (gamma * s_n * F64(2.0))
            c_p = np.sqrt((gamma + beta) / (gamma * F64(2.0)))
            s_p = p / (gamma * c_p * F64(2.0))
            neg = beta < 0
            c = np.where(neg, c_n, c_p)
            s = np.where(neg, s_n, s_p)
            t0s, t1s = [], []
            for k in range(4):
                t0 = c * At[i][k] + s * At[j][k]
                t1 = c * At[j][k] - s * At[i][k]          # == -s*ai + c*aj
                t0s.append(t0)
                t1s.append(t1)
                At[i][k] = np.where(rot, t0, At[i][k])
                At[j][k] = np.where(rot, t1, At[j][k])
            W[i] = np.where(rot, _sum4(*[t * t for t in t0s]), W[i])
            W[j] = np.where(rot, _sum4(*[t * t for t in t1s]), W[j])
            for k in range(4):
                t0 = c * V[i][k] + s * V[j][k]
                t1 = c * V[j][k] - s * V[i][k]
                V[i][k] = np.where(rot, t0, V[i][k])
                V[j][k] = np.where(rot, t1, V[j][k])
            changed |= rot
        sweeps += live
        live = live & changed
        if not live.any():
            break
    W = [np.sqrt(_sum4(*[At[i][k] * At[i][k] for k in range(4)])) for i in range(4)]
    idx = [np.full(n, i, np.int32) for i in range(4)]
    for i in range(3):                                   # selection sort, descending, on (W, row index)
        j = np.full(n, i, np.int32)
        wj = W[i]
        for k in range(i + 1, 4):
            lt = wj < W[k]
            j = np.where(lt, k, j)
            wj = np.where(lt, W[k], wj)
        for m in range(i + 1, 4):
            sw = j == m
            W[i], W[m] = np.where(sw, W[m], W[i]), np.where(sw, W[i], W[m])
            idx[i], idx[m] = np.where(sw, idx[m], idx[i]), np.where(sw, idx[i], idx[m])
    r = idx[3]
    out = np.stack([np.where(r == 0, V[0][k], np.where(r == 1, V[1][k], np.where(r == 2, V[2][k], V[3][k])))
                    for k in range(4)], axis=1)
    return out, sweeps


def dlt_matrix(PL, PR, xl, yl, xr, yr):
    """The 4x4 system of cv::triangulatePoints: two rows per view, x * P[2] - P[0], y * P[2] - P[1]."""
    n = len(xl)
    A = np.empty((n, 4, 4))
    for v, (P, x, y) in enumerate(((PL, xl, yl), (PR, xr, yr))):
        P = np.asarray(P, F64).reshape(3, 4)
        x, y = x.astype(F64), y.astype(F64)
        for k in range(4):
            A[:, 2 * v, k] = x * P[2, k] - P[0, k]
            A[:, 2 * v + 1, k] = y * P[2, k] - P[1, k]
    return A


@np.errstate(all="ignore")
def from_homogeneous(h):
    """convertPointsFromHomogeneous on float32 (n x 4): scale = W != 0 ? 1/W : 1."""
    h = h.astype(F32)
    w = h[:, 3]
    scale = np.where(w != 0, F32(1.0) / w, F32(1.0)).astype(F32)
    return h[:, 0] * scale, h[:, 1] * scale, h[:, 2] * scale


def project(X, Y, Z, P, cam):
    """cv::projectPoints with R, t of the 3x4 pose: float32 coordinates -> float32 pixel coordinates."""
    P = np.asarray(P, F64).reshape(3, 4)
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    k1, k2, p1, p2, k3 = cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"]
    X, Y, Z = X.astype(F64), Y.astype(F64), Z.astype(F64)
    x = P[0, 0] * X + P[0, 1] * Y + P[0, 2] * Z + P[0, 3]
    y = P[1, 0] * X + P[1, 1] * Y + P[1, 2] * Z + P[1, 3]
    z = P[2, 0] * X + P[2, 1] * Y + P[2, 2] * Z + P[2, 3]
    z = np.where(z != 0, F64(1.0) / z, F64(1.0))
    x = x * z
    y = y * z
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    a1 = F64(2.0) * x * y
    a2 = r2 + F64(2.0) * x * x
    a3 = r2 + F64(2.0) * y * y
    cdist = F64(1.0) + k1 * r2 + k2 * r4 + k3 * r6
    xd = x * cdist + p1 * a1 + p2 * a2
    yd = y * cdist + p1 * a3 + p2 * a1
    u = xd * fx + cx
    v = yd * fy + cy
    return u.astype(F32), v.astype(F32)


def reprojection_error(u, v, pt):
    du = (u - pt[:, 0]).astype(F32)
    dv = (v - pt[:, 1]).astype(F32)
    du, dv = du.astype(F64), dv.astype(F64)
    return np.sqrt(du * du + dv * dv)


def _canon32(a):
    return np.where(np.isnan(a), F32(np.nan), a).astype(F32)     # the canonical quiet NaN 0x7FC00000


def _canon64(a):
    return np.where(np.isnan(a), F64(np.nan), a).astype(F64)     # 0x7FF8000000000000


def triangulate_pair(l, r, PL, PR, camL, camR):
    """l, r: aligned (n x 2) float32 keypoints -> X, Y, Z float32, eL, eR float64, sweeps."""
    with np.errstate(all="ignore"):
        xl, yl = undistort(l, camL)
        xr, yr = undistort(r, camR)
        h, sweeps = jacobi_null(dlt_matrix(PL, PR, xl, yl, xr, yr))
        X, Y, Z = from_homogeneous(h)
        eL = reprojection_error(*project(X, Y, Z, PL, camL), l)
        eR = reprojection_error(*project(X, Y, Z, PR, camR), r)
    return _canon32(X), _canon32(Y), _canon32(Z), _canon64(eL), _canon64(eR), sweeps


def triangulate_matches(keypoints, cameras, shot_camera, shot_pose, pairs, matches, offsets,
                        max_reprojection_error=MAX_REPROJECTION_ERROR):
    """The whole call of sfmx_triangulate_matches: dict of the ABI's output arrays (+ per-match xyz32, sweeps)."""
    kps = [np.ascontiguousarray(k, F32).reshape(-1, 2) for k in keypoints]
    cams = [cam_params(K, d) for K, d in cameras]
    poses = np.asarray(shot_pose, F64).reshape(-1, 12)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    off = np.asarray(offsets, np.int64)
    n = int(off[-1]) if len(off) else 0
    xyz32 = np.zeros((n, 3), F32)
    err = np.zeros((n, 2), F64)
    sweeps = np.zeros(n, np.int32)
    keep = np.zeros(n, bool)
    shots = np.zeros((n, 2), np.int32)
    oxy = np.zeros((n, 4), F64)
    for p, (L, R) in enumerate(pairs):
        a, b = int(off[p]), int(off[p + 1])
        if b == a:
            continue
        q, t = matches["queryIdx"][a:b], matches["trainIdx"][a:b]
        if q.min() < 0 or q.max() >= len(kps[L]) or t.min() < 0 or t.max() >= len(kps[R]):
            raise ValueError("match index outside its image's keypoints")
        l, r = kps[L][q], kps[R][t]
        X, Y, Z, eL, eR, sw = triangulate_pair(l, r, poses[L], poses[R], cams[shot_camera[L]], cams[shot_camera[R]])
        xyz32[a:b] = np.stack([X, Y, Z], axis=1)
        err[a:b, 0], err[a:b, 1] = eL, eR
        sweeps[a:b] = sw
        keep[a:b] = ~((eL > max_reprojection_error) | (eR > max_reprojection_error))
        shots[a:b] = (L, R)
        oxy[a:b, :2], oxy[a:b, 2:] = l.astype(F64), r.astype(F64)
    ck = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    sel = np.flatnonzero(keep).astype(np.int64)
    n_points = len(sel)
    return dict(point_offsets=ck[off] if len(off) else np.zeros(1, np.int64), xyz=xyz32[sel].astype(F64),
                match=sel, origin_shot=shots[sel].reshape(-1), origin_xy=oxy[sel].reshape(-1, 2), err=err,
                n_points=n_points, origin_offsets=2 * np.arange(n_points + 1, dtype=np.int64), xyz32=xyz32,
                sweeps=sweeps)
