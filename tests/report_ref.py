"""numpy restatement of the scene outputs (include/sfmx_report.h), shared by the report tests.

The reprojection error is SceneUtils.cpp:43-62 operation by operation: the point rounded to float32, the
projection of tests/tri_ref.py (float64, u and v rounded to float32), then the difference and the norm in
float64.  The colour rule is Scene::colorizePointcloud twice: the literal shot-major loop and the per-point
reduction the kernel computes.  Statistics and histogram are tests/cloud_ref.py's; the four writers return the
files' bytes.  Correctly rounded operations only; nothing here calls the library.
"""
import numpy as np

import cloud_ref
import tri_ref

F32, F64 = np.float32, np.float64


def point_of_record(origin_offsets):
    off = np.asarray(origin_offsets, np.int64)
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))


def reprojection_errors(xyz, origin_offsets, origin_shot, origin_xy, cameras, shot_camera, shot_pose):
    """-> float64 (n_origins), record order; a NaN is the canonical quiet NaN."""
    x = np.asarray(xyz, F64).reshape(-1, 3)
    osh = np.asarray(origin_shot, np.int64).reshape(-1)
    q = np.asarray(origin_xy, F64).reshape(-1, 2)
    pose = np.asarray(shot_pose, F64).reshape(-1, 12)
    pt = point_of_record(origin_offsets)
    err = np.zeros(len(osh), F64)
    with np.errstate(all="ignore"):
        X = x.astype(F32)                                     # cv::Point3f(getCoordinates())
        for s in np.unique(osh):
            i = np.flatnonzero(osh == s)
            K, dist = cameras[int(shot_camera[s])]
            u, v = tri_ref.project(X[pt[i], 0], X[pt[i], 1], X[pt[i], 2], pose[s], tri_ref.cam_params(K, dist))
            du = q[i, 0] - u.astype(F64)                      # point2d - cv::Point2d(point2dReprojected)
            dv = q[i, 1] - v.astype(F64)
            err[i] = np.sqrt(du * du + dv * dv)
    return np.where(np.isnan(err), F64(np.nan), err).astype(F64)


def reprojection_errors_f64(xyz, origin_offsets, origin_shot, origin_xy, cameras, shot_camera, shot_pose):
    """The anchor: a plain float64 pinhole-plus-distortion projection with no float rounding of u, v.
    -> (error, |u| + |v|)."""
    x = np.asarray(xyz, F64).reshape(-1, 3)
    osh = np.asarray(origin_shot, np.int64).reshape(-1)
    q = np.asarray(origin_xy, F64).reshape(-1, 2)
    pt = point_of_record(origin_offsets)
    P = np.asarray(shot_pose, F64).reshape(-1, 3, 4)[osh]
    cam = np.array([[K[0][0], K[1][1], K[0][2], K[1][2], *dist] for K, dist in
                    [(np.asarray(K, F64).reshape(3, 3), np.asarray(d, F64).reshape(5)) for K, d in cameras]])
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam[np.asarray(shot_camera, np.int64)[osh]].T
    Xc = np.einsum("nij,nj->ni", P[:, :, :3], x[pt]) + P[:, :, 3]
    a, b = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = a * a + b * b
    cd = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    u = (a * cd + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)) * fx + cx
    v = (b * cd + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b) * fy + cy
    return np.hypot(q[:, 0] - u, q[:, 1] - v), np.abs(u) + np.abs(v)


# ---- colours -----------------------------------------------------------------------------------------------

def pixel_position(x, y):
    """image.at<Vec3b>(Point2d): saturate_cast<int> = cvRound, round half to even.  None: not finite."""
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    return int(np.rint(F64(x))), int(np.rint(F64(y)))


def _pixel(image, x, y, default):
    p = pixel_position(x, y)
    h, w = image.shape[:2]
    if p is None or not (0 <= p[0] < w and 0 <= p[1] < h):
        return tuple(default)                                 # the reference reads out of bounds
    b, g, r = image[p[1], p[0]]
    return int(r), int(g), int(b)


def colorize_literal(n_points, origin_offsets, origin_shot, origin_xy, images, default=(0, 0, 0)):
    """Scene.cpp:580-616 as written: shots in scene order, every still-uncoloured point, its first origin in
    the shot.  -> (rgb (n x 3) uint8, record (n) int64)."""
    off = np.asarray(origin_offsets, np.int64)
    osh = np.asarray(origin_shot, np.int64).reshape(-1)
    q = np.asarray(origin_xy, F64).reshape(-1, 2)
    rgb = np.zeros((n_points, 3), np.uint8)
    rec = np.full(n_points, -1, np.int64)
    for s, image in enumerate(images):
        for p in range(n_points):
            if rec[p] >= 0:
                continue
            hit = [i for i in range(off[p], off[p + 1]) if osh[i] == s]
            if not hit:
                continue
            rec[p] = hit[0]
            rgb[p] = _pixel(image, q[hit[0], 0], q[hit[0], 1], default)
    rgb[rec < 0] = default
    return rgb, rec


def colorize(n_points, origin_offsets, origin_shot, origin_xy, images, default=(0, 0, 0)):
    """The reduction: the record with the lowest shot index, the first such in CSR order."""
    off = np.asarray(origin_offsets, np.int64)
    osh = np.asarray(origin_shot, np.int64).reshape(-1)
    q = np.asarray(origin_xy, F64).reshape(-1, 2)
    rgb = np.zeros((n_points, 3), np.uint8)
    rec = np.full(n_points, -1, np.int64)
    for p in range(n_points):
        sh = osh[off[p]:off[p + 1]]
        if len(sh) == 0:
            rgb[p] = default
            continue
        i = int(off[p] + np.argmin(sh))                       # argmin: the first of equal minima
        rec[p] = i
        rgb[p] = _pixel(images[int(osh[i])], q[i, 0], q[i, 1], default)
    return rgb, rec


# ---- statistics and files ----------------------------------------------------------------------------------

def error_statistics(errors):
    """MathUtils::calculateStatistics as SceneUtils.cpp:71-73 calls it.  NaN errors stand behind the ordered
    ones (np.sort's order); min and max are std::min / std::max folds from 0, which pass a NaN over; the
    sums run over the whole list."""
    e = np.asarray(errors, F64).reshape(-1)
    with np.errstate(all="ignore"):
        s = cloud_ref.statistics(e)
    ok = e[~np.isnan(e)]
    s["min"] = float(min(0.0, ok.min())) if len(ok) else 0.0
    s["max"] = float(max(0.0, ok.max())) if len(ok) else 0.0
    return s


def error_histogram(errors):
    with np.errstate(all="ignore"):
        return cloud_ref.histogram(np.asarray(errors, F64).reshape(-1), -1.0)


def stats_csv(s):
    head = "N_Points,Max_Error,Min_Error,Avg_Error,Median_Error,Variance_Error,Deviation_Error\n"
    vals = ",".join(cloud_ref.fmt6(s[k]) for k in ("max", "min", "mean", "median", "variance", "deviation"))
    return (head + "%d,%s\n" % (s["n_points"], vals)).encode()


def hist_csv(keys, counts):
    return ("Error,Count\n" + "".join("%s,%d\n" % (cloud_ref.fmt6(k), int(c)) for k, c in zip(keys, counts))).encode()


CLOUD_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def pointcloud_ply(xyz, rgb=None):
    x = np.asarray(xyz, F64).reshape(-1, 3)
    rec = np.zeros(len(x), np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    assert rec.dtype.itemsize == 15
    with np.errstate(all="ignore"):
        rec["p"] = x.astype(F32)
    if rgb is not None:
        rec["c"] = np.asarray(rgb, np.uint8).reshape(-1, 3)
    return (CLOUD_HEADER % len(x)).encode() + rec.tobytes()


CAMERA_HEADER = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nelement edge %d\n"
                 "property int vertex1\nproperty int vertex2\nproperty uchar red\nproperty uchar green\n"
                 "property uchar blue\nend_header\n")


def cameras_ply(cameras, shots, color=None, only_recovered=True):
    """cameras: [(width, height, K)]; shots: [(camera, recovered, pose 3x4)].  PclUtils.cpp:466-590."""
    use = [s for s in shots if s[1] or not only_recovered]
    r, g, b = (255, 255, 0) if color is None else [int(v) for v in color]
    tail = " %d %d %d\n" % (r, g, b)
    out = [CAMERA_HEADER % (5 * len(use) + 4, 8 * len(use) + 3), "0 0 0 0 0 0\n1 0 0 255 0 0\n0 1 0 0 255 0\n0 0 1 0 0 255\n"]
    with np.errstate(all="ignore"):
        for cam, _, pose in use:
            w, h, K = cameras[cam]
            K = np.asarray(K, F64).reshape(9)
            m = np.asarray(pose, F64).reshape(12)
            norm = F64(1.0) / F64(max(int(w), int(h)))
            width, height = F64(int(w)) * norm, F64(int(h)) * norm
            cx, cy = K[2] * norm, K[5] * norm
            focal = (K[0] if K[0] == K[4] else (K[0] + K[4]) / F64(2.0)) * norm
            left, right, top, bottom = -cx, width - cx, -cy, height - cy
            for x, y, z in ((F64(0), F64(0), F64(0)), (left, top, focal), (right, top, focal), (left, bottom, focal),
                            (right, bottom, focal)):
                t = [((m[4 * k] * x + m[4 * k + 1] * y) + m[4 * k + 2] * z) + m[4 * k + 3] for k in range(3)]
                out.append(" ".join(cloud_ref.fmt6(v) for v in t) + tail)
    for i in range(len(use)):
        f = 4 + 5 * i
        tl, tr, bl, br = f + 1, f + 2, f + 3, f + 4
        for a, c in ((f, tl), (f, tr), (f, bl), (f, br), (tl, tr), (tr, br), (br, bl), (bl, tl)):
            out.append("%d %d" % (a, c) + tail)
    out.append("0 1 255 0 0\n0 2 0 255 0\n0 3 0 0 255\n")
    return "".join(out).encode()
