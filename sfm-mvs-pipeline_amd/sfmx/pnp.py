"""Registration pose of a new shot — host mirror of
``SfM::findCameraPoseFrom3d2dMatch`` (src/photogrammetrie/sfm/SfM.cpp:453-489), the
row between the 3D-2D search and the relative poses of a registered shot.  All
arithmetic runs in the HIP kernels behind ``sfmx_register_poses`` and
``sfmx_distinct_3d2d_points`` (include/sfmx_pnp.h); this module only marshals
buffers.

Every call poses any number of candidate sets: ``cv::solvePnPRansac`` (EPnP RANSAC,
the ``solvePnP(ITERATIVE)`` refit on the inliers) and the inlier ratio SfM.cpp:311
tests.  P3P for exactly 4 points is not built (status 2).  The threshold is the reference's
``ransacReprojectionPoseThreshold`` (``sfmx_cli_config.ransac_pose_threshold``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, check, sfmx_tri_camera

CONFIDENCE = 0.99    # solvePnPRansac's default
MAX_ITERS = 100      # iterationsCount
THRESHOLD = -8.0     # -Pransac-pose-threshold's default


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _small_arrays(set_shot, cameras, shot_camera, shot_size):
    """The arrays that are host memory in every call: set_shot, cameras, shot_camera, sizes."""
    cams = (sfmx_tri_camera * max(len(cameras), 1))()
    for c, (K, dist) in zip(cams, cameras):
        c.K[:] = np.asarray(K, np.float64).reshape(9).tolist()
        c.dist[:] = np.asarray(dist, np.float64).reshape(5).tolist()
    sc = _i32(shot_camera).reshape(-1)
    size = _i32(shot_size).reshape(-1, 2)
    if len(sc) != len(size):
        raise ValueError("shot_camera and shot_size must have one entry per shot")
    return _i32(set_shot).reshape(-1), cams, sc, size


def register_poses(points3d, points2d, set_offsets, set_shot, cameras, shot_camera, shot_size,
                   threshold: float = THRESHOLD, confidence: float = CONFIDENCE, max_iters: int = MAX_ITERS,
                   device: int = 0, stream: int = 0) -> dict:
    """points3d (n x 3) / points2d (n x 2) float64: the packed candidate sets, set s = [set_offsets[s],
    set_offsets[s + 1]); set_shot[s]: the shot it would register; cameras: [(K 3x3, dist k1 k2 p1 p2 k3)];
    shot_camera[i]: camera of shot i; shot_size: n_shots x (width, height).
    -> dict(status, pose (n_sets x 12, after the refit), ransac_pose (n_sets x 12, the best EPnP model), mask (n),
    n_inliers, inlier_ratio, refit_start (0 DLT, 1 the EPnP model, -1 no refit))."""
    p3 = np.ascontiguousarray(points3d, np.float64).reshape(-1, 3)
    p2 = np.ascontiguousarray(points2d, np.float64).reshape(-1, 2)
    off = np.ascontiguousarray(set_offsets, np.int64).reshape(-1)
    ss, cams, sc, size = _small_arrays(set_shot, cameras, shot_camera, shot_size)
    if len(off) != len(ss) + 1:
        raise ValueError("set_offsets must have n_sets + 1 entries")
    n, ns = len(p3), len(ss)
    if len(p2) != n or int(off[-1]) != n:
        raise ValueError("set_offsets must end at the number of points, one 2-D point per 3-D point")
    status = np.zeros(max(ns, 1), np.int32)
    final = np.zeros((max(ns, 1), 12))
    pose = np.zeros((max(ns, 1), 12))
    mask = np.zeros(max(n, 1), np.uint8)
    ni = np.zeros(max(ns, 1), np.int32)
    ratio = np.zeros(max(ns, 1))
    start = np.zeros(max(ns, 1), np.int32)
    check(lib.sfmx_register_poses(p3.ctypes.data if n else None, p2.ctypes.data if n else None, off.ctypes.data,
                                  _p(ss, C.c_int32), ns, cams, len(cameras), _p(sc, C.c_int32), _p(size, C.c_int32),
                                  len(sc), float(threshold), float(confidence), int(max_iters), 0, int(device),
                                  stream or None, status.ctypes.data, final.ctypes.data, pose.ctypes.data,
                                  mask.ctypes.data, ni.ctypes.data, ratio.ctypes.data, start.ctypes.data),
          "sfmx_register_poses")
    return dict(status=status[:ns], pose=final[:ns], ransac_pose=pose[:ns], mask=mask[:n], n_inliers=ni[:ns],
                inlier_ratio=ratio[:ns], refit_start=start[:ns])


def register_poses_device(points3d_ptr: int, points2d_ptr: int, set_offsets_ptr: int, n_points: int, set_shot,
                          cameras, shot_camera, shot_size, threshold: float = THRESHOLD,
                          confidence: float = CONFIDENCE, max_iters: int = MAX_ITERS, device: int = 0,
                          stream: int = 0) -> dict:
    """Same, with the points and offsets already resident on `device` (torch tensors' data_ptr(), the outputs
    of distinct_3d2d_points_device); n_points = set_offsets[n_sets].  The outputs are torch tensors on `device`."""
    import torch
    ss, cams, sc, size = _small_arrays(set_shot, cameras, shot_camera, shot_size)
    ns = len(ss)
    dev = torch.device("cuda", int(device))
    status = torch.zeros(max(ns, 1), dtype=torch.int32, device=dev)
    pose = torch.empty((max(ns, 1), 12), dtype=torch.float64, device=dev)
    final = torch.empty((max(ns, 1), 12), dtype=torch.float64, device=dev)
    start = torch.zeros(max(ns, 1), dtype=torch.int32, device=dev)
    mask = torch.zeros(max(int(n_points), 1), dtype=torch.uint8, device=dev)
    ni = torch.zeros(max(ns, 1), dtype=torch.int32, device=dev)
    ratio = torch.zeros(max(ns, 1), dtype=torch.float64, device=dev)
    if not stream:
        torch.cuda.synchronize(dev)   # the tensors above were made on torch's stream, the call runs on the default one
    check(lib.sfmx_register_poses(points3d_ptr or None, points2d_ptr or None, set_offsets_ptr, _p(ss, C.c_int32), ns,
                                  cams, len(cameras), _p(sc, C.c_int32), _p(size, C.c_int32), len(sc), float(threshold),
                                  float(confidence), int(max_iters), 1, int(device), stream or None, status.data_ptr(),
                                  final.data_ptr(), pose.data_ptr(), mask.data_ptr(), ni.data_ptr(), ratio.data_ptr(),
                                  start.data_ptr()), "sfmx_register_poses")
    return dict(status=status[:ns], pose=final[:ns], ransac_pose=pose[:ns], mask=mask[:int(n_points)],
                n_inliers=ni[:ns], inlier_ratio=ratio[:ns], refit_start=start[:ns])


def distinct_3d2d_points(cloud_xyz, origin_offsets, found_keypoint, found_xy, device: int = 0, stream: int = 0):
    """ShotMatches3d2d::getDistinct3d2dPoints on find_3d2d_matches' per-origin-record output
    (found_keypoint, found_xy) -> (points3d (n x 3), points2d (n x 2)) float64, first-appearance order."""
    xyz = np.ascontiguousarray(cloud_xyz, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(origin_offsets, np.int64).reshape(-1)
    kp = _i32(found_keypoint).reshape(-1)
    xy = np.ascontiguousarray(found_xy, np.float32).reshape(-1, 2)
    if len(off) != len(xyz) + 1:
        raise ValueError("origin_offsets must have n_points + 1 entries")
    nr = len(kp)
    if len(xy) != nr or int(off[-1]) != nr:
        raise ValueError("origin_offsets must end at the number of records, one found_xy per record")
    o3 = np.zeros((max(nr, 1), 3))
    o2 = np.zeros((max(nr, 1), 2))
    cnt = C.c_int64(0)
    check(lib.sfmx_distinct_3d2d_points(xyz.ctypes.data if len(xyz) else None, len(xyz), off.ctypes.data,
                                        kp.ctypes.data if nr else None, xy.ctypes.data if nr else None, 0, int(device),
                                        stream or None, o3.ctypes.data, o2.ctypes.data, C.byref(cnt)),
          "sfmx_distinct_3d2d_points")
    return o3[:cnt.value].copy(), o2[:cnt.value].copy()


def distinct_3d2d_points_device(cloud_xyz_ptr: int, n_points: int, origin_offsets_ptr: int, found_keypoint_ptr: int,
                                found_xy_ptr: int, n_records: int, device: int = 0, stream: int = 0):
    """Same on device pointers; n_records = origin_offsets[n_points].  -> (points3d, points2d) torch tensors on
    `device`, views of buffers of n_records capacity."""
    import torch
    dev = torch.device("cuda", int(device))
    o3 = torch.empty((max(int(n_records), 1), 3), dtype=torch.float64, device=dev)
    o2 = torch.empty((max(int(n_records), 1), 2), dtype=torch.float64, device=dev)
    cnt = C.c_int64(0)
    if not stream:
        torch.cuda.synchronize(dev)
    check(lib.sfmx_distinct_3d2d_points(cloud_xyz_ptr or None, int(n_points), origin_offsets_ptr, found_keypoint_ptr or None,
                                        found_xy_ptr or None, 1, int(device), stream or None, o3.data_ptr(),
                                        o2.data_ptr(), C.byref(cnt)), "sfmx_distinct_3d2d_points")
    return o3[:cnt.value], o2[:cnt.value]


def last_kernel_ms() -> float:
    return float(lib.sfmx_register_poses_last_kernel_ms())


def distinct_last_kernel_ms() -> float:
    return float(lib.sfmx_distinct_3d2d_last_kernel_ms())


def findCameraPoseFrom3d2dMatch(points3d, points2d, camera, image_size, threshold: float = THRESHOLD):
    """SfM::findCameraPoseFrom3d2dMatch (SfM.cpp:453-489) for one shot's distinct 3D-2D points; camera = (K, dist) of the shot, image_size = (width, height), threshold =
    ransacReprojectionPoseThreshold.  -> (pose 3x4 [R|t] after the refit, the inlier ratio SfM.cpp:311 tests).  Raises RuntimeError where the reference throws cv::Exception (fewer than 4 points, no model) and
    NotImplementedError for exactly 4 points (P3P is the host's)."""
    p3 = np.ascontiguousarray(points3d, np.float64).reshape(-1, 3)
    r = register_poses(p3, points2d, np.array([0, len(p3)], np.int64), [0], [camera], [0], [image_size], threshold)
    st = int(r["status"][0])
    if st == 2:
        raise NotImplementedError("findCameraPoseFrom3d2dMatch: exactly 4 points need P3P, which is not built")
    if st != 1:
        raise RuntimeError("findCameraPoseFrom3d2dMatch: no pose for this shot (cv::Exception in the reference)")
    return r["pose"][0].reshape(3, 4).copy(), float(r["inlier_ratio"][0])
