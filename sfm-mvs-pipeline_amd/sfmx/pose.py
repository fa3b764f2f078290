"""Relative pose of shot matches — host mirror of ``SfM::findCameraPoseFromMatch``
(src/photogrammetrie/sfm/SfM.cpp:491-540), the row between the homography ratio
and the triangulation of a posed pair.  All arithmetic runs in the HIP kernels
behind ``sfmx_relative_poses`` (include/sfmx_pose.h); this module only marshals
buffers.

Every call poses all pairs of a packed match graph: ``cv::findEssentialMat``
(RANSAC), ``cv::recoverPose`` and the reduction of each DMatch list to the
inliers that survive both.  ``matches`` / ``pair_offsets`` of the result are the
lists ``setMatches`` installs (SfM.cpp:213,350) and go into
``triangulate_matches`` unchanged.  The threshold is the reference's
``ransacReprojectionBaselineThreshold`` (``sfmx_cli_config.ransac_baseline_threshold``).
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from ._lib import lib, check, sfmx_tri_camera
from .matching import DMATCH_DTYPE, Scene, ShotMatches

CONFIDENCE = 0.999   # SfM.cpp:524
MAX_ITERS = 1000     # RANSACPointSetRegistrator's default


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _small_arrays(cameras, shot_camera, shot_size, pairs, n_shots):
    """The arrays that are host memory in every call: cameras, shot_camera, sizes, pairs."""
    cams = (sfmx_tri_camera * max(len(cameras), 1))()
    for c, (K, dist) in zip(cams, cameras):
        c.K[:] = np.asarray(K, np.float64).reshape(9).tolist()
        c.dist[:] = np.asarray(dist, np.float64).reshape(5).tolist()
    sc = _i32(shot_camera).reshape(-1)
    size = _i32(shot_size).reshape(-1, 2)
    if len(sc) != n_shots or len(size) != n_shots:
        raise ValueError("shot_camera and shot_size must have one entry per shot")
    return cams, sc, size, _i32(pairs).reshape(-1, 2)


def relative_poses(keypoints: Sequence[np.ndarray], cameras, shot_camera, shot_size, pairs: np.ndarray,
                   matches: np.ndarray, offsets: np.ndarray, threshold: float = -1.0, confidence: float = CONFIDENCE,
                   max_iters: int = MAX_ITERS, device: int = 0, stream: int = 0) -> dict:
    """keypoints[i]: (n_i x 2) float32; cameras: [(K 3x3, dist k1 k2 p1 p2 k3)]; shot_camera[i]: camera of shot
    i; shot_size: n_shots x (width, height); matches / offsets: packed DMatch lists as BFMatcher.fetch returns
    them.  -> dict(status, E (n_pairs x 9), pose (n_pairs x 12), mask (n_matches), n_ransac_inliers, n_inliers,
    matches (the inlier DMatches), pair_offsets)."""
    kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    nkp = _i32([len(k) for k in kps])
    cams, sc, size, pairs = _small_arrays(cameras, shot_camera, shot_size, pairs, len(kps))
    m = np.ascontiguousarray(matches, DMATCH_DTYPE)
    off = np.ascontiguousarray(offsets, np.int64)
    if len(off) != len(pairs) + 1:
        raise ValueError("offsets must have n_pairs + 1 entries")
    n, npair = len(m), len(pairs)
    if int(off[-1]) != n:
        raise ValueError("offsets must end at the number of matches")
    ptrs = (C.c_void_p * max(len(kps), 1))(*[k.ctypes.data for k in kps])
    status = np.zeros(max(npair, 1), np.int32)
    E = np.zeros((max(npair, 1), 9))
    pose = np.zeros((max(npair, 1), 12))
    mask = np.zeros(max(n, 1), np.uint8)
    nr = np.zeros(max(npair, 1), np.int32)
    ni = np.zeros(max(npair, 1), np.int32)
    om = np.zeros(max(n, 1), DMATCH_DTYPE)
    po = np.zeros(npair + 1, np.int64)
    check(lib.sfmx_relative_poses(ptrs, _p(nkp, C.c_int32), len(kps), cams, len(cameras), _p(sc, C.c_int32),
                                  _p(size, C.c_int32), _p(pairs, C.c_int32), npair, m.ctypes.data if n else None,
                                  off.ctypes.data, float(threshold), float(confidence), int(max_iters), 0, int(device),
                                  stream or None, status.ctypes.data, E.ctypes.data, pose.ctypes.data, mask.ctypes.data,
                                  nr.ctypes.data, ni.ctypes.data, om.ctypes.data, po.ctypes.data),
          "sfmx_relative_poses")
    return dict(status=status[:npair], E=E[:npair], pose=pose[:npair], mask=mask[:n], n_ransac_inliers=nr[:npair],
                n_inliers=ni[:npair], matches=om[:int(po[-1])], pair_offsets=po)


def relative_poses_device(keypoint_ptrs: Sequence[int], n_keypoints, cameras, shot_camera, shot_size,
                          pairs: np.ndarray, matches_ptr: int, offsets_ptr: int, n_matches: int,
                          threshold: float = -1.0, confidence: float = CONFIDENCE, max_iters: int = MAX_ITERS,
                          device: int = 0, stream: int = 0) -> dict:
    """Same, with keypoints and match lists already resident on `device` (torch tensors' data_ptr(),
    sfmx_matcher_device_results); n_matches = offsets[n_pairs].  The outputs are torch tensors on `device`;
    `matches` is a uint8 tensor of 16-byte DMatch records (a view of a buffer of n_matches capacity) whose
    data_ptr(), with pair_offsets.data_ptr(), goes into triangulate_matches_device."""
    import torch
    nkp = _i32(n_keypoints)
    cams, sc, size, pairs = _small_arrays(cameras, shot_camera, shot_size, pairs, len(nkp))
    ptrs = (C.c_void_p * max(len(nkp), 1))(*keypoint_ptrs)
    n, npair = max(int(n_matches), 1), max(len(pairs), 1)
    dev = torch.device("cuda", int(device))
    status = torch.zeros(npair, dtype=torch.int32, device=dev)
    E = torch.empty((npair, 9), dtype=torch.float64, device=dev)
    pose = torch.empty((npair, 12), dtype=torch.float64, device=dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    nr = torch.zeros(npair, dtype=torch.int32, device=dev)
    ni = torch.zeros(npair, dtype=torch.int32, device=dev)
    om = torch.empty((n, DMATCH_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    po = torch.zeros(len(pairs) + 1, dtype=torch.int64, device=dev)
    if not stream:
        torch.cuda.synchronize(dev)   # the tensors above were made on torch's stream, the call runs on the default one
    check(lib.sfmx_relative_poses(ptrs, _p(nkp, C.c_int32), len(nkp), cams, len(cameras), _p(sc, C.c_int32),
                                  _p(size, C.c_int32), _p(pairs, C.c_int32), len(pairs), matches_ptr or None,
                                  offsets_ptr, float(threshold), float(confidence), int(max_iters), 1, int(device),
                                  stream or None, status.data_ptr(), E.data_ptr(), pose.data_ptr(), mask.data_ptr(),
                                  nr.data_ptr(), ni.data_ptr(), om.data_ptr(), po.data_ptr()),
          "sfmx_relative_poses")
    k = len(pairs)
    return dict(status=status[:k], E=E[:k], pose=pose[:k], mask=mask[:int(n_matches)], n_ransac_inliers=nr[:k],
                n_inliers=ni[:k], matches=om, pair_offsets=po)


def last_kernel_ms() -> float:
    return float(lib.sfmx_relative_poses_last_kernel_ms())


def findCameraPoseFromMatch(scene: Scene, shot_matches: ShotMatches, threshold: float = -1.0, cameras=None):
    """SfM::findCameraPoseFromMatch (SfM.cpp:491-540) for one ShotMatches; threshold =
    ransacReprojectionBaselineThreshold.  cameras[i] = (K, dist) of scene shot i (CameraShot::getCamera); without
    it every shot must carry a `camera` attribute of that form.  -> (pose 3x4 [R|t], the inlier DMatches: what
    the caller passes to setMatches).  Raises RuntimeError where the reference throws cv::Exception (fewer than
    5 matches, no model)."""
    shots = scene.getShots()
    if cameras is None:
        cameras = [getattr(sh, "camera", None) for sh in shots]
        if any(c is None for c in cameras):
            raise ValueError("findCameraPoseFromMatch: pass cameras or give every shot a camera = (K, dist)")
    m = np.asarray(shot_matches.getMatches(), DMATCH_DTYPE)
    r = relative_poses([sh.keypoints for sh in shots], list(cameras), np.arange(len(shots), dtype=np.int32),
                       [sh.getImageSize() for sh in shots], np.array([[shot_matches.left, shot_matches.right]], np.int32),
                       m, np.array([0, len(m)], np.int64), threshold)
    if int(r["status"][0]) != 1:
        raise RuntimeError("findCameraPoseFromMatch: no pose for this pair (cv::Exception in the reference)")
    return r["pose"][0].reshape(3, 4).copy(), r["matches"].copy()
