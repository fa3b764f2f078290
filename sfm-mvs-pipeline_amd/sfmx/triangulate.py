"""Triangulation of shot matches into 3D points — host mirror of
``SfM::triangulateMatch`` (src/photogrammetrie/sfm/SfM.cpp:383-451), the row
between the match graph and the 3D-2D search / bundle adjustment.  All
arithmetic runs in the HIP kernels behind ``sfmx_triangulate_matches``
(include/sfmx_triangulate.h); this module only marshals buffers.

Every call returns the points pair-major in ``pairs`` order and match-list
order within a pair, each with one origin of two records (left, right):
``origin_offsets`` / ``origin_shot`` / ``origin_xy`` are the origin CSR of
``sfmx.scene`` and go into ``find_3d2d_matches`` and
``ba_observations_from_origins`` unchanged.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from ._lib import lib, check, sfmx_tri_camera
from .matching import DMATCH_DTYPE, Scene, ShotMatches

MAX_REPROJECTION_ERROR = 10.0   # SfM.h:55


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _small_arrays(cameras, shot_camera, shot_pose, pairs, n_shots):
    """The arrays that are host memory in every call: cameras, shot_camera, poses, pairs."""
    cams = (sfmx_tri_camera * max(len(cameras), 1))()
    for c, (K, dist) in zip(cams, cameras):
        c.K[:] = np.asarray(K, np.float64).reshape(9).tolist()
        c.dist[:] = np.asarray(dist, np.float64).reshape(5).tolist()
    sc = _i32(shot_camera).reshape(-1)
    pose = np.ascontiguousarray(shot_pose, np.float64).reshape(-1, 12)
    if len(sc) != n_shots or len(pose) != n_shots:
        raise ValueError("shot_camera and shot_pose must have one entry per shot")
    return cams, sc, pose, _i32(pairs).reshape(-1, 2)


def triangulate_matches(keypoints: Sequence[np.ndarray], cameras, shot_camera, shot_pose, pairs: np.ndarray,
                        matches: np.ndarray, offsets: np.ndarray,
                        max_reprojection_error: float = MAX_REPROJECTION_ERROR, device: int = 0, stream: int = 0) -> dict:
    """keypoints[i]: (n_i x 2) float32; cameras: [(K 3x3, dist k1 k2 p1 p2 k3)]; shot_camera[i]: camera of
    shot i; shot_pose: n_shots x 3x4 [R|t]; matches / offsets: packed DMatch lists as BFMatcher.fetch
    returns them.  -> dict(n_points, point_offsets, xyz (n x 3), match, origin_offsets, origin_shot,
    origin_xy (2n x 2), err (n_matches x 2: left, right error of every match))."""
    kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    nkp = _i32([len(k) for k in kps])
    cams, sc, pose, pairs = _small_arrays(cameras, shot_camera, shot_pose, pairs, len(kps))
    m = np.ascontiguousarray(matches, DMATCH_DTYPE)
    off = np.ascontiguousarray(offsets, np.int64)
    if len(off) != len(pairs) + 1:
        raise ValueError("offsets must have n_pairs + 1 entries")
    n = len(m)
    if int(off[-1]) != n:
        raise ValueError("offsets must end at the number of matches")
    ptrs = (C.c_void_p * max(len(kps), 1))(*[k.ctypes.data for k in kps])
    po = np.zeros(len(pairs) + 1, np.int64)
    xyz = np.zeros((max(n, 1), 3))
    om = np.zeros(max(n, 1), np.int64)
    osh = np.zeros(2 * max(n, 1), np.int32)
    oxy = np.zeros((2 * max(n, 1), 2))
    err = np.zeros((max(n, 1), 2))
    npts = C.c_int64(0)
    check(lib.sfmx_triangulate_matches(ptrs, _p(nkp, C.c_int32), len(kps), cams, len(cameras), _p(sc, C.c_int32),
                                       _p(pose, C.c_double), _p(pairs, C.c_int32), len(pairs),
                                       m.ctypes.data if n else None, off.ctypes.data, float(max_reprojection_error), 0,
                                       int(device), stream or None, po.ctypes.data, xyz.ctypes.data, om.ctypes.data,
                                       osh.ctypes.data, oxy.ctypes.data, err.ctypes.data, C.byref(npts)),
          "sfmx_triangulate_matches")
    k = int(npts.value)
    return dict(n_points=k, point_offsets=po, xyz=xyz[:k], match=om[:k],
                origin_offsets=2 * np.arange(k + 1, dtype=np.int64), origin_shot=osh[:2 * k], origin_xy=oxy[:2 * k],
                err=err[:n])


def triangulate_matches_device(keypoint_ptrs: Sequence[int], n_keypoints, cameras, shot_camera, shot_pose,
                               pairs: np.ndarray, matches_ptr: int, offsets_ptr: int, n_matches: int,
                               max_reprojection_error: float = MAX_REPROJECTION_ERROR, with_err: bool = False,
                               device: int = 0, stream: int = 0) -> dict:
    """Same, with keypoints and match lists already resident on `device` (torch tensors' data_ptr(),
    sfmx_matcher_device_results); n_matches = offsets[n_pairs].  The outputs are torch tensors on
    `device` (views of buffers of n_matches capacity); `err` only with with_err."""
    import torch
    nkp = _i32(n_keypoints)
    cams, sc, pose, pairs = _small_arrays(cameras, shot_camera, shot_pose, pairs, len(nkp))
    ptrs = (C.c_void_p * max(len(nkp), 1))(*keypoint_ptrs)
    n = max(int(n_matches), 1)
    dev = torch.device("cuda", int(device))
    po = torch.zeros(len(pairs) + 1, dtype=torch.int64, device=dev)
    xyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
    om = torch.empty(n, dtype=torch.int64, device=dev)
    osh = torch.empty(2 * n, dtype=torch.int32, device=dev)
    oxy = torch.empty((2 * n, 2), dtype=torch.float64, device=dev)
    err = torch.empty((n, 2), dtype=torch.float64, device=dev) if with_err else None
    if not stream:
        torch.cuda.synchronize(dev)   # the tensors above were made on torch's stream, the call runs on the default one
    npts = C.c_int64(0)
    check(lib.sfmx_triangulate_matches(ptrs, _p(nkp, C.c_int32), len(nkp), cams, len(cameras), _p(sc, C.c_int32),
                                       _p(pose, C.c_double), _p(pairs, C.c_int32), len(pairs), matches_ptr or None,
                                       offsets_ptr, float(max_reprojection_error), 1, int(device), stream or None,
                                       po.data_ptr(), xyz.data_ptr(), om.data_ptr(), osh.data_ptr(), oxy.data_ptr(),
                                       err.data_ptr() if with_err else None, C.byref(npts)),
          "sfmx_triangulate_matches")
    k = int(npts.value)
    out = dict(n_points=k, point_offsets=po, xyz=xyz[:k], match=om[:k],
               origin_offsets=2 * torch.arange(k + 1, dtype=torch.int64, device=dev), origin_shot=osh[:2 * k],
               origin_xy=oxy[:2 * k])
    if with_err:
        out["err"] = err[:int(n_matches)]
    return out


def last_kernel_ms() -> float:
    return float(lib.sfmx_triangulate_last_kernel_ms())


def triangulateMatch(scene: Scene, shot_match, cameras, poses,
                     maxReprojectionError: float = MAX_REPROJECTION_ERROR) -> dict:
    """SfM::triangulateMatch (SfM.cpp:383-451) for one ShotMatches (or a list of them, triangulated in one
    call): cameras[i] = (K, dist) and poses[i] = 3x4 [R|t] of scene shot i (CameraShot::getCamera /
    getPose).  -> the dict of triangulate_matches; its points are the PointcloudElements the reference
    appends, in its order."""
    sms = [shot_match] if isinstance(shot_match, ShotMatches) else list(shot_match)
    shots = scene.getShots()
    pairs = np.array([[s.left, s.right] for s in sms], np.int32).reshape(-1, 2)
    counts = np.array([len(s.getMatches()) for s in sms], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    m = np.concatenate([np.asarray(s.getMatches(), DMATCH_DTYPE) for s in sms]) if off[-1] else np.zeros(0, DMATCH_DTYPE)
    return triangulate_matches([sh.keypoints for sh in shots], list(cameras), np.arange(len(shots), dtype=np.int32),
                               poses, pairs, m, off, maxReprojectionError)
