"""Scene bookkeeping around bundle adjustment — host
mirror over include/sfmx_scene.h:

* ``find_3d2d_matches``: ``Scene::find3d2dMatches`` (common/Scene.cpp:369-424),
  a GPU hash join (csrc/scene.hip) instead of the reference's nested scans;
* ``ba_observations_from_origins``: the Ceres problem's observation arrays
  (BundleAdjustment.cpp:50-91), O(n) native host code.

Point-cloud origins are flattened per point (PointcloudElement::getOriginPoints,
Scene.cpp:162-185): ``origin_offsets[n_points+1]``, ``origin_shot``,
``origin_xy`` (n x 2 float64, cv::Point2d).
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from ._lib import lib, check
from .matching import DMATCH_DTYPE


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def find_3d2d_matches(keypoints: Sequence[np.ndarray], pairs, matches, offsets, origin_offsets, origin_shot,
                      origin_xy, shot: int, device: int = 0, stream: int = 0):
    """-> (keypoint index in `shot` per origin record or -1, pair index or -1,
    matched keypoint positions n x 2 float32 (NaN where none))."""
    kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    nkp = np.array([len(k) for k in kps], np.int32)
    ptrs = (C.c_void_p * max(len(kps), 1))(*[k.ctypes.data for k in kps])
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = np.ascontiguousarray(matches, DMATCH_DTYPE)
    off = np.ascontiguousarray(offsets, np.int64)
    oo = np.ascontiguousarray(origin_offsets, np.int64)
    os_ = np.ascontiguousarray(origin_shot, np.int32)
    oxy = np.ascontiguousarray(origin_xy, np.float64).reshape(-1, 2)
    n = int(oo[-1])
    okp = np.zeros(max(n, 1), np.int32)
    opr = np.zeros(max(n, 1), np.int32)
    oxy_out = np.zeros((max(n, 1), 2), np.float32)
    check(lib.sfmx_find_3d2d_matches(ptrs, _p(nkp, C.c_int32), len(kps), _p(pairs, C.c_int32), len(pairs),
                                     m.ctypes.data if len(m) else None, off.ctypes.data, oo.ctypes.data, len(oo) - 1,
                                     os_.ctypes.data if n else None, oxy.ctypes.data if n else None, int(shot), 0,
                                     int(device), stream or None, okp.ctypes.data, opr.ctypes.data, oxy_out.ctypes.data),
          "sfmx_find_3d2d_matches")
    return okp[:n], opr[:n], oxy_out[:n]


def find_3d2d_matches_device(keypoint_ptrs, n_keypoints, pairs, matches_ptr, offsets_ptr, origin_offsets_ptr,
                             n_points, origin_shot_ptr, origin_xy_ptr, shot, out_kp_ptr, out_pair_ptr, out_xy_ptr=0,
                             device: int = 0, stream: int = 0):
    """Same with every array resident on `device` (pairs stays host)."""
    nkp = np.ascontiguousarray(n_keypoints, np.int32)
    ptrs = (C.c_void_p * max(len(nkp), 1))(*keypoint_ptrs)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    check(lib.sfmx_find_3d2d_matches(ptrs, _p(nkp, C.c_int32), len(nkp), _p(pairs, C.c_int32), len(pairs), matches_ptr,
                                     offsets_ptr, origin_offsets_ptr, int(n_points), origin_shot_ptr, origin_xy_ptr,
                                     int(shot), 1, int(device), stream or None, out_kp_ptr, out_pair_ptr,
                                     out_xy_ptr or None), "sfmx_find_3d2d_matches")


def last_kernel_ms() -> float:
    return float(lib.sfmx_find_3d2d_last_kernel_ms())


def count_3d2d_matches(keypoints: Sequence[np.ndarray], pairs, matches, offsets, origin_offsets, origin_shot,
                       origin_xy, candidates, pair_active=None, device: int = 0, stream: int = 0) -> np.ndarray:
    """The candidate ranking of SfM::triangulate (SfM.cpp:276-300) in one call: -> int32 per candidate shot,
    the number of origin records ``find_3d2d_matches(shot=candidate)`` matches over the pairs that
    `pair_active` (None: all) leaves visible."""
    kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    nkp = np.array([len(k) for k in kps], np.int32)
    ptrs = (C.c_void_p * max(len(kps), 1))(*[k.ctypes.data for k in kps])
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    act = None if pair_active is None else np.ascontiguousarray(pair_active, np.int32)
    if act is not None and len(act) != len(pairs):
        raise ValueError("pair_active must have one entry per pair")
    m = np.ascontiguousarray(matches, DMATCH_DTYPE)
    off = np.ascontiguousarray(offsets, np.int64)
    if len(off) != len(pairs) + 1:
        raise ValueError("offsets must have n_pairs + 1 entries")
    oo = np.ascontiguousarray(origin_offsets, np.int64)
    os_ = np.ascontiguousarray(origin_shot, np.int32)
    oxy = np.ascontiguousarray(origin_xy, np.float64).reshape(-1, 2)
    cand = np.ascontiguousarray(candidates, np.int32).reshape(-1)
    if len(oo) < 1 or len(os_) != len(oxy) or int(oo[-1]) > len(os_):
        raise ValueError("origin arrays shorter than their offsets")
    n = int(oo[-1])
    out = np.zeros(max(len(cand), 1), np.int32)
    check(lib.sfmx_count_3d2d_matches(ptrs, _p(nkp, C.c_int32), len(kps), _p(pairs, C.c_int32), len(pairs),
                                      None if act is None else _p(act, C.c_int32), m.ctypes.data if len(m) else None,
                                      off.ctypes.data, oo.ctypes.data, len(oo) - 1, os_.ctypes.data if n > 0 else None,
                                      oxy.ctypes.data if n > 0 else None, _p(cand, C.c_int32), len(cand), 0, int(device),
                                      stream or None, out.ctypes.data), "sfmx_count_3d2d_matches")
    return out[:len(cand)]


def count_3d2d_matches_device(keypoint_ptrs, n_keypoints, pairs, matches_ptr, offsets_ptr, origin_offsets_ptr, n_points,
                              origin_shot_ptr, origin_xy_ptr, candidates, out_count_ptr, pair_active=None,
                              device: int = 0, stream: int = 0):
    """Same with every array resident on `device` (pairs, pair_active and candidates stay host)."""
    nkp = np.ascontiguousarray(n_keypoints, np.int32)
    ptrs = (C.c_void_p * max(len(nkp), 1))(*keypoint_ptrs)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    act = None if pair_active is None else np.ascontiguousarray(pair_active, np.int32)
    if act is not None and len(act) != len(pairs):
        raise ValueError("pair_active must have one entry per pair")
    cand = np.ascontiguousarray(candidates, np.int32).reshape(-1)
    check(lib.sfmx_count_3d2d_matches(ptrs, _p(nkp, C.c_int32), len(nkp), _p(pairs, C.c_int32), len(pairs),
                                      None if act is None else _p(act, C.c_int32), matches_ptr or None, offsets_ptr,
                                      origin_offsets_ptr, int(n_points), origin_shot_ptr or None, origin_xy_ptr or None,
                                      _p(cand, C.c_int32), len(cand), 1, int(device), stream or None,
                                      out_count_ptr or None), "sfmx_count_3d2d_matches")


def count_last_kernel_ms() -> float:
    return float(lib.sfmx_count_3d2d_last_kernel_ms())


def ba_observations_from_origins(origin_offsets, origin_shot, origin_xy, n_shots: int):
    """-> dict(obs_point, obs_cam, obs_xy, pose_of_shot, shot_of_pose): the
    sfmx_ba_problem observation arrays in AddResidualBlock order
    (BundleAdjustment.cpp:50-91), poses in first-appearance order."""
    oo = np.ascontiguousarray(origin_offsets, np.int64)
    os_ = np.ascontiguousarray(origin_shot, np.int32)
    oxy = np.ascontiguousarray(origin_xy, np.float64).reshape(-1, 2)
    n = int(oo[-1])
    op = np.zeros(max(n, 1), np.int32)
    oc = np.zeros(max(n, 1), np.int32)
    ox = np.zeros((max(n, 1), 2))
    pos = np.zeros(max(n_shots, 1), np.int32)
    sop = np.zeros(max(n_shots, 1), np.int32)
    npose = C.c_int32(0)
    check(lib.sfmx_ba_observations_from_origins(_p(oo, C.c_int64), len(oo) - 1, _p(os_, C.c_int32),
                                                _p(oxy, C.c_double), int(n_shots), _p(op, C.c_int32), _p(oc, C.c_int32),
                                                _p(ox, C.c_double), _p(pos, C.c_int32), _p(sop, C.c_int32),
                                                C.byref(npose)), "sfmx_ba_observations_from_origins")
    return dict(obs_point=op[:n], obs_cam=oc[:n], obs_xy=ox[:n], pose_of_shot=pos[:n_shots],
                shot_of_pose=sop[:npose.value])


POINT_MERGE_DISTANCE = 0.01     # SfM.h:56
FEATURE_MERGE_DISTANCE = 20.0   # SfM.h:57


def merge_pointcloud_3d2d(keypoints: Sequence[np.ndarray], pairs, matches, offsets, cloud_xyz, cloud_origin_offsets,
                          cloud_origin_shot, cloud_origin_xy, new_xyz, new_origin_offsets, new_origin_shot,
                          new_origin_xy, point_merge_distance: float = POINT_MERGE_DISTANCE,
                          feature_merge_distance: float = FEATURE_MERGE_DISTANCE, device: int = 0, stream: int = 0) -> dict:
    """The merge loop of SfM.cpp:354-363 (Scene::mergePointcloudElement3d2d, common/Scene.cpp:470-567):
    the new elements (an origin CSR, e.g. triangulate_matches' output) are folded into the cloud in index
    order.  -> dict(xyz (n x 3), origin_offsets, origin_shot, origin_xy: the merged cloud, again an origin
    CSR; target: cloud index each element ended in; merge_distance: distance to the point it was merged
    into, -1.0 if it was appended)."""
    kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    nkp = np.array([len(k) for k in kps], np.int32)
    ptrs = (C.c_void_p * max(len(kps), 1))(*[k.ctypes.data for k in kps])
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = np.ascontiguousarray(matches, DMATCH_DTYPE)
    off = np.ascontiguousarray(offsets, np.int64)
    if len(off) != len(pairs) + 1:
        raise ValueError("offsets must have n_pairs + 1 entries")
    if len(m) != (int(off[-1]) if len(off) else 0):
        raise ValueError("offsets must end at the number of matches")
    cx = np.ascontiguousarray(cloud_xyz, np.float64).reshape(-1, 3)
    co = np.ascontiguousarray(cloud_origin_offsets, np.int64)
    cs = np.ascontiguousarray(cloud_origin_shot, np.int32)
    cxy = np.ascontiguousarray(cloud_origin_xy, np.float64).reshape(-1, 2)
    nx = np.ascontiguousarray(new_xyz, np.float64).reshape(-1, 3)
    no = np.ascontiguousarray(new_origin_offsets, np.int64)
    ns = np.ascontiguousarray(new_origin_shot, np.int32)
    nxy = np.ascontiguousarray(new_origin_xy, np.float64).reshape(-1, 2)
    if len(co) != len(cx) + 1 or len(no) != len(nx) + 1:
        raise ValueError("origin offsets must have one entry per point plus one")
    if len(cs) != len(cxy) or len(ns) != len(nxy) or int(co[-1]) > len(cs) or int(no[-1]) > len(ns):
        raise ValueError("origin arrays shorter than their offsets")
    n_pts, n_rec = len(cx) + len(nx), len(cs) + len(ns)
    tgt = np.zeros(max(len(nx), 1), np.int32)
    dist = np.zeros(max(len(nx), 1))
    oxyz = np.zeros((max(n_pts, 1), 3))
    ooff = np.zeros(n_pts + 1, np.int64)
    oshot = np.zeros(max(n_rec, 1), np.int32)
    oxy = np.zeros((max(n_rec, 1), 2))
    k, r = C.c_int32(0), C.c_int64(0)
    check(lib.sfmx_merge_pointcloud_3d2d(ptrs, _p(nkp, C.c_int32), len(kps), _p(pairs, C.c_int32), len(pairs),
                                         m.ctypes.data if len(m) else None, off.ctypes.data,
                                         cx.ctypes.data if len(cx) else None, len(cx), co.ctypes.data,
                                         cs.ctypes.data if len(cs) else None, cxy.ctypes.data if len(cs) else None,
                                         nx.ctypes.data if len(nx) else None, len(nx), no.ctypes.data,
                                         ns.ctypes.data if len(ns) else None, nxy.ctypes.data if len(ns) else None,
                                         float(point_merge_distance), float(feature_merge_distance), 0, int(device),
                                         stream or None, tgt.ctypes.data, dist.ctypes.data, oxyz.ctypes.data,
                                         ooff.ctypes.data, oshot.ctypes.data, oxy.ctypes.data, C.byref(k), C.byref(r)),
          "sfmx_merge_pointcloud_3d2d")
    k, r = int(k.value), int(r.value)
    return dict(xyz=oxyz[:k], origin_offsets=ooff[:k + 1], origin_shot=oshot[:r], origin_xy=oxy[:r],
                target=tgt[:len(nx)], merge_distance=dist[:len(nx)])


def merge_pointcloud_3d2d_device(keypoint_ptrs, n_keypoints, pairs, matches_ptr, offsets_ptr, cloud_xyz, cloud_origin_offsets,
                                 cloud_origin_shot, cloud_origin_xy, new_xyz, new_origin_offsets, new_origin_shot,
                                 new_origin_xy, point_merge_distance: float = POINT_MERGE_DISTANCE,
                                 feature_merge_distance: float = FEATURE_MERGE_DISTANCE, device: int = 0,
                                 stream: int = 0) -> dict:
    """Same with keypoints and match lists resident on `device` (their data_ptr()s; pairs stays host) and
    both clouds as contiguous torch tensors on `device` (xyz n x 3 float64, origin_offsets int64,
    origin_shot int32, origin_xy n x 2 float64).  The outputs are torch tensors on `device`."""
    import torch
    nkp = np.ascontiguousarray(n_keypoints, np.int32)
    ptrs = (C.c_void_p * max(len(nkp), 1))(*keypoint_ptrs)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    dev = torch.device("cuda", int(device))
    for t, dt in ((cloud_xyz, torch.float64), (cloud_origin_offsets, torch.int64), (cloud_origin_shot, torch.int32),
                  (cloud_origin_xy, torch.float64), (new_xyz, torch.float64), (new_origin_offsets, torch.int64),
                  (new_origin_shot, torch.int32), (new_origin_xy, torch.float64)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError("cloud tensors must be contiguous, on the device and of the documented dtypes")
    n_cloud, n_new = len(cloud_origin_offsets) - 1, len(new_origin_offsets) - 1
    if cloud_xyz.numel() != 3 * n_cloud or new_xyz.numel() != 3 * n_new:
        raise ValueError("origin offsets must have one entry per point plus one")
    n_pts, n_rec = n_cloud + n_new, len(cloud_origin_shot) + len(new_origin_shot)
    tgt = torch.zeros(max(n_new, 1), dtype=torch.int32, device=dev)
    dist = torch.zeros(max(n_new, 1), dtype=torch.float64, device=dev)
    oxyz = torch.empty((max(n_pts, 1), 3), dtype=torch.float64, device=dev)
    ooff = torch.zeros(n_pts + 1, dtype=torch.int64, device=dev)
    oshot = torch.empty(max(n_rec, 1), dtype=torch.int32, device=dev)
    oxy = torch.empty((max(n_rec, 1), 2), dtype=torch.float64, device=dev)
    if not stream:
        torch.cuda.synchronize(dev)   # the tensors above were made on torch's stream, the call runs on the default one
    k, r = C.c_int32(0), C.c_int64(0)
    check(lib.sfmx_merge_pointcloud_3d2d(ptrs, _p(nkp, C.c_int32), len(nkp), _p(pairs, C.c_int32), len(pairs),
                                         matches_ptr or None, offsets_ptr, cloud_xyz.data_ptr() or None, n_cloud,
                                         cloud_origin_offsets.data_ptr(), cloud_origin_shot.data_ptr() or None,
                                         cloud_origin_xy.data_ptr() or None, new_xyz.data_ptr() or None, n_new,
                                         new_origin_offsets.data_ptr(), new_origin_shot.data_ptr() or None,
                                         new_origin_xy.data_ptr() or None, float(point_merge_distance),
                                         float(feature_merge_distance), 1, int(device), stream or None, tgt.data_ptr(),
                                         dist.data_ptr(), oxyz.data_ptr(), ooff.data_ptr(), oshot.data_ptr(), oxy.data_ptr(),
                                         C.byref(k), C.byref(r)), "sfmx_merge_pointcloud_3d2d")
    k, r = int(k.value), int(r.value)
    return dict(xyz=oxyz[:k], origin_offsets=ooff[:k + 1], origin_shot=oshot[:r], origin_xy=oxy[:r],
                target=tgt[:n_new], merge_distance=dist[:n_new])


def merge_last_kernel_ms() -> float:
    return float(lib.sfmx_merge_pointcloud_last_kernel_ms())


def merge_last_stats() -> dict:
    """Counts of the last merge call on this thread: merges whose winner qualifies through a record it held
    at call start (static), merges whose winner qualifies only through a record or point added during the
    call (dynamic), links among the new elements."""
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(lib.sfmx_merge_pointcloud_last_stats(C.byref(a), C.byref(b), C.byref(c)), "sfmx_merge_pointcloud_last_stats")
    return dict(merged_static=int(a.value), merged_dynamic=int(b.value), links=int(c.value))


def merge_set_max_rounds(max_rounds: int) -> None:
    """The cap on the device resolution's rounds for this thread's merge calls: 0 the library default, > 0 that
    cap, < 0 always the host resolution.  A call that reaches the cap finishes on the host, with the same result."""
    check(lib.sfmx_merge_pointcloud_set_max_rounds(int(max_rounds)), "sfmx_merge_pointcloud_set_max_rounds")


def merge_last_path() -> dict:
    """How the last merge call on this thread ran: resolve rounds launched, whether the host resolution decided
    the result, and every byte the call copied between host and device."""
    a, b, c = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    check(lib.sfmx_merge_pointcloud_last_path(C.byref(a), C.byref(b), C.byref(c)), "sfmx_merge_pointcloud_last_path")
    return dict(rounds=int(a.value), host_fallback=int(b.value), host_bytes=int(c.value))
