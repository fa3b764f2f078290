"""Scene outputs — host mirror of what ``PhotogrammetrieCli::runSfM`` does after ``reconstructScene``
(src/cli/PhotogrammetrieCli.cpp:115-132): ``Scene::colorizePointcloud`` (common/Scene.cpp:569-617), the two
``PclUtils::writeToPLY`` (util/PclUtils.cpp:401-590) and the reprojection-error CSVs of ``SceneUtils``
(util/SceneUtils.cpp:28-144).  The per-record reprojection error and the per-point colour run in the HIP
kernels behind ``sfmx_reprojection_errors`` / ``sfmx_colorize_pointcloud``; statistics, histogram and the four
writers are the library's C++ host code (include/sfmx_report.h, include/sfmx_cloud.h).  This module only
marshals buffers.

A cloud is its coordinates ``xyz`` (n x 3 float64) and the origin CSR of ``sfmx.scene``
(``origin_offsets`` n + 1 int64, ``origin_shot`` int32, ``origin_xy`` m x 2 float64).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Sequence

import numpy as np

from ._lib import lib, check, sfmx_cloud_stats, sfmx_tri_camera
from . import cloud as _cloud
from .mvs import sfmx_mvs_camera, sfmx_mvs_shot

DEFAULT_COLOR = (0, 0, 0)          # Scene.h:484
CAMERA_COLOR = (255, 255, 0)       # PclUtils.h:125


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _tri_cameras(cameras, shot_camera, shot_pose):
    cams = (sfmx_tri_camera * max(len(cameras), 1))()
    for c, (K, dist) in zip(cams, cameras):
        c.K[:] = np.asarray(K, np.float64).reshape(9).tolist()
        c.dist[:] = np.asarray(dist, np.float64).reshape(5).tolist()
    sc = np.ascontiguousarray(shot_camera, np.int32).reshape(-1)
    pose = np.ascontiguousarray(shot_pose, np.float64).reshape(-1, 12)
    if len(sc) != len(pose):
        raise ValueError("shot_camera and shot_pose must have one entry per shot")
    return cams, sc, pose


def _host_csr(origin_offsets, origin_shot, origin_xy):
    off = np.ascontiguousarray(origin_offsets, np.int64).reshape(-1)
    osh = np.ascontiguousarray(origin_shot, np.int32).reshape(-1)
    oxy = np.ascontiguousarray(origin_xy, np.float64).reshape(-1, 2)
    if len(off) < 1 or len(osh) != len(oxy):
        raise ValueError("origin_offsets needs n_points + 1 entries, origin_shot and origin_xy one per record")
    return off, osh, oxy


def _device_csr(origin_offsets, origin_shot, origin_xy):
    import torch
    for t, dt in ((origin_offsets, torch.int64), (origin_shot, torch.int32), (origin_xy, torch.float64)):
        if not t.is_cuda or t.dtype != dt:
            raise ValueError("device inputs must be int64 / int32 / float64 tensors on a GPU")
    off, osh, oxy = origin_offsets.contiguous().reshape(-1), origin_shot.contiguous().reshape(-1), origin_xy.contiguous().reshape(-1, 2)
    if off.shape[0] < 1 or osh.shape[0] != oxy.shape[0]:
        raise ValueError("origin_offsets needs n_points + 1 entries, origin_shot and origin_xy one per record")
    return off, osh, oxy


def reprojection_errors(xyz, origin_offsets, origin_shot, origin_xy, cameras, shot_camera, shot_pose,
                        device: int = 0, stream: int = 0) -> np.ndarray:
    """cameras: [(K 3x3, dist k1 k2 p1 p2 k3)]; shot_camera[i]: camera of shot i; shot_pose: n_shots x 3x4 [R|t].
    -> the reprojection error of every origin record, in record order (float64)."""
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    off, osh, oxy = _host_csr(origin_offsets, origin_shot, origin_xy)
    if len(off) != len(x) + 1:
        raise ValueError("origin_offsets must have n_points + 1 entries")
    cams, sc, pose = _tri_cameras(cameras, shot_camera, shot_pose)
    m = len(osh)
    err = np.zeros(max(m, 1), np.float64)
    check(lib.sfmx_reprojection_errors(x.ctypes.data if len(x) else None, len(x), off.ctypes.data, osh.ctypes.data if m else None,
                                       oxy.ctypes.data if m else None, m, cams, len(cameras), _p(sc, C.c_int32),
                                       _p(pose, C.c_double), len(sc), 0, int(device), stream or None, err.ctypes.data),
          "sfmx_reprojection_errors")
    return err[:m]


def reprojection_errors_device(xyz, origin_offsets, origin_shot, origin_xy, cameras, shot_camera, shot_pose, stream: int = 0):
    """Same, with the cloud resident on a GPU: float64 / int64 / int32 / float64 tensors.  -> a float64 tensor
    on that device."""
    import torch
    if not xyz.is_cuda or xyz.dtype != torch.float64:
        raise ValueError("xyz must be a float64 tensor on a GPU")
    x = xyz.contiguous().reshape(-1, 3)
    off, osh, oxy = _device_csr(origin_offsets, origin_shot, origin_xy)
    if off.shape[0] != x.shape[0] + 1:
        raise ValueError("origin_offsets must have n_points + 1 entries")
    cams, sc, pose = _tri_cameras(cameras, shot_camera, shot_pose)
    m, dev = osh.shape[0], x.device
    err = torch.empty(max(m, 1), dtype=torch.float64, device=dev)
    if not stream:
        torch.cuda.synchronize(dev)   # the tensors were made on torch's stream, the call runs on the default one
    check(lib.sfmx_reprojection_errors(x.data_ptr() if x.shape[0] else None, x.shape[0], off.data_ptr(),
                                       osh.data_ptr() if m else None, oxy.data_ptr() if m else None, m, cams, len(cameras),
                                       _p(sc, C.c_int32), _p(pose, C.c_double), len(sc), 1, dev.index or 0, stream or None,
                                       err.data_ptr()), "sfmx_reprojection_errors")
    return err[:m]


def reprojection_last_kernel_ms() -> float:
    return float(lib.sfmx_reprojection_last_kernel_ms())


def _default(default_color):
    d = np.asarray(default_color, np.uint8).reshape(-1)[:3].copy()
    if len(d) != 3:
        raise ValueError("a colour has three components")
    return d


def colorize_pointcloud(n_points: int, origin_offsets, origin_shot, origin_xy, images: Sequence[np.ndarray],
                        default_color=DEFAULT_COLOR, device: int = 0, stream: int = 0):
    """images[s]: the 8-bit BGR image of shot s (h x w x 3 uint8, any row stride, unit pixel stride) in host
    memory.  -> (rgb (n x 3) uint8, record (n) int64: the origin record a colour came from, -1 for none)."""
    off, osh, oxy = _host_csr(origin_offsets, origin_shot, origin_xy)
    if len(off) != n_points + 1:
        raise ValueError("origin_offsets must have n_points + 1 entries")
    ims = [np.asarray(im) for im in images]
    for im in ims:
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or (im.size and (im.strides[2] != 1 or im.strides[1] != 3)):
            raise ValueError("h x w x 3 uint8 images with packed pixels expected")
    ns = len(ims)
    ptrs = (C.c_void_p * max(ns, 1))(*[im.ctypes.data for im in ims])
    w = np.array([im.shape[1] for im in ims], np.int32)
    h = np.array([im.shape[0] for im in ims], np.int32)
    pitch = np.array([im.strides[0] if im.shape[0] > 1 else 3 * im.shape[1] for im in ims], np.int64)
    d = _default(default_color)
    m = len(osh)
    rgb = np.zeros((max(n_points, 1), 3), np.uint8)
    rec = np.full(max(n_points, 1), -1, np.int64)
    check(lib.sfmx_colorize_pointcloud(n_points, off.ctypes.data, osh.ctypes.data if m else None, oxy.ctypes.data if m else None,
                                       m, ptrs, _p(w, C.c_int32), _p(h, C.c_int32), _p(pitch, C.c_int64), ns, d.ctypes.data, 0,
                                       int(device), stream or None, rgb.ctypes.data, rec.ctypes.data),
          "sfmx_colorize_pointcloud")
    return rgb[:n_points], rec[:n_points]


def colorize_pointcloud_device(n_points: int, origin_offsets, origin_shot, origin_xy, images, default_color=DEFAULT_COLOR,
                               stream: int = 0):
    """Same, with the CSR and the images (h x w x 3 uint8 tensors, any row stride) resident on one GPU.
    -> (rgb, record) tensors on that device."""
    import torch
    off, osh, oxy = _device_csr(origin_offsets, origin_shot, origin_xy)
    if off.shape[0] != n_points + 1:
        raise ValueError("origin_offsets must have n_points + 1 entries")
    for im in images:
        if not im.is_cuda or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or \
                (im.numel() and (im.stride(2) != 1 or im.stride(1) != 3)):
            raise ValueError("h x w x 3 uint8 GPU tensors with packed pixels expected")
    ns, dev = len(images), off.device
    ptrs = (C.c_void_p * max(ns, 1))(*[im.data_ptr() for im in images])
    w = np.array([im.shape[1] for im in images], np.int32)
    h = np.array([im.shape[0] for im in images], np.int32)
    pitch = np.array([im.stride(0) if im.shape[0] > 1 else 3 * im.shape[1] for im in images], np.int64)
    d = _default(default_color)
    m = osh.shape[0]
    rgb = torch.empty((max(n_points, 1), 3), dtype=torch.uint8, device=dev)
    rec = torch.empty(max(n_points, 1), dtype=torch.int64, device=dev)
    if not stream:
        torch.cuda.synchronize(dev)
    check(lib.sfmx_colorize_pointcloud(n_points, off.data_ptr(), osh.data_ptr() if m else None, oxy.data_ptr() if m else None, m,
                                       ptrs, _p(w, C.c_int32), _p(h, C.c_int32), _p(pitch, C.c_int64), ns, d.ctypes.data, 1,
                                       dev.index or 0, stream or None, rgb.data_ptr(), rec.data_ptr()),
          "sfmx_colorize_pointcloud")
    return rgb[:n_points], rec[:n_points]


def colorize_last_kernel_ms() -> float:
    return float(lib.sfmx_colorize_last_kernel_ms())


def error_statistics(errors) -> dict:
    """MathUtils::calculateStatistics of an error list as SceneUtils.cpp:71-73 calls it (N_Points = len)."""
    return _cloud.statistics(errors)


def error_histogram(errors):
    """SceneUtils.cpp:119-134 with the default resolution (the variance of the list)."""
    return _cloud.neighbor_histogram(errors, -1.0)


def write_reprojection_stats_csv(path, stats: dict) -> None:
    s = sfmx_cloud_stats(*[stats[k] for k in _cloud.STAT_FIELDS])
    check(lib.sfmx_reprojection_write_stats_csv(os.fsencode(path), C.byref(s)), "sfmx_reprojection_write_stats_csv")


def write_reprojection_hist_csv(path, keys, counts) -> None:
    k = np.ascontiguousarray(keys, np.float64).reshape(-1)
    c = np.ascontiguousarray(counts, np.uint64).reshape(-1)
    if len(k) != len(c):
        raise ValueError("keys and counts differ in length")
    check(lib.sfmx_reprojection_write_hist_csv(os.fsencode(path), k.ctypes.data if len(k) else None,
                                               c.ctypes.data if len(c) else None, len(k)), "sfmx_reprojection_write_hist_csv")


def write_pointcloud_ply(path, xyz, rgb=None) -> None:
    """pointcloud_sparse.ply; rgb None: every point 0, 0, 0 (the run without --colored)."""
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    if c is not None and len(c) != len(x):
        raise ValueError("one colour per point expected")
    check(lib.sfmx_write_pointcloud_ply(os.fsencode(path), x.ctypes.data if len(x) else None, len(x),
                                        c.ctypes.data if c is not None and len(c) else None), "sfmx_write_pointcloud_ply")


def write_cameras_ply(path, cameras, shots, color=None, only_recovered: bool = True) -> None:
    """cameras_recovered.ply.  cameras: [(width, height, K 3x3)]; shots: [(camera index, recovered, pose 3x4)];
    color None: 255, 255, 0."""
    cams = (sfmx_mvs_camera * max(len(cameras), 1))()
    for i, (w, h, K) in enumerate(cameras):
        cams[i].width, cams[i].height = int(w), int(h)
        cams[i].K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
    sh = (sfmx_mvs_shot * max(len(shots), 1))()
    for i, s in enumerate(shots):
        sh[i].camera, sh[i].recovered = int(s[0]), int(bool(s[1]))
        sh[i].pose[:] = [float(v) for v in np.asarray(s[2], np.float64).reshape(12)]
        sh[i].image_name = None
    col = None if color is None else _default(color)
    check(lib.sfmx_write_cameras_ply(os.fsencode(path), C.cast(cams, C.c_void_p), len(cameras), C.cast(sh, C.c_void_p), len(shots),
                                     col.ctypes.data if col is not None else None, int(bool(only_recovered))),
          "sfmx_write_cameras_ply")


# ---- mirrors named after the reference functions ----------------------------------------------------------


def writeToReprojectionErrorStatisticsCSV(errors, outPath) -> None:
    """SceneUtils::writeToReprojectionErrorStatisticsCSV (SceneUtils.cpp:28-80) from the error list of
    reprojection_errors."""
    e = np.asarray(errors.cpu() if hasattr(errors, "cpu") else errors, np.float64)
    write_reprojection_stats_csv(outPath, error_statistics(e))


def writeToReprojectionErrorHistogramCSV(errors, outPath) -> None:
    """SceneUtils::writeToReprojectionErrorHistogramCSV (SceneUtils.cpp:82-144), resolution = -1."""
    e = np.asarray(errors.cpu() if hasattr(errors, "cpu") else errors, np.float64)
    write_reprojection_hist_csv(outPath, *error_histogram(e))


def colorizePointcloud(n_points, origin_offsets, origin_shot, origin_xy, images, defaultColor=DEFAULT_COLOR):
    """Scene::colorizePointcloud(defaultColor) (Scene.cpp:569-617) -> rgb (n x 3) uint8."""
    return colorize_pointcloud(n_points, origin_offsets, origin_shot, origin_xy, images, defaultColor)[0]


def writeToPLY(path, xyz=None, rgb=None, *, cameras=None, shots=None, color=None, onlyRecovered: bool = True) -> None:
    """PclUtils::writeToPLY, both overloads.  writeToPLY(path, xyz, rgb_or_None): the cloud (PclUtils.cpp:401-460);
    writeToPLY(path, cameras=[(width, height, K)], shots=[(camera, recovered, pose)], color=None,
    onlyRecovered=True): the cameras (PclUtils.cpp:466-590)."""
    if (cameras is None) != (shots is None) or (xyz is None) == (cameras is None):
        raise ValueError("pass either xyz (and rgb) or cameras and shots")
    if cameras is not None:
        write_cameras_ply(path, cameras, shots, color, onlyRecovered)
    else:
        write_pointcloud_ply(path, xyz, rgb)
