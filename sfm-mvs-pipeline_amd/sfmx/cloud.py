"""Point-cloud neighbour statistics — host mirror of ``PclUtils::writeToStatisticsCSV`` /
``writeToNeighborCSV`` / ``writeToNeighborPLY`` (src/photogrammetrie/util/PclUtils.cpp:75-399), the
``-Prun=pcl-stats`` sub-program.  The per-point nearest-neighbour search runs in the HIP kernels behind
``sfmx_cloud_neighbor_distances``; statistics, histogram, PLY reading and the three writers are the
library's C++ host code (include/sfmx_cloud.h).  This module only marshals buffers.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import lib, check, sfmx_cloud_stats, SFMX_ECAPACITY


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch") and hasattr(a, "data_ptr")


def neighbor_distances(xyz, max_equal: int = 0, neighbors: bool = False, device: int = 0, stream: int = 0):
    """xyz: (n x 3) float32 numpy array, or a float32 tensor on a GPU (the result is then tensors on that
    device).  -> distances (n, float64), or (distances, neighbor (n, int64)) with neighbors=True: the
    smallest index among the nearest points at a positive float distance, -1 where the distance is 0."""
    if _is_tensor(xyz):
        import torch
        if not xyz.is_cuda or xyz.dtype != torch.float32:
            raise ValueError("a tensor input must be a float32 tensor on a GPU")
        x = xyz.contiguous().reshape(-1, 3)
        n, dev = x.shape[0], x.device
        dist = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        nb = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if neighbors else None
        if not stream:
            torch.cuda.synchronize(dev)   # the tensors were made on torch's stream, the call runs on the default one
        check(lib.sfmx_cloud_neighbor_distances(x.data_ptr() if n else None, n, int(max_equal), 1, dev.index or 0,
                                                stream or None, dist.data_ptr(), nb.data_ptr() if neighbors else None),
              "sfmx_cloud_neighbor_distances")
        return (dist[:n], nb[:n]) if neighbors else dist[:n]
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(x)
    dist = np.zeros(max(n, 1), np.float64)
    nb = np.full(max(n, 1), -1, np.int64)
    check(lib.sfmx_cloud_neighbor_distances(x.ctypes.data if n else None, n, int(max_equal), 0, int(device), stream or None,
                                            dist.ctypes.data, nb.ctypes.data if neighbors else None),
          "sfmx_cloud_neighbor_distances")
    return (dist[:n], nb[:n]) if neighbors else dist[:n]


def last_stats() -> dict:
    """kernel_ms, evaluations, brute_queries of this thread's last neighbor_distances call."""
    ms, ev, bq = C.c_float(0), C.c_int64(0), C.c_int64(0)
    check(lib.sfmx_cloud_last_stats(C.byref(ms), C.byref(ev), C.byref(bq)), "sfmx_cloud_last_stats")
    return dict(kernel_ms=float(ms.value), evaluations=int(ev.value), brute_queries=int(bq.value))


STAT_FIELDS = ("n_points", "max", "min", "mean", "median", "variance", "deviation")


def statistics(distances, n_points: int | None = None) -> dict:
    """MathUtils::calculateStatistics of a distance list (n_points: the N_Points column; default len)."""
    d = np.ascontiguousarray(distances, np.float64).reshape(-1)
    s = sfmx_cloud_stats()
    check(lib.sfmx_cloud_statistics(d.ctypes.data if len(d) else None, len(d), len(d) if n_points is None else int(n_points),
                                    C.byref(s)), "sfmx_cloud_statistics")
    return {k: getattr(s, k) for k in STAT_FIELDS}


def neighbor_histogram(distances, resolution: float = -1.0):
    """-> (keys float64 ascending, counts uint64); resolution < 0: the variance of the list."""
    d = np.ascontiguousarray(distances, np.float64).reshape(-1)
    need = C.c_int64(0)
    p = d.ctypes.data if len(d) else None
    rc = lib.sfmx_cloud_histogram(p, len(d), float(resolution), None, None, 0, C.byref(need))
    if rc != SFMX_ECAPACITY:
        check(rc, "sfmx_cloud_histogram")
    k = np.zeros(max(int(need.value), 1), np.float64)
    c = np.zeros(max(int(need.value), 1), np.uint64)
    check(lib.sfmx_cloud_histogram(p, len(d), float(resolution), k.ctypes.data, c.ctypes.data, len(k), C.byref(need)),
          "sfmx_cloud_histogram")
    return k[:need.value], c[:need.value]


def read_ply(path) -> dict:
    """-> dict(xyz (n x 3) float32, face_sizes (f) int32, face_indices int32 concatenated).  ValueError for a
    file the reader does not take (include/sfmx_cloud.h)."""
    p = os.fsencode(path)
    n, f, k = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(lib.sfmx_ply_read(p, None, 0, C.byref(n), None, 0, C.byref(f), None, 0, C.byref(k)), "sfmx_ply_read")
    xyz = np.zeros((max(n.value, 1), 3), np.float32)
    fs = np.zeros(max(f.value, 1), np.int32)
    fi = np.zeros(max(k.value, 1), np.int32)
    check(lib.sfmx_ply_read(p, xyz.ctypes.data, len(xyz), C.byref(n), fs.ctypes.data, len(fs), C.byref(f),
                            fi.ctypes.data, len(fi), C.byref(k)), "sfmx_ply_read")
    return dict(xyz=xyz[:n.value], face_sizes=fs[:f.value], face_indices=fi[:k.value])


def write_stats_csv(path, stats: dict) -> None:
    s = sfmx_cloud_stats(*[stats[k] for k in STAT_FIELDS])
    check(lib.sfmx_cloud_write_stats_csv(os.fsencode(path), C.byref(s)), "sfmx_cloud_write_stats_csv")


def write_neighbors_csv(path, keys, counts) -> None:
    k = np.ascontiguousarray(keys, np.float64).reshape(-1)
    c = np.ascontiguousarray(counts, np.uint64).reshape(-1)
    if len(k) != len(c):
        raise ValueError("keys and counts differ in length")
    check(lib.sfmx_cloud_write_neighbors_csv(os.fsencode(path), k.ctypes.data if len(k) else None,
                                             c.ctypes.data if len(c) else None, len(k)), "sfmx_cloud_write_neighbors_csv")


def write_quality_ply(path, xyz, distances, face_sizes=(), face_indices=(), distance_cutoff: float = -1.0) -> None:
    """distances: one per point of xyz, or empty (a cloud of at most one point)."""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(distances, np.float64).reshape(-1)
    fs = np.ascontiguousarray(face_sizes, np.int32).reshape(-1)
    fi = np.ascontiguousarray(face_indices, np.int32).reshape(-1)
    if len(d) not in (0, len(x)):
        raise ValueError("distances must be empty or have one entry per point")
    if int(fs.sum()) != len(fi) or (len(fs) and fs.min() < 0):
        raise ValueError("face_sizes do not add up to len(face_indices)")
    check(lib.sfmx_cloud_write_quality_ply(os.fsencode(path), x.ctypes.data if len(x) else None,
                                           d.ctypes.data if len(d) else None, len(d), fs.ctypes.data if len(fs) else None,
                                           len(fs), fi.ctypes.data if len(fi) else None, float(distance_cutoff)),
          "sfmx_cloud_write_quality_ply")
