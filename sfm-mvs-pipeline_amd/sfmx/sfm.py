"""The incremental reconstruction loop, ``SfM::triangulate`` (sfm/SfM.cpp:164-381) — host mirror over
include/sfmx_sfm.h.

``triangulate_steps`` runs the loop's control flow (native, csrc/sfm_host.hpp) over steps given as Python
callables: the loop owns the pair lists, the recovered flags, the pairs' match counts and the homography
ratios; the steps own keypoints, poses and the cloud.  It needs no GPU.  The steps object has

    relative_pose(pair) -> (status, n_inliers)              status 1, or 0 where the reference throws
    triangulate_pair(pair, initial) -> n_points              list := inliers, (initial: poses), triangulateMatch
    add_elements(pair, merge)                                append (merge False) or mergePointcloudElement3d2d
    count_candidates(shots) -> counts                        sizes of find3d2dMatches' lists
    register_shot(shot) -> (status, ratio, distinct_pairs)   status 1, or another value >= 0 for "throws"
    accept_shot(shot)                                        the found pose becomes the shot's pose
    bundle_adjust() -> (iterations, termination_type)

An exception raised by a step aborts the loop and is raised again by ``triangulate_steps``.

``triangulate`` is the same loop with the library's own rows as steps (sfmx_sfm_triangulate): the reconstruction
of a scene from its keypoints, its match graph and the pairs' homography ratios.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check

EVENT_NAMES = {1: "NO_CANDIDATE_PAIR", 2: "INITIAL_TRY", 3: "INITIAL_THROWS", 4: "INITIAL_LOW_RATIO", 5: "INITIAL_PAIR",
               6: "NO_INITIAL_PAIR", 7: "BUNDLE_ADJUST", 8: "SHOT_CHOSEN", 9: "SHOT_FAILED", 10: "PAIR_FAILED",
               11: "SHOT_REGISTERED", 12: "PAIR_SKIPPED", 13: "PAIR_THROWS", 14: "PAIR_TRIANGULATED",
               15: "NO_REMAINING_SHOT", 16: "DONE"}
EVENTS = {v: k for k, v in EVENT_NAMES.items()}
PAIR_OPEN, PAIR_DONE, PAIR_LOST = 0, 1, 2
STEP_NAMES = ("relative_pose", "triangulate_pair", "add_elements", "count_candidates", "register_shot", "accept_shot",
              "bundle_adjust")
EVENT_DTYPE = np.dtype([("event", np.int32), ("a", np.int32), ("b", np.int32), ("_pad", np.int32), ("value", np.float64)])


def default_params(**overrides) -> _lib.sfmx_sfm_params:
    """SfM.h:48-57; keyword arguments replace single fields."""
    p = _lib.sfmx_sfm_params()
    check(lib.sfmx_sfm_default_params(C.byref(p)), "sfmx_sfm_default_params")
    for k, v in overrides.items():
        if k not in dict(p._fields_):
            raise TypeError(f"sfmx_sfm_params has no field {k}")
        setattr(p, k, v)
    return p


def _trace_list(ev):
    return [(EVENT_NAMES[int(e["event"])], int(e["a"]), int(e["b"]), float(e["value"])) for e in ev]


def _summary_dict(summ):
    summary = {n: int(getattr(summ, n)) for n, _ in summ._fields_ if not n.startswith("step_")}
    summary["step_calls"] = dict(zip(STEP_NAMES, (int(v) for v in summ.step_calls)))
    summary["step_wall_ms"] = dict(zip(STEP_NAMES, (float(v) for v in summ.step_wall_ms)))
    return summary


ROW_NAMES = ("count", "find", "register", "pose", "triangulate", "merge", "ba", "handoff")


def triangulate(keypoints, shot_size, camera, camera_model: int, pairs, matches, offsets, homography_ratio, params=None,
                device: int = 0, trace_capacity: int | None = None) -> dict:
    """SfM::triangulate over the GPU rows.  keypoints[i]: n_i x 2 float32; shot_size: n_shots x 2 (width, height);
    camera: (K 3x3, dist k1 k2 p1 p2 k3), the scene's one camera; camera_model: sfmx.ba.CAM_*; pairs, matches,
    offsets: the packed match graph; homography_ratio: one per pair.
    -> dict(recovered bool[n_shots], poses n_shots x 3 x 4 (NaN where not recovered), camera (K, dist) after the last
    adjustment, xyz, origin_offsets, origin_shot, origin_xy: the cloud, matches, offsets: the final lists,
    pair_state, trace, summary, timing: per row dict(calls, device_ms, wall_ms, handoff_bytes))."""
    from .matching import DMATCH_DTYPE
    kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    n_shots = len(kps)
    nkp = np.array([len(k) for k in kps], np.int32)
    ptrs = (C.c_void_p * max(n_shots, 1))(*[k.ctypes.data for k in kps])
    size = np.ascontiguousarray(shot_size, np.int32).reshape(-1, 2)
    if len(size) != n_shots:
        raise ValueError("shot_size must have one (width, height) per shot")
    K, dist = camera
    cam = _lib.sfmx_tri_camera()
    cam.K[:] = np.asarray(K, np.float64).reshape(9).tolist()
    cam.dist[:] = np.asarray(dist, np.float64).reshape(5).tolist()
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n_pairs = len(pairs)
    m = np.ascontiguousarray(matches, DMATCH_DTYPE)
    off = np.ascontiguousarray(offsets, np.int64)
    hr = np.ascontiguousarray(homography_ratio, np.float64).reshape(-1)
    if len(off) != n_pairs + 1 or len(hr) != n_pairs or len(m) != int(off[-1]):
        raise ValueError("offsets, homography_ratio and matches must fit the pair list")
    prm = params if params is not None else default_params()
    M = len(m)
    if trace_capacity is None:
        trace_capacity = 2 * n_pairs + 8 + (n_shots + n_pairs) * (n_pairs + 4)
    rec = np.zeros(max(n_shots, 1), np.int32)
    pose = np.zeros((max(n_shots, 1), 3, 4))
    out_cam = _lib.sfmx_tri_camera()
    xyz = np.zeros((max(M, 1), 3))
    oo = np.zeros(M + 1, np.int64)
    osh = np.zeros(max(2 * M, 1), np.int32)
    oxy = np.zeros((max(2 * M, 1), 2))
    n_pts, n_rec = C.c_int64(0), C.c_int64(0)
    om = np.zeros(max(M, 1), DMATCH_DTYPE)
    ooff = np.zeros(n_pairs + 1, np.int64)
    state = np.zeros(max(n_pairs, 1), np.int32)
    ev = np.zeros(max(trace_capacity, 1), EVENT_DTYPE)
    n_ev = C.c_int64(0)
    summ, tim = _lib.sfmx_sfm_summary(), _lib.sfmx_sfm_timing()
    i32, i64, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    check(lib.sfmx_sfm_triangulate(ptrs, nkp.ctypes.data_as(i32), n_shots, size.ctypes.data_as(i32), C.byref(cam), 1,
                                   int(camera_model), pairs.ctypes.data_as(i32), n_pairs, m.ctypes.data if M else None,
                                   off.ctypes.data_as(i64), hr.ctypes.data_as(f64), C.byref(prm), int(device),
                                   rec.ctypes.data_as(i32), pose.ctypes.data_as(f64), C.byref(out_cam), xyz.ctypes.data, M,
                                   oo.ctypes.data_as(i64), osh.ctypes.data_as(i32), oxy.ctypes.data, 2 * M, C.byref(n_pts),
                                   C.byref(n_rec), om.ctypes.data, ooff.ctypes.data_as(i64), state.ctypes.data_as(i32),
                                   ev.ctypes.data_as(C.POINTER(_lib.sfmx_sfm_event)), int(trace_capacity), C.byref(n_ev),
                                   C.byref(summ), C.byref(tim)), "sfmx_sfm_triangulate")
    k, r = int(n_pts.value), int(n_rec.value)
    timing = {name: dict(calls=int(tim.calls[i]), device_ms=float(tim.device_ms[i]), wall_ms=float(tim.wall_ms[i]),
                         handoff_bytes=int(tim.handoff_bytes[i])) for i, name in enumerate(ROW_NAMES)}
    return dict(recovered=rec[:n_shots].astype(bool), poses=pose[:n_shots],
                camera=(np.array(out_cam.K[:]).reshape(3, 3), np.array(out_cam.dist[:])),
                xyz=xyz[:k], origin_offsets=oo[:k + 1], origin_shot=osh[:r], origin_xy=oxy[:r],
                matches=om[:int(ooff[-1])], offsets=ooff, pair_state=state[:n_pairs], trace=_trace_list(ev[:n_ev.value]),
                summary=_summary_dict(summ), timing=timing)


def triangulate_steps(steps, n_shots: int, pairs, pair_n_matches, homography_ratio, params=None,
                      trace_capacity: int | None = None) -> dict:
    """-> dict(recovered bool[n_shots], pair_state int32[n_pairs] (PAIR_*), pair_n_matches int32[n_pairs],
    trace: list of (event name, a, b, value), summary: dict)."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n_pairs = len(pairs)
    cnt = np.ascontiguousarray(pair_n_matches, np.int32).reshape(-1)
    hr = np.ascontiguousarray(homography_ratio, np.float64).reshape(-1)
    if len(cnt) != n_pairs or len(hr) != n_pairs:
        raise ValueError("pair_n_matches and homography_ratio must have one entry per pair")
    prm = params if params is not None else default_params()
    failure = []

    def guarded(fn):
        def call(*a):
            try:
                return fn(*a)
            except BaseException as e:   # nothing may propagate through the C frames
                failure.append(e)
                return _lib.SFMX_ESTATE
        return call

    def relative_pose(_, pair, n_inliers):
        status, n = steps.relative_pose(int(pair))
        n_inliers[0] = int(n)
        return int(status)

    def triangulate_pair(_, pair, initial, n_points):
        n_points[0] = int(steps.triangulate_pair(int(pair), bool(initial)))
        return 0

    def add_elements(_, pair, merge):
        steps.add_elements(int(pair), bool(merge))
        return 0

    def count_candidates(_, shots, n, counts):
        got = steps.count_candidates([int(shots[i]) for i in range(n)])
        if len(got) != n:
            raise ValueError("count_candidates must return one count per shot")
        for i in range(n):
            counts[i] = int(got[i])
        return 0

    def register_shot(_, shot, ratio, distinct, capacity, n_distinct):
        status, r, dp = steps.register_shot(int(shot))
        if len(dp) > capacity:
            raise ValueError("register_shot returned more pairs than the scene has")
        ratio[0] = float(r)
        for i, p in enumerate(dp):
            distinct[i] = int(p)
        n_distinct[0] = len(dp)
        return int(status)

    def accept_shot(_, shot):
        steps.accept_shot(int(shot))
        return 0

    def bundle_adjust(_, iterations, termination):
        it, term = steps.bundle_adjust()
        iterations[0], termination[0] = int(it), int(term)
        return 0

    table = _lib.sfmx_sfm_steps(_lib.SFM_RELATIVE_POSE_FN(guarded(relative_pose)),
                                _lib.SFM_TRIANGULATE_PAIR_FN(guarded(triangulate_pair)),
                                _lib.SFM_ADD_ELEMENTS_FN(guarded(add_elements)),
                                _lib.SFM_COUNT_CANDIDATES_FN(guarded(count_candidates)),
                                _lib.SFM_REGISTER_SHOT_FN(guarded(register_shot)),
                                _lib.SFM_ACCEPT_SHOT_FN(guarded(accept_shot)),
                                _lib.SFM_BUNDLE_ADJUST_FN(guarded(bundle_adjust)))
    if trace_capacity is None:   # per iteration: chosen, registered or failed, one event per pair, BA
        trace_capacity = 2 * n_pairs + 8 + (int(n_shots) + n_pairs) * (n_pairs + 4)
    rec = np.zeros(max(int(n_shots), 1), np.int32)
    state = np.zeros(max(n_pairs, 1), np.int32)
    out_cnt = np.zeros(max(n_pairs, 1), np.int32)
    ev = np.zeros(max(trace_capacity, 1), EVENT_DTYPE)
    n_ev = C.c_int64(0)
    summ = _lib.sfmx_sfm_summary()
    i32 = C.POINTER(C.c_int32)
    rc = lib.sfmx_sfm_triangulate_steps(C.byref(table), None, C.byref(prm), int(n_shots), pairs.ctypes.data_as(i32), n_pairs,
                                        cnt.ctypes.data_as(i32), hr.ctypes.data_as(C.POINTER(C.c_double)),
                                        rec.ctypes.data_as(i32), state.ctypes.data_as(i32), out_cnt.ctypes.data_as(i32),
                                        ev.ctypes.data_as(C.POINTER(_lib.sfmx_sfm_event)), int(trace_capacity),
                                        C.byref(n_ev), C.byref(summ))
    if failure:
        raise failure[0]
    check(rc, "sfmx_sfm_triangulate_steps")
    return dict(recovered=rec[:int(n_shots)].astype(bool), pair_state=state[:n_pairs], pair_n_matches=out_cnt[:n_pairs],
                trace=_trace_list(ev[:n_ev.value]), summary=_summary_dict(summ))


def reconstructScene(images, camera, camera_model: int, pairs=None, detector=None, params=None, norm=None,
                     match_threshold: int = 20, distinct_matches: bool = False,
                     ransac_matching_threshold: float | None = None, device: int = 0) -> dict:
    """SfM::reconstructScene (SfM.cpp:143-162) over the existing mirrors: extractFeatures (detector.detectAndCompute on
    every 8-bit gray image; default SIFT(0, 3, 0.09)), calculateShotMatches (exact 2-NN + ratio 0.7 + the match-graph
    filters over `pairs`, default every unordered pair), calculateHomography over the kept pairs, then ``triangulate``.
    -> triangulate's dict plus keypoints, descriptors, kept pairs, homography_ratio."""
    from . import features, homography
    from .matching import BFMatcher, LOWE_RATIO, NORM_L2, pairs_unordered
    if len(images) < 2:
        raise ValueError("the scene needs at least two shots")   # SfM.cpp:147-149
    det = detector or features.SIFT.create(0, 3, 0.09)
    feats = [det.detectAndCompute(np.ascontiguousarray(im, np.uint8)) for im in images]
    kps = [np.stack([k["x"], k["y"]], 1) for k, _ in feats]
    pairs = pairs_unordered(len(images)) if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = BFMatcher(NORM_L2 if norm is None else norm, device=device)
    try:
        m.set_images([d for _, d in feats])
        m.run(pairs, LOWE_RATIO, bool(distinct_matches), int(match_threshold))
        matches, off, keep = m.fetch()
    finally:
        m.close()
    kept = [p for p in range(len(pairs)) if keep[p]]
    kpairs = pairs[kept].reshape(-1, 2)
    koff = np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[kept])]).astype(np.int64)
    kmatches = np.concatenate([matches[off[p]:off[p + 1]] for p in kept]) if kept else matches[:0]
    sizes = [(im.shape[1], im.shape[0]) for im in images]
    kw = {} if ransac_matching_threshold is None else {"threshold": ransac_matching_threshold}
    ratios = homography.homography_ratios(kps, sizes, kpairs, kmatches, koff, device=device, **kw)
    r = triangulate(kps, sizes, camera, camera_model, kpairs, kmatches, koff, ratios, params, device=device)
    r.update(keypoints=kps, descriptors=[d for _, d in feats], pairs=kpairs, homography_ratio=ratios)
    return r
