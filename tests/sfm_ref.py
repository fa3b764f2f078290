"""A literal Python restatement of SfM::triangulate (sfm/SfM.cpp:164-381) over per-object scene state: lists of
pair objects that are filtered, sorted, removed from and appended to as the reference does with its vectors of
shared_ptrs.  The steps are the callables of sfmx.sfm.triangulate_steps; the trace it returns has that function's
records.  Its only departures from the reference are the order decisions of DESIGN.md §9 (initial candidates:
enough matches first, ascending ratio, stable; remaining shots by index; count ties to the lower index; no
candidate pair: nothing recovered)."""
from dataclasses import dataclass

import numpy as np


@dataclass(eq=False)
class ShotObj:
    index: int
    recovered: bool = False


@dataclass(eq=False)
class PairObj:
    index: int
    left: ShotObj
    right: ShotObj
    n_matches: int          # getMatches().size()
    homography_ratio: float
    state: int = 0          # the list it was moved to last (0 open, 1 triangulated, 2 failed)


def _div(a, b):
    """(double) a / (double) b, the hardware's quotient also for b == 0"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def triangulate(steps, n_shots, pairs, pair_n_matches, homography_ratio, min_match_count_for_baseline=100,
                min_homography_inlier_ratio=0.5, min_pose_inlier_ratio=0.5):
    shots = [ShotObj(i) for i in range(n_shots)]
    scene_pairs = [PairObj(i, shots[int(l)], shots[int(r)], int(n), float(h))
                   for i, ((l, r), n, h) in enumerate(zip(pairs, pair_n_matches, homography_ratio))]
    trace = []
    ba = dict(calls=0, iterations=0, last=-1)

    def bundle_adjust():
        it, term = steps.bundle_adjust()
        ba["calls"] += 1
        ba["iterations"] += int(it)
        ba["last"] = int(term)
        trace.append(("BUNDLE_ADJUST", int(it), int(term), 0.0))

    def result():
        return dict(recovered=[s.recovered for s in shots], pair_state=[p.state for p in scene_pairs],
                    pair_n_matches=[p.n_matches for p in scene_pairs], trace=trace, ba=ba)

    to_triangulate = list(scene_pairs)
    triangulated = []
    failed = []
    if not to_triangulate:
        return result()

    # initial pair
    ordered = list(to_triangulate)
    ordered = [m for m in ordered if not (m.homography_ratio < min_homography_inlier_ratio)]
    enough = sorted([m for m in ordered if m.n_matches >= min_match_count_for_baseline], key=lambda m: m.homography_ratio)
    fewer = sorted([m for m in ordered if not (m.n_matches >= min_match_count_for_baseline)], key=lambda m: m.homography_ratio)
    ordered = enough + fewer
    if not ordered:
        trace.append(("NO_CANDIDATE_PAIR", -1, -1, 0.0))
    found = False
    for match in ordered:
        trace.append(("INITIAL_TRY", match.index, match.n_matches, match.homography_ratio))
        status, n_inliers = steps.relative_pose(match.index)
        if status != 1:
            trace.append(("INITIAL_THROWS", match.index, -1, 0.0))
            continue
        ratio = _div(n_inliers, match.n_matches)
        if ratio < min_pose_inlier_ratio:
            trace.append(("INITIAL_LOW_RATIO", match.index, int(n_inliers), ratio))
            continue
        match.n_matches = int(n_inliers)
        n_points = steps.triangulate_pair(match.index, True)
        steps.add_elements(match.index, False)
        match.left.recovered = True
        match.right.recovered = True
        to_triangulate = [m for m in to_triangulate if m is not match]
        triangulated.append(match)
        match.state = 1
        trace.append(("INITIAL_PAIR", match.index, int(n_points), ratio))
        found = True
        break
    if found:
        bundle_adjust()

    if not triangulated:
        trace.append(("NO_INITIAL_PAIR", -1, -1, 0.0))
        return result()

    while to_triangulate:
        remaining = set()
        for m in to_triangulate:
            if not m.left.recovered:
                remaining.add(m.left.index)
            if not m.right.recovered:
                remaining.add(m.right.index)
        remaining = sorted(remaining)
        if not remaining:
            trace.append(("NO_REMAINING_SHOT", len(to_triangulate), -1, 0.0))
            break
        counts = steps.count_candidates(list(remaining))
        matches3d2d = sorted(zip(remaining, counts), key=lambda sc: -sc[1])   # stable: ties keep the index order
        best_shot, best_count = matches3d2d[0]
        trace.append(("SHOT_CHOSEN", best_shot, int(best_count), float(len(remaining))))
        status, ratio, distinct = steps.register_shot(best_shot)
        if status != 1:
            ratio = -1.0
        if ratio < min_pose_inlier_ratio:
            trace.append(("SHOT_FAILED", best_shot, int(status), float(ratio)))
            failed_matches = [m for m in to_triangulate if m.left.index == best_shot or m.right.index == best_shot]
            for fm in failed_matches:
                to_triangulate = [m for m in to_triangulate if m is not fm]
                failed.append(fm)
                fm.state = 2
                trace.append(("PAIR_FAILED", fm.index, best_shot, 0.0))
            continue
        steps.accept_shot(best_shot)
        shots[best_shot].recovered = True
        trace.append(("SHOT_REGISTERED", best_shot, len(distinct), float(ratio)))
        for pi in distinct:
            sm = scene_pairs[pi]
            if not sm.left.recovered or not sm.right.recovered:
                trace.append(("PAIR_SKIPPED", sm.index, -1, 0.0))
                continue
            status, n_inliers = steps.relative_pose(sm.index)
            if status != 1:
                trace.append(("PAIR_THROWS", sm.index, -1, 0.0))
                continue
            sm.n_matches = int(n_inliers)
            n_points = steps.triangulate_pair(sm.index, False)
            steps.add_elements(sm.index, True)
            to_triangulate = [m for m in to_triangulate if m is not sm]
            triangulated.append(sm)
            sm.state = 1
            trace.append(("PAIR_TRIANGULATED", sm.index, int(n_points), float(n_inliers)))
        bundle_adjust()
    trace.append(("DONE", len(triangulated), len(failed), float(len(to_triangulate))))
    return result()
