"""CPU: the control flow of sfmx_sfm_triangulate_steps (csrc/sfm_host.hpp) against the literal restatement
tests/sfm_ref.py of SfM::triangulate, both over the toy world of tests/sfm_toy.py.  The traces, the steps' call
logs, the recovered flags, the pair states and the final match counts must be equal.  Fails without the feature:
the entry point does not exist."""
import ctypes as C

import numpy as np
import pytest

import sfm_ref
import sfm_toy
from sfmx import _lib, sfm


def run_both(sc):
    wr = sfm_toy.World(sc)
    ref = sfm_ref.triangulate(wr, sc.n_shots, sc.pairs, sc.n_matches, sc.homography, **sc.params)
    wn = sfm_toy.World(sc)
    got = sfm.triangulate_steps(wn, sc.n_shots, sc.pairs, sc.n_matches, sc.homography, sfm.default_params(**sc.params))
    return ref, wr, got, wn


def check_equal(sc):
    ref, wr, got, wn = run_both(sc)
    assert sfm_toy.same_trace(got["trace"], ref["trace"]), (sc.name, got["trace"], ref["trace"])
    assert wn.log == wr.log, sc.name
    assert got["recovered"].tolist() == ref["recovered"], sc.name
    assert got["pair_state"].tolist() == ref["pair_state"], sc.name
    assert got["pair_n_matches"].tolist() == ref["pair_n_matches"], sc.name
    s = got["summary"]
    assert (s["ba_calls"], s["ba_iterations"], s["last_termination_type"]) == (ref["ba"]["calls"], ref["ba"]["iterations"], ref["ba"]["last"])
    assert s["shots_recovered"] == sum(ref["recovered"])
    assert [s["pairs_open"], s["pairs_triangulated"], s["pairs_failed"]] == [ref["pair_state"].count(k) for k in (0, 1, 2)]
    assert s["step_calls"]["bundle_adjust"] == s["ba_calls"] and s["step_calls"]["relative_pose"] == sum(e[0] == "relative_pose" for e in wn.log)
    return ref, got


@pytest.mark.parametrize("sc", sfm_toy.named_scenarios(), ids=lambda sc: sc.name)
def test_named_scenes_equal_the_literal_loop(sc):
    check_equal(sc)


def test_random_graphs_equal_the_literal_loop():
    seen = set()
    for sc in sfm_toy.random_scenarios():
        ref, _ = check_equal(sc)
        seen |= {e[0] for e in ref["trace"]}
    # the random tables reach every branch of the loop
    assert seen == set(sfm.EVENT_NAMES.values()), set(sfm.EVENT_NAMES.values()) - seen


def by_name(name):
    return next(sc for sc in sfm_toy.named_scenarios() if sc.name == name)


def test_what_the_scenes_are_about():
    """The named scenes take the branches they are named for (on the literal loop)."""
    ev = lambda name: [e for e in run_both(by_name(name))[0]["trace"]]
    names = lambda name: [e[0] for e in ev(name)]
    assert names("all_below_homography") == ["NO_CANDIDATE_PAIR", "NO_INITIAL_PAIR"]
    t = names("two_initial_rejected")
    assert t[:5] == ["INITIAL_TRY", "INITIAL_THROWS", "INITIAL_TRY", "INITIAL_LOW_RATIO", "INITIAL_TRY"] and t[5] == "INITIAL_PAIR"
    t = ev("below_min_baseline_mixed")
    assert t[0][:2] == ("INITIAL_TRY", 1)   # pair 0 has the lowest ratio and too few matches: it comes after the others
    assert "SHOT_FAILED" in names("one_registration_fails") and names("one_registration_fails")[-1] == "DONE"
    t = ev("registration_status_2")
    assert ("SHOT_FAILED", 2, 2, -1.0) in t
    t = run_both(by_name("every_registration_fails"))[0]
    assert sum(t["recovered"]) == 2 and t["pair_state"].count(0) == 0
    t = run_both(by_name("pair_throws_in_loop"))[0]
    assert "PAIR_THROWS" in [e[0] for e in t["trace"]] and t["pair_state"][2] == 0 and all(t["recovered"])
    assert "NO_REMAINING_SHOT" in [e[0] for e in t["trace"]]
    t = run_both(by_name("two_components"))[0]
    assert t["recovered"] == [True] * 3 + [False] * 3 and t["pair_state"] == [1, 1, 1, 2, 2, 2]
    t = run_both(by_name("two_shots"))[0]
    assert [e[0] for e in t["trace"]] == ["INITIAL_TRY", "INITIAL_PAIR", "BUNDLE_ADJUST", "DONE"]
    t = run_both(by_name("ties"))[0]
    chosen = [e for e in t["trace"] if e[0] == "SHOT_CHOSEN"]
    assert chosen[0][1] == 2   # pair (0, 1) is the initial pair; every other shot counts the same: the lowest index


def test_short_trace_is_a_capacity_error_with_complete_outputs():
    sc = by_name("complete6")
    full = sfm.triangulate_steps(sfm_toy.World(sc), sc.n_shots, sc.pairs, sc.n_matches, sc.homography)
    with pytest.raises(_lib.SfmxError) as e:
        sfm.triangulate_steps(sfm_toy.World(sc), sc.n_shots, sc.pairs, sc.n_matches, sc.homography, trace_capacity=3)
    assert e.value.code == _lib.SFMX_ECAPACITY and len(full["trace"]) > 3


def test_a_raising_step_aborts_the_loop():
    sc = by_name("ring6")

    class Bad(sfm_toy.World):
        def register_shot(self, shot):
            raise KeyError("boom")
    w = Bad(sc)
    with pytest.raises(KeyError):
        sfm.triangulate_steps(w, sc.n_shots, sc.pairs, sc.n_matches, sc.homography)
    assert w.log[-1][0] == "count_candidates"   # nothing ran after the failing step


class NoStepMayRun:
    def __getattr__(self, name):
        def step(*a):
            raise AssertionError(f"step {name} was called")
        return step


@pytest.mark.parametrize("field,value", [("min_match_count_for_baseline", 3), ("min_homography_inlier_ratio", -0.01),
                                         ("min_homography_inlier_ratio", 1.5), ("min_pose_inlier_ratio", float("nan")),
                                         ("min_pose_inlier_ratio", 1.0001), ("point_merge_distance", float("nan")),
                                         ("feature_merge_distance", float("nan"))])
def test_bad_parameters_fail_before_any_step(field, value):
    sc = by_name("ring6")
    with pytest.raises(ValueError):
        sfm.triangulate_steps(NoStepMayRun(), sc.n_shots, sc.pairs, sc.n_matches, sc.homography, sfm.default_params(**{field: value}))


def test_bad_graph_fails_before_any_step():
    sc = by_name("ring6")
    for pairs in ([(0, 6)] + [(1, 2)] * 5, [(-1, 0)] + [(1, 2)] * 5):
        with pytest.raises(ValueError):
            sfm.triangulate_steps(NoStepMayRun(), sc.n_shots, pairs, sc.n_matches, sc.homography)
    bad = sc.n_matches.copy()
    bad[2] = -1
    with pytest.raises(ValueError):
        sfm.triangulate_steps(NoStepMayRun(), sc.n_shots, sc.pairs, bad, sc.homography)
    h = sc.homography.copy()
    h[1] = np.nan
    with pytest.raises(ValueError):
        sfm.triangulate_steps(NoStepMayRun(), sc.n_shots, sc.pairs, sc.n_matches, h)


def test_null_pointers_fail_before_any_step():
    sc = by_name("two_shots")
    prm = sfm.default_params()
    calls = []
    fns = [t(lambda *a: calls.append(1) or 0) for t in (_lib.SFM_RELATIVE_POSE_FN, _lib.SFM_TRIANGULATE_PAIR_FN,
                                                         _lib.SFM_ADD_ELEMENTS_FN, _lib.SFM_COUNT_CANDIDATES_FN,
                                                         _lib.SFM_REGISTER_SHOT_FN, _lib.SFM_ACCEPT_SHOT_FN,
                                                         _lib.SFM_BUNDLE_ADJUST_FN)]
    table = _lib.sfmx_sfm_steps(*fns)
    pairs, cnt, hr = sc.pairs.copy(), sc.n_matches.copy(), sc.homography.copy()
    rec, state = np.zeros(2, np.int32), np.zeros(1, np.int32)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    good = [C.byref(table), None, C.byref(prm), 2, pairs.ctypes.data_as(i32), 1, cnt.ctypes.data_as(i32),
            hr.ctypes.data_as(f64), rec.ctypes.data_as(i32), state.ctypes.data_as(i32), None, None, 0, None, None]
    for i in (0, 2, 4, 6, 7, 8, 9):
        args = list(good)
        args[i] = None
        assert _lib.lib.sfmx_sfm_triangulate_steps(*args) == _lib.SFMX_EINVAL, i
    hole = _lib.sfmx_sfm_steps(*fns[:4])   # the last three steps are null
    assert _lib.lib.sfmx_sfm_triangulate_steps(C.byref(hole), *good[1:]) == _lib.SFMX_EINVAL
    assert not calls
    assert _lib.lib.sfmx_sfm_triangulate_steps(*good) == _lib.SFMX_OK and calls   # and the good call runs
    assert _lib.lib.sfmx_sfm_default_params(None) == _lib.SFMX_EINVAL


def test_two_cameras_are_a_capacity_error_before_any_step():
    """sfmx_sfm_triangulate adjusts one intrinsics block: a second camera is refused with a text before any device is
    touched."""
    cams = (_lib.sfmx_tri_camera * 2)()
    z = C.c_int64(0)
    rc = _lib.lib.sfmx_sfm_triangulate(None, None, 0, None, cams, 2, 1, None, 0, None, C.byref(z), None,
                                       C.byref(sfm.default_params()), 0, None, None, None, None, 0, None, None, None, 0, None,
                                       None, None, None, None, None, 0, None, None, None)
    assert rc == _lib.SFMX_ECAPACITY and b"one camera" in _lib.lib.sfmx_last_error()
    assert _lib.lib.sfmx_sfm_triangulate(None, None, 0, None, None, 0, 1, None, 0, None, C.byref(z), None,
                                         C.byref(sfm.default_params()), 0, None, None, None, None, 0, None, None, None, 0, None,
                                         None, None, None, None, None, 0, None, None, None) == _lib.SFMX_EINVAL
