"""GPU: sfmx_sfm_triangulate (SfM::triangulate over the library's rows) against the literal loop tests/sfm_ref.py
with the existing Python mirrors as its steps (tests/sfm_rows.py: one row call per reference call).  The rows are
deterministic and both runs make the same calls in the same order, so every output is compared bit for bit.
Fails without the feature: the entry point does not exist.

Measured on MI355X (mean reprojection error of the final scene, px): see DESIGN.md §8l."""
import numpy as np
import pytest

import sfm_cases
import sfm_ref
import sfm_rows
import sfm_toy
from sfmx import _lib, ba, report, sfm

pytestmark = pytest.mark.gpu

MAX_REPROJECTION_ERROR = 10.0   # SFMX_MAX_REPROJECTION_ERROR, the reference's own filter


def bits(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype).view(np.uint8)


def literal(sc, prm):
    rows = sfm_rows.RowSteps(sc["keypoints"], sc["shot_size"], sfm_cases.camera(), ba.CAM_SIMPLE_RADIAL, sc["pairs"],
                             sc["matches"], sc["offsets"], prm)
    ref = sfm_ref.triangulate(rows, len(sc["keypoints"]), sc["pairs"], np.diff(sc["offsets"]), sc["homography"],
                              min_match_count_for_baseline=prm.min_match_count_for_baseline,
                              min_homography_inlier_ratio=prm.min_homography_inlier_ratio,
                              min_pose_inlier_ratio=prm.min_pose_inlier_ratio)
    return ref, rows


def native(sc, prm):
    return sfm.triangulate(sc["keypoints"], sc["shot_size"], sfm_cases.camera(), ba.CAM_SIMPLE_RADIAL, sc["pairs"],
                           sc["matches"], sc["offsets"], sc["homography"], prm)


def same_rows_state(a, b):
    """Two literal runs: every array equal as bits."""
    ma, oa = a.graph()
    mb, ob = b.graph()
    return {"matches": ma.tobytes() == mb.tobytes() and np.array_equal(oa, ob), "xyz": np.array_equal(bits(a.xyz), bits(b.xyz)),
            "origins": np.array_equal(a.oo, b.oo) and np.array_equal(a.osh, b.osh) and np.array_equal(bits(a.oxy), bits(b.oxy)),
            "poses": np.array_equal(bits(a.poses), bits(b.poses)),
            "camera": np.array_equal(bits(a.K), bits(b.K)) and np.array_equal(bits(a.dist), bits(b.dist))}


def compare(sc, prm=None):
    prm = prm or sfm.default_params()
    ba.release_cache()
    got = native(sc, prm)
    ba.release_cache()
    ref, rows = literal(sc, prm)
    ba.release_cache()
    ref2, rows2 = literal(sc, prm)
    # precondition: the literal loop repeats itself exactly
    assert sfm_toy.same_trace(ref["trace"], ref2["trace"])
    same = same_rows_state(rows, rows2)
    assert all(same.values()), same
    # the native loop equals it
    assert sfm_toy.same_trace(got["trace"], ref["trace"]), (got["trace"], ref["trace"])
    assert got["recovered"].tolist() == ref["recovered"]
    assert got["pair_state"].tolist() == ref["pair_state"]
    m, off = rows.graph()
    assert np.array_equal(got["offsets"], off) and got["matches"].tobytes() == m.tobytes()
    assert np.array_equal(got["origin_offsets"], rows.oo) and np.array_equal(got["origin_shot"], rows.osh)
    assert np.array_equal(bits(got["origin_xy"]), bits(rows.oxy))
    assert np.array_equal(bits(got["xyz"]), bits(rows.xyz))
    rec = got["recovered"]
    assert np.array_equal(bits(got["poses"][rec]), bits(rows.poses[rec])) and np.all(np.isnan(got["poses"][~rec]))
    assert np.array_equal(bits(got["camera"][0]), bits(rows.K)) and np.array_equal(bits(got["camera"][1]), bits(rows.dist))
    s = got["summary"]
    assert (s["ba_calls"], s["ba_iterations"], s["last_termination_type"]) == (ref["ba"]["calls"], ref["ba"]["iterations"], ref["ba"]["last"])
    t = got["timing"]
    assert t["ba"]["calls"] == s["ba_calls"] and t["count"]["calls"] == s["step_calls"]["count_candidates"]
    assert t["pose"]["calls"] == s["step_calls"]["relative_pose"]
    if t["pose"]["calls"]:
        assert t["pose"]["device_ms"] > 0 and t["pose"]["handoff_bytes"] > 0
    return got, ref, rows


def mean_reprojection_error(got):
    poses = np.where(np.isnan(got["poses"]), 0.0, got["poses"])
    err = report.reprojection_errors(got["xyz"], got["origin_offsets"], got["origin_shot"], got["origin_xy"], [got["camera"]],
                                     np.zeros(len(poses), np.int32), poses)
    return float(np.mean(err))


def test_complete_graph_five_shots():
    sc = sfm_cases.scene(5, 300, noise=0.3, wrong=0.1, graph="complete", seed=11)
    got, ref, _ = compare(sc)
    assert got["recovered"].all() and (got["pair_state"] == sfm.PAIR_DONE).all()
    assert got["summary"]["last_termination_type"] == ba.CONVERGENCE
    e = mean_reprojection_error(got)
    print("scene 1 mean reprojection error", e, "points", len(got["xyz"]), "BA calls", got["summary"]["ba_calls"])
    assert e < MAX_REPROJECTION_ERROR


def test_a_shot_whose_lists_are_all_wrong_partners_fails_and_the_rest_is_reconstructed():
    sc = sfm_cases.scene(5, 300, noise=0.3, wrong=0.1, graph="complete", seed=11, all_wrong_shot=3)
    got, ref, _ = compare(sc)
    assert got["recovered"].tolist() == [True, True, True, False, True]
    names = [e[0] for e in got["trace"]]
    assert "SHOT_FAILED" in names and names[-1] == "DONE"
    lost = [p for p, (l, r) in enumerate(sc["pairs"]) if 3 in (l, r)]
    assert (got["pair_state"][lost] == sfm.PAIR_LOST).all() and (np.delete(got["pair_state"], lost) == sfm.PAIR_DONE).all()
    e = mean_reprojection_error(got)
    print("scene 2 mean reprojection error", e, "points", len(got["xyz"]))
    assert e < MAX_REPROJECTION_ERROR


def test_chain_of_six_shots_with_sequence_two_pairs():
    sc = sfm_cases.scene(6, 300, noise=0.3, wrong=0.1, graph="chain2", seed=12)
    got, ref, _ = compare(sc)
    assert got["recovered"].all()
    assert got["summary"]["last_termination_type"] == ba.CONVERGENCE
    e = mean_reprojection_error(got)
    print("scene 3 mean reprojection error", e, "points", len(got["xyz"]), "BA calls", got["summary"]["ba_calls"])
    assert e < MAX_REPROJECTION_ERROR


def test_two_shots():
    sc = sfm_cases.scene(2, 200, graph="complete", seed=13)
    got, ref, _ = compare(sc)
    assert got["recovered"].all() and [e[0] for e in got["trace"]] == ["INITIAL_TRY", "INITIAL_PAIR", "BUNDLE_ADJUST", "DONE"]
    assert np.array_equal(got["poses"][0], np.eye(3, 4)) or got["summary"]["ba_calls"] == 1   # [I|0], then adjusted


def test_no_pair_passes_the_homography_filter():
    sc = sfm_cases.scene(4, 200, graph="complete", seed=14)
    sc["homography"] = np.full(len(sc["pairs"]), 0.3)
    got, ref, _ = compare(sc)
    assert not got["recovered"].any() and len(got["xyz"]) == 0 and got["summary"]["ba_calls"] == 0
    assert [e[0] for e in got["trace"]] == ["NO_CANDIDATE_PAIR", "NO_INITIAL_PAIR"]
    assert got["matches"].tobytes() == sc["matches"].tobytes() and (got["pair_state"] == sfm.PAIR_OPEN).all()


def test_arguments_are_checked_before_any_row_runs():
    sc = sfm_cases.scene(3, 100, graph="complete", seed=15)
    cam = sfm_cases.camera()
    args = lambda **kw: {**dict(keypoints=sc["keypoints"], shot_size=sc["shot_size"], camera=cam, camera_model=ba.CAM_SIMPLE_RADIAL,
                                pairs=sc["pairs"], matches=sc["matches"], offsets=sc["offsets"],
                                homography_ratio=sc["homography"]), **kw}
    for prm in (sfm.default_params(min_match_count_for_baseline=3), sfm.default_params(min_pose_inlier_ratio=1.5),
                sfm.default_params(min_homography_inlier_ratio=-0.1), sfm.default_params(point_merge_distance=float("nan"))):
        with pytest.raises(ValueError):
            sfm.triangulate(**args(), params=prm)
    bad = sc["pairs"].copy()
    bad[0, 1] = 3
    with pytest.raises(ValueError):
        sfm.triangulate(**args(pairs=bad))
    bm = sc["matches"].copy()
    bm["queryIdx"][0] = 10 ** 6
    with pytest.raises(ValueError):
        sfm.triangulate(**args(matches=bm))
    with pytest.raises(ValueError):
        sfm.triangulate(**args(camera_model=2))


def functor_residuals(got):
    """The residual of every origin record under the reference's own Distortion cost functor
    (common/DistortionCamera.cpp:75-109), which is what its adjustment minimises: xd = f xp, r2 = xp^2 + yp^2,
    xu = xd + xd (k1 r2 + k2 r4) + (p1 (r2 + 2 xd^2) + 2 p2 xd yd), yu alike, residual = (xu, yu) - (observed - centre).
    Its tangential terms act on the pixel-scaled xd, yd: once p1, p2 leave zero it is not cv::projectPoints' model."""
    K, dist = got["camera"]
    f, cx, cy = K[0, 0], K[0, 2], K[1, 2]
    k1, k2, p1, p2 = dist[:4]
    point = np.repeat(np.arange(len(got["xyz"])), np.diff(got["origin_offsets"]))
    P = got["poses"][got["origin_shot"]]
    p = np.einsum("nij,nj->ni", P[:, :, :3], got["xyz"][point]) + P[:, :, 3]
    xp, yp = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    xd, yd = f * xp, f * yp
    r2 = xp * xp + yp * yp
    rad = k1 * r2 + k2 * r2 * r2
    xu = xd + xd * rad + (p1 * (r2 + 2.0 * (xd * xd)) + 2.0 * p2 * xd * yd)
    yu = yd + yd * rad + (2.0 * p1 * xd * yd + p2 * (r2 + 2.0 * (yd * yd)))
    return np.hypot(xu - (got["origin_xy"][:, 0] - cx), yu - (got["origin_xy"][:, 1] - cy))


@pytest.mark.parametrize("model", [ba.CAM_SIMPLE, ba.CAM_DISTORTION], ids=["Simple", "Distortion"])
def test_the_other_camera_models_fill_and_apply_their_intrinsics_block(model):
    """The intrinsics block of the Simple and the Distortion model (sfmx_ba.h: [f], [f, cx, cy, k1, k2, p1, p2]) and its
    write-back, pinned without a restatement of the mapping in the loop: a block filled or applied in the wrong order
    adjusts the wrong parameters (a centre of 360 px taken for a distortion coefficient, or the reverse, moves the
    projections by hundreds of pixels), and the mean residual of the returned scene under the returned camera leaves
    the bound.  The write-back's exact facts are checked beside it: f -> fx = fy; Simple touches nothing else;
    Distortion leaves k3.
    The bound (10 px, SFMX_MAX_REPROJECTION_ERROR): on this scene only the initial pair is recovered (below), so the
    returned scene is what the one adjustment left.  Before it, every point passed the triangulation's filter with both
    errors <= 10 px under cv::projectPoints, and with p1 = p2 = 0 the models' functors are that projection; LM never
    accepts a step that raises the cost, so the root mean square residual under the model's functor stays <= 10 px, and
    the mean is no larger than the root mean square.  Simple: the functor is the projection itself, so the figure is
    sfmx_reprojection_errors'.  Distortion: the figure is the reference's functor (functor_residuals); under
    cv::projectPoints the same scene measures 18.72 px, because the reference's Distortion functor is not that model
    once p1, p2 leave zero (adjusted here: f 398.8, centre (448.1, 204.4), k1 0.132, k2 -0.078, p1 3.5e-4, p2 8.8e-5):
    the reference's own adjustment and its own reprojection disagree in the same way.
    Distortion: the scene's camera has k1 = -0.05, k2 = 0.01.  Simple: the reference's SimpleCamera has no distortion
    (ICamera::getDistortion gives zeros), so its scene is projected without one.
    How many shots are recovered is not asserted beyond the initial pair.  Measured on MI355X, both models: the two-view
    adjustment after the initial pair has free intrinsics and nothing that fixes them (Simple: f from 864 to 2280 in 531
    iterations at a mean error of 0.164 px), and the three registrations that follow fall below min_pose_inlier_ratio
    (Simple: 0.42, 0.48, 0.21 < 0.5).  SimpleRadial's k1, k2 hold f on the same scene (scene 1)."""
    distorted = model != ba.CAM_SIMPLE
    sc = sfm_cases.scene(5, 300, noise=0.3, wrong=0.1, graph="complete", seed=11, distorted=distorted)
    ba.release_cache()
    got = sfm.triangulate(sc["keypoints"], sc["shot_size"], sfm_cases.camera(distorted), model, sc["pairs"], sc["matches"],
                          sc["offsets"], sc["homography"])
    e_cv = mean_reprojection_error(got)
    e = e_cv if model == ba.CAM_SIMPLE else float(np.mean(functor_residuals(got)))
    K, dist = got["camera"]
    print("\nmodel", model, "recovered", got["recovered"].tolist(), "points", len(got["xyz"]), "BA calls", got["summary"]["ba_calls"],
          "mean residual under the model's functor", e, "under projectPoints", e_cv, "f", K[0, 0], "centre", K[0, 2], K[1, 2],
          "dist", dist.tolist())
    assert got["summary"]["initial_pair"] >= 0 and got["recovered"].sum() >= 2 and got["summary"]["ba_calls"] >= 1
    assert len(got["xyz"]) > 100
    assert e < MAX_REPROJECTION_ERROR
    K0, d0 = sfm_cases.camera(distorted)
    assert K[0, 0] == K[1, 1]                                                   # f -> fx = fy
    assert K[0, 1] == 0 and K[1, 0] == 0 and np.array_equal(K[2], [0, 0, 1])
    if model == ba.CAM_SIMPLE:
        assert np.array_equal(K[:, 2], K0[:, 2]) and np.array_equal(dist, d0)   # only f is a parameter
    else:
        assert dist[4] == d0[4]                                                 # k3 is no parameter of the block
