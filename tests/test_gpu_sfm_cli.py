"""GPU: `Photogrammetrie ... --sfmx-reconstruct` on the three insel images with run-sequence-flann.sh's flag set:
the `reconstruction` object and the four scene files must equal what sfmx.sfm.triangulate plus the scene-output
writers give when called on the arrays the same run saved under features/ and matches/.  This is equality with the
library, whatever the images reconstruct to.  The same flag set without the flag writes exactly the files it
wrote before and no `reconstruction` key.  Fails without the feature: the flag is ignored."""
import json
import os

import numpy as np
import pytest

from sfmx import ba, cli, report, sfm
from test_gpu_cli import RUN_SCRIPTS, _argv   # the run-scripts' words with the insel directory (no test runs on import)

pytestmark = pytest.mark.gpu

FILES_BEFORE = {"shot_matches.csv", "sfmx_pipeline.json", "app.stat.csv", "features", "matches"}
SCENE_FILES = ["cameras_recovered.ply", "pointcloud_sparse.ply", "reprojectionerror.stat.csv", "reprojectionerror.hist.csv"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("sfm_cli")
    with_flag, without = base / "with" / "reconstruction", base / "without" / "reconstruction"
    assert "run-sequence-flann.sh" in RUN_SCRIPTS
    assert cli.main(_argv("run-sequence-flann.sh", "2", "", ["--sfmx-reconstruct"], with_flag)) == 0
    assert cli.main(_argv("run-sequence-flann.sh", "2", "", [], without)) == 0
    return with_flag, without


def library_result(out):
    s = json.load(open(out / "sfmx_pipeline.json"))
    paths, cfg = s["images"], s["config"]
    kps = []
    for i, p in enumerate(paths):
        k = np.load(out / "features" / f"{i}{os.path.basename(p)}.npz")["keypoints"]
        kps.append(np.stack([k["x"], k["y"]], 1))
    pairs = np.asarray(s["kept_pairs"], np.int32).reshape(-1, 2)
    lists = [np.load(out / "matches" / f"{j}{os.path.basename(paths[l])}-{os.path.basename(paths[r])}.npy")
             for j, (l, r) in enumerate(pairs)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    cam = s["camera"]
    K = np.array([[cam["focal_length"], 0, cam["cx"]], [0, cam["focal_length"], cam["cy"]], [0, 0, 1.0]])
    prm = sfm.default_params(min_match_count_for_baseline=cfg["baseline_homography_threshold"],
                             ransac_baseline_threshold=cfg["ransac_baseline_threshold"],
                             ransac_pose_threshold=cfg["ransac_pose_threshold"],
                             min_homography_inlier_ratio=cfg["homography_inlier_ratio_threshold"],
                             min_pose_inlier_ratio=cfg["pose_inlier_ratio_threshold"],
                             max_reprojection_error=cfg["reprojection_error_threshold"],
                             point_merge_distance=cfg["pointcloud_point_merge_distance"],
                             feature_merge_distance=cfg["pointcloud_feature_merge_distance"])
    ba.release_cache()
    r = sfm.triangulate(kps, [cam["resolution"]] * len(paths), (K, np.zeros(5)), cfg["camera_model"], pairs,
                        np.concatenate(lists), off, s["homography_inlier_ratios"], prm)
    return s, r, paths, cam["resolution"]


def test_reconstruction_equals_the_library_on_the_saved_arrays(runs, tmp_path):
    out, _ = runs
    s, r, paths, (w, h) = library_result(out)
    rec = s["reconstruction"]
    print("insel: recovered", rec["recovered_shots"], "points", rec["points"], "trace", [e[0] for e in rec["trace"]])
    assert rec["recovered_shots"] == np.flatnonzero(r["recovered"]).tolist()
    assert rec["points"] == len(r["xyz"]) and rec["records"] == len(r["origin_shot"])
    assert rec["pair_state"] == r["pair_state"].tolist() and rec["match_counts"] == np.diff(r["offsets"]).tolist()
    assert rec["trace"] == json.loads(json.dumps([list(e) for e in r["trace"]]))
    assert rec["summary"] == json.loads(json.dumps({k: v for k, v in r["summary"].items() if k != "step_wall_ms"}))
    assert rec["camera"]["K"] == r["camera"][0].reshape(-1).tolist() and rec["camera"]["distortion"] == r["camera"][1].tolist()
    # the four files from the library's result and the scene-output writers
    n = len(paths)
    poses = np.where(np.isnan(r["poses"]), 0.0, r["poses"])
    images = [cli.load_color(p, (w, h)) for p in paths]
    rgb = report.colorizePointcloud(len(r["xyz"]), r["origin_offsets"], r["origin_shot"], r["origin_xy"], images)
    report.writeToPLY(tmp_path / SCENE_FILES[0], cameras=[(w, h, r["camera"][0])],
                      shots=[(0, bool(r["recovered"][i]), poses[i]) for i in range(n)])
    report.writeToPLY(tmp_path / SCENE_FILES[1], r["xyz"], rgb)
    err = report.reprojection_errors(r["xyz"], r["origin_offsets"], r["origin_shot"], r["origin_xy"], [r["camera"]],
                                     np.zeros(n, np.int32), poses)
    report.writeToReprojectionErrorStatisticsCSV(err, tmp_path / SCENE_FILES[2])
    report.writeToReprojectionErrorHistogramCSV(err, tmp_path / SCENE_FILES[3])
    for name in SCENE_FILES:
        assert (out / name).read_bytes() == (tmp_path / name).read_bytes(), name
    assert "triangulate" in s["timings_ms"] and "reconstruction_timing" in s


def test_without_the_flag_the_run_is_the_one_before(runs):
    with_flag, without = runs
    assert set(os.listdir(without)) == FILES_BEFORE
    assert set(os.listdir(with_flag)) == FILES_BEFORE | set(SCENE_FILES)
    a, b = json.load(open(without / "sfmx_pipeline.json")), json.load(open(with_flag / "sfmx_pipeline.json"))
    assert "reconstruction" not in a and "reconstruction_timing" not in a
    same = set(a) - {"timings_ms", "config", "images"}
    assert same == set(b) - {"timings_ms", "config", "images", "reconstruction", "reconstruction_timing"}
    assert all(a[k] == b[k] for k in same)
    assert set(a["timings_ms"]) == {"extract_features", "match", "homography"}
    assert (without / "shot_matches.csv").read_bytes() == (with_flag / "shot_matches.csv").read_bytes()
    for sub in ("features", "matches"):
        assert sorted(os.listdir(without / sub)) == sorted(os.listdir(with_flag / sub))
        for f in os.listdir(without / sub):
            assert (without / sub / f).read_bytes() == (with_flag / sub / f).read_bytes(), f


def test_reconstruct_scene_composes_the_same_run(runs):
    """sfmx.sfm.reconstructScene (extract -> match -> homography -> triangulate) on the decoded images gives the
    reconstruction the command line wrote."""
    out, _ = runs
    s = json.load(open(out / "sfmx_pipeline.json"))
    cfg, cam = s["config"], s["camera"]
    images = [cli.load_gray(p, cam["resolution"]) for p in s["images"]]
    ba.release_cache()
    r = sfm.reconstructScene(images, cli.initial_camera(cam), cfg["camera_model"], pairs=s["pairs"], params=cli.sfm_params(
        type("Cfg", (), cfg)), match_threshold=cfg["match_threshold"], distinct_matches=bool(cfg["distinct_matches"]),
        ransac_matching_threshold=cfg["ransac_matching_threshold"])
    assert r["pairs"].tolist() == s["kept_pairs"] and [float(x) for x in r["homography_ratio"]] == s["homography_inlier_ratios"]
    assert json.loads(json.dumps(cli.reconstruction_object(r))) == s["reconstruction"]


def test_no_initial_pair_writes_the_empty_scene_and_exits_0(tmp_path):
    """-Phomography-inlier-ratio-threshold=1 drops every pair: the warning, the files of the empty scene, exit code 0."""
    out = tmp_path / "reconstruction"
    assert cli.main(_argv("run-sequence-flann.sh", "2", "", ["--sfmx-reconstruct", "-Phomography-inlier-ratio-threshold=1"], out)) == 0
    rec = json.load(open(out / "sfmx_pipeline.json"))["reconstruction"]
    assert rec["recovered_shots"] == [] and rec["points"] == 0 and rec["summary"]["ba_calls"] == 0
    assert [e[0] for e in rec["trace"]] == ["NO_CANDIDATE_PAIR", "NO_INITIAL_PAIR"]
    empty = tmp_path / "empty"
    empty.mkdir()
    report.writeToPLY(empty / "cloud.ply", np.zeros((0, 3)), np.zeros((0, 3), np.uint8))
    assert (out / "pointcloud_sparse.ply").read_bytes() == (empty / "cloud.ply").read_bytes()
    assert all((out / f).exists() for f in SCENE_FILES)
