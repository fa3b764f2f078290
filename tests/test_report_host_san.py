"""CPU: csrc/report_host.hpp (and the statistics of csrc/cloud_host.hpp it rests on) under AddressSanitizer and
UndefinedBehaviorSanitizer.

A stand-alone program (tests/cpp/report_host_main.cpp, its own main) includes the header and writes the two CSVs,
the cloud PLY, the camera PLY and the host colour gather for the golden scene and for hand cases.  It runs as a
child process, must exit clean with nothing on stderr, and its outputs must equal the bytes of the numpy
restatement.  The sanitizer runtimes are linked into the program, so it needs nothing from the environment it is
started in.  Fails without the feature: the header does not exist."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import report_cases
import report_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("report_host") / "report_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", os.path.join(REPO, "tests", "cpp", "report_host_main.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def _run(driver, tmp_path, tag, errors, xyz, rgb, cams, shots, color=None, only_recovered=True, colour=None, cameras_fail=False):
    """colour: (n_points, offsets, shots, positions, images): the host gather over the restatement's records."""
    src = tmp_path / f"{tag}.bin"
    out = tmp_path / tag
    out.mkdir()
    e = np.ascontiguousarray(errors, np.float64)
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    n = len(x)
    ims = colour[4] if colour else []
    with open(src, "wb") as f:
        np.array([len(e), n, rgb is not None, len(cams), len(shots), only_recovered, color is not None, len(ims)], np.int64).tofile(f)
        e.tofile(f)
        x.tofile(f)
        if rgb is not None:
            np.ascontiguousarray(rgb, np.uint8).tofile(f)
        for w, h, K in cams:
            K = np.asarray(K, np.float64).reshape(9)
            np.array([w, h, K[0], K[4], K[2], K[5]], np.float64).tofile(f)
        for c, r, pose in shots:
            np.concatenate([[c, r], np.asarray(pose, np.float64).reshape(12)]).astype(np.float64).tofile(f)
        if color is not None:
            np.array(color, np.uint8).tofile(f)
        if colour:
            _, off, osh, oxy, _ = colour
            assert colour[0] == n
            _, rec = report_ref.colorize(n, off, osh, oxy, ims, (9, 8, 7))
            pos = [report_ref.pixel_position(*oxy[r]) if r >= 0 else None for r in rec]
            clamp = lambda v: int(max(-2 ** 31, min(2 ** 31 - 1, v)))   # what the device's saturating conversion hands over
            np.array([len(osh)], np.int64).tofile(f)
            np.ascontiguousarray(osh, np.int32).tofile(f)
            rec.astype(np.int64).tofile(f)
            np.array([clamp(p[0]) if p else -1 for p in pos], np.int32).tofile(f)
            np.array([clamp(p[1]) if p else -1 for p in pos], np.int32).tofile(f)
            for im in ims:
                h, w = im.shape[:2]
                np.array([w, h, im.strides[0]], np.int64).tofile(f)
                np.lib.stride_tricks.as_strided(im, (h, im.strides[0]), (im.strides[0], 1)).tofile(f)
    r = subprocess.run([driver, "write", str(src), str(out)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and r.stderr == "", (tag, r.stdout + r.stderr)
    assert (out / "stats.csv").read_bytes() == report_ref.stats_csv(report_ref.error_statistics(e)), tag
    assert (out / "hist.csv").read_bytes() == report_ref.hist_csv(*report_ref.error_histogram(e)), tag
    assert (out / "cloud.ply").read_bytes() == report_ref.pointcloud_ply(x, rgb), tag
    if cameras_fail:
        assert (out / "cameras.rc").read_bytes() == b"-1" and not (out / "cameras.ply").exists(), tag
    else:
        assert (out / "cameras.ply").read_bytes() == report_ref.cameras_ply(cams, shots, color, only_recovered), tag
    if colour:
        exp, _ = report_ref.colorize(n, colour[1], colour[2], colour[3], ims, (9, 8, 7))
        assert (out / "colors.bin").read_bytes() == exp.tobytes(), tag
    return out


def test_golden_under_sanitizers(driver, tmp_path):
    g = fixtures.load("report_small")
    sc, ims, cams, shots = report_cases.from_golden(g)
    colour = (len(sc["xyz"]), sc["origin_offsets"], sc["origin_shot"], sc["origin_xy"], ims)
    out = _run(driver, tmp_path, "golden", g["err"], sc["xyz"], g["rgb"], cams, shots, colour=colour)
    for name, key in (("stats.csv", "stats_csv"), ("hist.csv", "hist_csv"), ("cloud.ply", "cloud_ply"), ("cameras.ply", "cameras_ply")):
        assert (out / name).read_bytes() == g[key].tobytes(), name
    assert (out / "colors.bin").read_bytes() != bytes(3 * len(sc["xyz"]))


def test_hand_cases_under_sanitizers(driver, tmp_path):
    sc = report_cases.golden_scene()
    cams = report_cases.mvs_cameras(sc)
    shots = report_cases.mvs_shots(sc, [True, False, True, True, False])
    x = np.array([[0.1, -0.0, 1e300], [np.nan, -np.inf, 1e-50], [1 + 2.0 ** -30, 3.0, -7.25]])
    none = np.zeros((0, 3))
    _run(driver, tmp_path, "nothing", [], none, None, cams, [])
    _run(driver, tmp_path, "one", [1.5], x, None, cams, shots, only_recovered=False)
    _run(driver, tmp_path, "equal", [0.25] * 7, x, [[1, 2, 3], [255, 0, 254], [9, 9, 9]], cams, shots, color=(1, 200, 30))
    _run(driver, tmp_path, "nan_inf", [2.0, np.nan, 1.0, np.inf, 3.0], none, None, [], [])
    _run(driver, tmp_path, "all_nan", [np.nan] * 3, none, None, cams, [(-1, False, np.zeros(12)), (1, True, sc["shot_pose"][0])])
    _run(driver, tmp_path, "no_camera", [1.0, 2.0], none, None, cams, [(2, True, np.zeros(12))], cameras_fail=True)
    n = report_cases.colour_case()[0]
    _run(driver, tmp_path, "colour", [], np.zeros((n, 3)), None, [], [], colour=report_cases.colour_case())
