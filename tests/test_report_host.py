"""CPU: the host-only entry points of include/sfmx_report.h (the two reprojection-error CSVs, the cloud PLY, the
camera PLY) through sfmx.report, byte for byte against the numpy restatement tests/report_ref.py, on the golden
scene and on hand cases.  The CSV numbers come from sfmx_cloud_statistics / sfmx_cloud_histogram, which must
order NaN errors behind the others.  Fails without the feature: sfmx.report and the symbols do not exist."""
import numpy as np
import pytest

import sfmx
from sfmx import report
import fixtures
import report_cases
import report_ref


def _csvs(tmp_path, tag, errors):
    e = np.asarray(errors, np.float64)
    a, b = tmp_path / f"{tag}.stat.csv", tmp_path / f"{tag}.hist.csv"
    report.writeToReprojectionErrorStatisticsCSV(e, a)
    report.writeToReprojectionErrorHistogramCSV(e, b)
    exp_s = report_ref.stats_csv(report_ref.error_statistics(e))
    exp_h = report_ref.hist_csv(*report_ref.error_histogram(e))
    assert a.read_bytes() == exp_s, (tag, a.read_bytes(), exp_s)
    assert b.read_bytes() == exp_h, (tag, b.read_bytes()[:200], exp_h[:200])
    return a.read_bytes(), b.read_bytes()


def test_golden_files(tmp_path):
    g = fixtures.load("report_small")
    sc, ims, cams, shots = report_cases.from_golden(g)
    s, h = _csvs(tmp_path, "golden", g["err"])
    assert s == g["stats_csv"].tobytes() and h == g["hist_csv"].tobytes()
    assert s.startswith(b"N_Points,Max_Error,Min_Error,Avg_Error,Median_Error,Variance_Error,Deviation_Error\n%d," % len(g["err"]))
    assert h.startswith(b"Error,Count\n") and h.count(b"\n") > 10
    p = tmp_path / "cloud.ply"
    report.writeToPLY(p, sc["xyz"], g["rgb"])
    assert p.read_bytes() == g["cloud_ply"].tobytes()
    assert len(p.read_bytes()) == p.read_bytes().index(b"end_header\n") + 11 + 15 * len(sc["xyz"])
    report.writeToPLY(p, sc["xyz"])                                   # NULL colours: cv::Scalar(0, 0, 0, 255)
    assert p.read_bytes() == g["cloud_plain_ply"].tobytes() == report_ref.pointcloud_ply(sc["xyz"])
    c = tmp_path / "cameras.ply"
    report.writeToPLY(c, cameras=cams, shots=shots)
    assert c.read_bytes() == g["cameras_ply"].tobytes()
    assert b"element vertex %d\n" % (5 * 4 + 4) in c.read_bytes() and b"element edge %d\n" % (8 * 4 + 3) in c.read_bytes()


@pytest.mark.parametrize("tag,errors", [
    ("none", []), ("one", [1.5]), ("equal", [0.25] * 7), ("nan_inf", [2.0, np.nan, 1.0, np.inf, 3.0]),
    ("nan", [2.0, np.nan, 1.0, 3.0]), ("all_nan", [np.nan, np.nan]), ("inf", [0.5, np.inf]), ("two", [1.0, 4.0]),
])
def test_csv_hand_cases(tmp_path, tag, errors):
    s, h = _csvs(tmp_path, tag, errors)
    if tag == "none":
        assert s.endswith(b"\n0,0.000000,0.000000,0.000000,0.000000,0.000000,0.000000\n") and h == b"Error,Count\n"
    if tag == "one":                                                  # no `size > 1` guard: 0.0 / 0.0
        assert s.endswith(b"\n1,1.500000,0.000000,1.500000,1.500000,-nan,-nan\n") and h == b"Error,Count\nnan,1\n"
    if tag == "equal":
        assert h == b"Error,Count\n0.250000,7\n"


def test_statistics_order_nan_behind():
    s = sfmx.cloud.statistics([2.0, np.nan, 1.0, 3.0])
    assert s["max"] == 3.0 and s["min"] == 0.0 and s["median"] == 2.5 and np.isnan(s["mean"])
    assert sfmx.cloud.statistics([3.0, 1.0, 2.0]) == dict(n_points=3, max=3.0, min=0.0, mean=2.0, median=2.0, variance=1.0,
                                                          deviation=1.0)


def _cameras(tmp_path, cams, shots, **kw):
    p = tmp_path / "c.ply"
    report.write_cameras_ply(p, cams, shots, **kw)
    ref_kw = dict(color=kw.get("color"), only_recovered=kw.get("only_recovered", True))
    exp = report_ref.cameras_ply(cams, shots, **ref_kw)
    assert p.read_bytes() == exp, (p.read_bytes()[-300:], exp[-300:])
    return p.read_bytes()


def test_camera_ply_hand_cases(tmp_path):
    sc = report_cases.golden_scene()
    cams = report_cases.mvs_cameras(sc)                               # a landscape and a portrait camera
    assert cams[0][0] > cams[0][1] and cams[1][0] < cams[1][1]
    empty = _cameras(tmp_path, cams, [])                              # 0 shots: the coordinate system alone
    assert b"element vertex 4\n" in empty and b"element edge 3\n" in empty
    assert empty.endswith(b"end_header\n0 0 0 0 0 0\n1 0 0 255 0 0\n0 1 0 0 255 0\n0 0 1 0 0 255\n0 1 255 0 0\n0 2 0 255 0\n0 3 0 0 255\n")
    shots = report_cases.mvs_shots(sc, [True, False, True, True, False])
    kept = _cameras(tmp_path, cams, shots, only_recovered=True)
    all_ = _cameras(tmp_path, cams, shots, only_recovered=False)
    assert b"element vertex 19\n" in kept and b"element vertex 29\n" in all_ and b"element edge 43\n" in all_
    assert b" 255 255 0\n" in kept
    col = _cameras(tmp_path, cams, shots, color=(1, 200, 30))
    assert b" 1 200 30\n" in col and b" 255 255 0\n" not in col
    one = _cameras(tmp_path, [(4, 2, np.array([[2.0, 0, 1.0], [0, 4.0, 0.5], [0, 0, 1]]))],
                   [(0, True, np.hstack([np.eye(3), [[1.0], [2.0], [3.0]]]))])
    # norm 1/4: f = 3 / 4, corners (-0.25 | 0.75, -0.125 | 0.375), moved by (1, 2, 3)
    assert b"\n1.000000 2.000000 3.000000 255 255 0\n0.750000 1.875000 3.750000 255 255 0\n1.750000 1.875000 3.750000 255 255 0\n" \
           b"0.750000 2.375000 3.750000 255 255 0\n1.750000 2.375000 3.750000 255 255 0\n4 5 255 255 0\n" in one
    # a recovered shot without a camera is refused; an unrecovered one is not looked at
    with pytest.raises(ValueError):
        report.write_cameras_ply(tmp_path / "x.ply", cams, [(-1, True, np.zeros(12))])
    with pytest.raises(ValueError):
        report.write_cameras_ply(tmp_path / "x.ply", cams, [(2, False, np.zeros(12))], only_recovered=False)
    _cameras(tmp_path, cams, [(-1, False, np.zeros(12)), (1, True, sc["shot_pose"][0])])


def test_cloud_ply_hand_cases(tmp_path):
    p = tmp_path / "p.ply"
    report.write_pointcloud_ply(p, np.zeros((0, 3)))
    assert p.read_bytes() == report_ref.pointcloud_ply(np.zeros((0, 3))) and p.read_bytes().endswith(b"end_header\n")
    x = np.array([[0.1, -0.0, 1e300], [np.nan, -np.inf, 1e-50], [1 + 2.0 ** -30, 3.0, -7.25]])
    rgb = np.array([[1, 2, 3], [255, 0, 254], [9, 9, 9]], np.uint8)
    report.write_pointcloud_ply(p, x, rgb)
    assert p.read_bytes() == report_ref.pointcloud_ply(x, rgb)
    assert p.read_bytes()[-15:] == np.array([1, 3, -7.25], "<f4").tobytes() + b"\x09\x09\x09"
    with pytest.raises(ValueError):
        report.write_pointcloud_ply(p, x, rgb[:2])
    with pytest.raises(ValueError):
        report.write_pointcloud_ply(tmp_path / "no_such_dir" / "p.ply", x)


def test_empty_calls_need_no_device():
    """n_origins == 0 and n_points == 0 launch nothing: they return without a GPU."""
    sc = report_cases.scene([0, 0, 0], 1)
    e = report.reprojection_errors(*report_cases.args(sc))
    assert e.shape == (0,) and e.dtype == np.float64 and report.reprojection_last_kernel_ms() == 0.0
    rgb, rec = report.colorize_pointcloud(0, [0], [], np.zeros((0, 2)), report_cases.images(3))
    assert rgb.shape == (0, 3) and rec.shape == (0,) and report.colorize_last_kernel_ms() == 0.0


def test_host_validation_precedes_the_device():
    sc = report_cases.scene([2, 0, 3], 2)
    a = list(report_cases.args(sc))
    bad_shot = list(a)
    bad_shot[2] = np.array([0, 5, 1, 2, 3], np.int32)
    desc = list(a)
    desc[1] = np.array([0, 3, 2, 5], np.int64)
    zero_f = list(a)
    K = sc["cameras"][0][0].copy()
    K[0, 0] = 0.0
    zero_f[4] = [(K, sc["cameras"][0][1]), sc["cameras"][1]]
    short = list(a)
    short[1] = np.array([0, 2, 2, 4], np.int64)
    for bad in (bad_shot, desc, zero_f, short):
        with pytest.raises(ValueError):
            report.reprojection_errors(*bad)
    ims = report_cases.images(5)
    with pytest.raises(ValueError):
        report.colorize_pointcloud(3, desc[1], a[2], a[3], ims)
    with pytest.raises(ValueError):
        report.colorize_pointcloud(3, a[1], bad_shot[2], a[3], ims)
    with pytest.raises(ValueError):
        report.colorize_pointcloud(3, a[1], np.array([0, 4, 1, 2, 3], np.int32), a[3], ims[:3])   # shot 4 has no image
