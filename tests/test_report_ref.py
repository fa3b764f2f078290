"""CPU: the numpy restatement of the scene outputs (tests/report_ref.py) against independent forms.

- The reprojection error against a plain float64 pinhole-plus-distortion projection.  For float-representable
  points the two differ only in the float rounding of u and v (and in a few ulps of fp64 from the order of the
  operations): |u - fl(u)| <= 2^-24 |u|, likewise v, and the norm is 1-Lipschitz in (du, dv) for the 1-norm, so
  |e - e64| <= 2^-24 (|u| + |v|) (1 + 2^-20); the factor covers the fp64 reassociation (about 2^-50 relative,
  against 2^-24).  Derived, not measured.
- The per-point colour reduction against the literal shot-major loop of Scene::colorizePointcloud.
- cvRound's round-half-to-even pixel positions.
Fails without the feature: tests/report_ref.py, tests/report_cases.py and the golden file do not exist."""
import numpy as np

import fixtures
import report_cases
import report_ref


def test_error_anchor_float64_projection():
    sc = report_cases.scene(np.random.default_rng(1).integers(0, 6, 400), 9, float_points=True)
    e = report_ref.reprojection_errors(*report_cases.args(sc))
    e64, uv = report_ref.reprojection_errors_f64(*report_cases.args(sc))
    assert len(e) > 800 and np.isfinite(e).all()
    bound = 2.0 ** -24 * uv * (1 + 2.0 ** -20)
    print("max |e - e64| / bound", float((np.abs(e - e64) / bound).max()))
    assert (np.abs(e - e64) <= bound).all()
    assert e.mean() > 0.3                                   # pixel noise of sigma 0.75: the errors are not all zero


def test_error_uses_the_float_point():
    """Coordinates that are no float32 values: the error is that of the rounded point."""
    sc = report_cases.scene([2] * 50, 4)
    assert (sc["xyz"].astype(np.float32).astype(np.float64) != sc["xyz"]).any()
    rounded = dict(sc, xyz=sc["xyz"].astype(np.float32).astype(np.float64))
    a = report_ref.reprojection_errors(*report_cases.args(sc))
    b = report_ref.reprojection_errors(*report_cases.args(rounded))
    assert a.tobytes() == b.tobytes()


def test_golden_is_the_restatement():
    g = fixtures.load("report_small")
    sc, ims, cams, shots = report_cases.from_golden(g)
    n = len(sc["xyz"])
    counts = np.diff(sc["origin_offsets"])
    assert n == 301 and counts.max() == 300 and counts[0] == 0 and counts[150] == 0 and counts[-1] == 0
    assert set(counts[counts < 300]) == set(range(8)) and set(sc["origin_shot"]) == set(range(5))
    err = report_ref.reprojection_errors(*report_cases.args(sc))
    assert err.tobytes() == g["err"].tobytes()
    rgb, rec = report_ref.colorize(n, sc["origin_offsets"], sc["origin_shot"], sc["origin_xy"], ims)
    assert np.array_equal(rgb, g["rgb"]) and np.array_equal(rec, g["record"])
    assert (rgb.any(axis=1)).sum() > 100 and (rec < 0).sum() >= 6
    assert report_ref.cameras_ply(cams, shots) == g["cameras_ply"].tobytes()
    assert report_ref.pointcloud_ply(sc["xyz"], rgb) == g["cloud_ply"].tobytes()


def test_colour_reduction_is_the_literal_loop():
    rng = np.random.default_rng(12)
    ims = report_cases.images(5)
    for trial in range(6):
        n = 60
        counts = rng.integers(0, 6, n)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        osh = rng.integers(0, 5, off[-1]).astype(np.int32)
        oxy = rng.uniform(-3, 45, (off[-1], 2))
        oxy[rng.random(off[-1]) < 0.05] = np.nan
        a = report_ref.colorize_literal(n, off, osh, oxy, ims, (1, 2, 3))
        b = report_ref.colorize(n, off, osh, oxy, ims, (1, 2, 3))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), trial
    n, off, osh, oxy, ims3 = report_cases.colour_case()
    a = report_ref.colorize_literal(n, off, osh, oxy, ims3, (9, 8, 7))
    b = report_ref.colorize(n, off, osh, oxy, ims3, (9, 8, 7))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert b[1][12] == off[12] + 3 and b[1][13] == off[13]          # the lowest shot late and twice: its first record
    assert b[1][9] == off[9] and tuple(b[0][9]) == (9, 8, 7)        # NaN: the record is named, the colour the default
    assert b[1][11] == -1 and tuple(b[0][11]) == (9, 8, 7)


def test_round_half_even_positions():
    assert report_ref.pixel_position(2.5, 3.5) == (2, 4)
    assert report_ref.pixel_position(-0.5, 0.5) == (0, 0)
    assert report_ref.pixel_position(-0.4, -0.6) == (0, -1)
    assert report_ref.pixel_position(63.5, 36.5) == (64, 36)
    assert report_ref.pixel_position(float("nan"), 1.0) is None and report_ref.pixel_position(1.0, float("inf")) is None
    n, off, osh, oxy, ims = report_cases.colour_case()
    rgb, rec = report_ref.colorize(n, off, osh, oxy, ims, (9, 8, 7))
    px = lambda s, x, y: tuple(int(v) for v in ims[s][y, x][::-1])
    assert tuple(rgb[0]) == px(0, 2, 4) and tuple(rgb[1]) == px(0, 4, 2)
    assert tuple(rgb[2]) == px(0, 0, 0) and tuple(rgb[3]) == px(0, 0, 5) and tuple(rgb[4]) == (9, 8, 7)
    assert tuple(rgb[5]) == (9, 8, 7) and tuple(rgb[6]) == px(1, 36, 1)
    assert tuple(rgb[7]) == (9, 8, 7) and tuple(rgb[8]) == px(1, 5, 28)
    assert tuple(rgb[14]) == (9, 8, 7) and tuple(rgb[15]) == px(2, 4, 3)
    assert tuple(rgb[16]) == (9, 8, 7) and tuple(rgb[17]) == (9, 8, 7)


def test_statistics_with_nan_and_inf():
    s = report_ref.error_statistics([2.0, np.nan, 1.0, 3.0])
    assert s["n_points"] == 4 and s["max"] == 3.0 and s["min"] == 0.0 and np.isnan(s["mean"]) and np.isnan(s["variance"])
    assert s["median"] == 2.5                                        # sorted: 1 2 3 NaN
    k, c = report_ref.error_histogram([2.0, np.nan, 1.0, 3.0])
    assert len(k) == 1 and np.isnan(k[0]) and c[0] == 4
    z = report_ref.error_statistics([])
    assert report_ref.stats_csv(z).endswith(b"\n0,0.000000,0.000000,0.000000,0.000000,0.000000,0.000000\n")
    one = report_ref.stats_csv(report_ref.error_statistics([1.5]))
    assert one.endswith(b"\n1,1.500000,0.000000,1.500000,1.500000,-nan,-nan\n")   # 0.0 / 0.0 as glibc prints it
