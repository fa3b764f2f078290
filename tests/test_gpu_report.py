"""GPU parity for the scene outputs (include/sfmx_report.h): the reprojection-error kernel and the colour kernel
of csrc/report.hip through sfmx.report against the numpy restatement tests/report_ref.py.  Errors are compared as
uint64 bit patterns (every step is one correctly rounded operation on both sides), colours and records exactly,
the files byte for byte against tests/golden/report_small.npz."""
import numpy as np
import pytest
import torch

from sfmx import report
import fixtures
import report_cases
import report_ref

pytestmark = pytest.mark.gpu

BLOCK = 256   # csrc/report.hip: one thread per record, no stride loop

_CACHE = {}


def golden():
    if "golden" not in _CACHE:
        g = fixtures.load("report_small")
        for v in g.values():
            v.setflags(write=False)
        _CACHE["golden"] = (g,) + report_cases.from_golden(g)
    return _CACHE["golden"]


def on_device(sc):
    t = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()
    return (t(sc["xyz"], np.float64), t(sc["origin_offsets"], np.int64), t(sc["origin_shot"], np.int32),
            t(sc["origin_xy"], np.float64), sc["cameras"], sc["shot_camera"], sc["shot_pose"])


def same_bits(got, exp):
    assert got.dtype == np.float64 and got.shape == exp.shape
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])


def test_errors_golden_host_and_device():
    g, sc, _, _, _ = golden()
    assert (sc["xyz"].astype(np.float32).astype(np.float64) != sc["xyz"]).any()   # not float-representable
    e = report.reprojection_errors(*report_cases.args(sc))
    same_bits(e, g["err"])
    assert report.reprojection_last_kernel_ms() > 0
    d = report.reprojection_errors_device(*on_device(sc))
    assert d.is_cuda and d.dtype == torch.float64
    same_bits(d.cpu().numpy(), g["err"])                                          # device inputs == host inputs, bit for bit


def test_errors_degenerate_values():
    sc = report_cases.degenerate_scene()
    exp = report_ref.reprojection_errors(*report_cases.args(sc))
    nan = np.float64(np.nan).view(np.uint64)
    # on the camera plane: z = 1, the point projects as (0.5, 0.25); NaN / inf coordinates and a NaN position: NaN
    assert np.isfinite(exp[0]) and np.isfinite(exp[6]) and all(exp[i:i + 1].view(np.uint64)[0] == nan for i in (1, 2, 5))
    same_bits(report.reprojection_errors(*report_cases.args(sc)), exp)
    same_bits(report.reprojection_errors_device(*on_device(sc)).cpu().numpy(), exp)


@pytest.mark.parametrize("n_origins", [63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_errors_sizes(n_origins):
    sc = report_cases.sized_scene(n_origins)
    assert len(sc["origin_shot"]) == n_origins
    exp = report_ref.reprojection_errors(*report_cases.args(sc))
    same_bits(report.reprojection_errors(*report_cases.args(sc)), exp)
    same_bits(report.reprojection_errors_device(*on_device(sc)).cpu().numpy(), exp)


def test_errors_empty():
    sc = report_cases.scene([0, 0, 0], 1)
    report.reprojection_errors(*report_cases.args(report_cases.sized_scene(5)))    # a call that launched
    e = report.reprojection_errors(*report_cases.args(sc))
    assert e.shape == (0,) and report.reprojection_last_kernel_ms() == 0.0
    d = report.reprojection_errors_device(*on_device(sc))
    assert d.shape == (0,) and report.reprojection_last_kernel_ms() == 0.0


def test_errors_invalid_inputs():
    sc = report_cases.sized_scene(100)
    bad = dict(sc, origin_shot=sc["origin_shot"].copy())
    bad["origin_shot"][70] = 5                                                     # outside [0, n_shots)
    with pytest.raises(ValueError):
        report.reprojection_errors(*report_cases.args(bad))
    with pytest.raises(ValueError):
        report.reprojection_errors_device(*on_device(bad))                         # checked in the kernel
    bad["origin_shot"][70] = -1
    with pytest.raises(ValueError):
        report.reprojection_errors_device(*on_device(bad))
    K = sc["cameras"][1][0].copy()
    K[1, 1] = 0.0
    with pytest.raises(ValueError):
        report.reprojection_errors(*report_cases.args(dict(sc, cameras=[sc["cameras"][0], (K, sc["cameras"][1][1])])))
    off = sc["origin_offsets"].copy()
    off[10] = off[11] + 1                                                          # does not ascend
    with pytest.raises(ValueError):
        report.reprojection_errors(*report_cases.args(dict(sc, origin_offsets=off)))
    short = sc["origin_offsets"].copy()
    short[-1] -= 1                                                                 # the last record lies in no row
    with pytest.raises(ValueError):
        report.reprojection_errors_device(*on_device(dict(sc, origin_offsets=short)))
    same_bits(report.reprojection_errors(*report_cases.args(sc)), report_ref.reprojection_errors(*report_cases.args(sc)))


def _colour_both(n, off, osh, oxy, ims, default):
    exp_rgb, exp_rec = report_ref.colorize(n, off, osh, oxy, ims, default)
    rgb, rec = report.colorize_pointcloud(n, off, osh, oxy, ims, default)
    assert rgb.dtype == np.uint8 and rec.dtype == np.int64
    assert np.array_equal(rec, exp_rec), (rec, exp_rec)
    assert np.array_equal(rgb, exp_rgb), np.flatnonzero((rgb != exp_rgb).any(axis=1))
    t = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()
    dims = []
    for im in ims:                                                                 # device images with padded rows
        h, w = im.shape[:2]
        buf = torch.full((h, 3 * w + 5), 0xEE, dtype=torch.uint8, device="cuda")
        buf[:, :3 * w] = torch.from_numpy(np.ascontiguousarray(im).reshape(h, 3 * w)).cuda()
        dims.append(buf.as_strided((h, w, 3), (3 * w + 5, 3, 1)))
    drgb, drec = report.colorize_pointcloud_device(n, t(off, np.int64), t(osh, np.int32), t(oxy, np.float64), dims, default)
    assert drgb.cpu().numpy().tobytes() == rgb.tobytes() and np.array_equal(drec.cpu().numpy(), rec)   # equal bytes in both modes
    return rgb, rec


def test_colour_hand_case():
    n, off, osh, oxy, ims = report_cases.colour_case()
    assert [im.shape[:2] for im in ims] == [(48, 64), (29, 37), (4, 5)] and all(im.strides[0] > 3 * im.shape[1] for im in ims)
    rgb, rec = _colour_both(n, off, osh, oxy, ims, (9, 8, 7))
    assert report.colorize_last_kernel_ms() > 0
    assert rec[11] == -1 and rec[9] == off[9] and rec[12] == off[12] + 3 and tuple(rgb[9]) == (9, 8, 7)
    assert len({tuple(int(v) for v in c) for c in rgb}) == 10                       # nine distinct pixels and the default


def test_colour_golden_and_default():
    g, sc, ims, _, _ = golden()
    n = len(sc["xyz"])
    rgb, rec = _colour_both(n, sc["origin_offsets"], sc["origin_shot"], sc["origin_xy"], ims, (0, 0, 0))
    assert np.array_equal(rgb, g["rgb"]) and np.array_equal(rec, g["record"])
    assert np.array_equal(report.colorizePointcloud(n, sc["origin_offsets"], sc["origin_shot"], sc["origin_xy"], ims), g["rgb"])


def test_colour_invalid_inputs():
    n, off, osh, oxy, ims = report_cases.colour_case()
    t = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()
    dims = [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in ims]
    bad = osh.copy()
    bad[3] = 3
    with pytest.raises(ValueError):
        report.colorize_pointcloud(n, off, bad, oxy, ims)
    with pytest.raises(ValueError):
        report.colorize_pointcloud_device(n, t(off, np.int64), t(bad, np.int32), t(oxy, np.float64), dims)
    boff = off.copy()
    boff[-1] += 4                                                                  # a row past the record arrays
    with pytest.raises(ValueError):
        report.colorize_pointcloud_device(n, t(boff, np.int64), t(osh, np.int32), t(oxy, np.float64), dims)


def test_end_to_end_files(tmp_path):
    """errors -> statistics -> histogram -> the two CSVs, colours -> the sparse PLY, the cameras: the golden bytes."""
    g, sc, ims, cams, shots = golden()
    n = len(sc["xyz"])
    e = report.reprojection_errors_device(*on_device(sc))
    report.writeToReprojectionErrorStatisticsCSV(e, tmp_path / "reprojectionerror.stat.csv")
    report.writeToReprojectionErrorHistogramCSV(e, tmp_path / "reprojectionerror.hist.csv")
    rgb = report.colorizePointcloud(n, sc["origin_offsets"], sc["origin_shot"], sc["origin_xy"], ims)
    report.writeToPLY(tmp_path / "pointcloud_sparse.ply", sc["xyz"], rgb)
    report.writeToPLY(tmp_path / "cameras_recovered.ply", cameras=cams, shots=shots)
    assert (tmp_path / "reprojectionerror.stat.csv").read_bytes() == g["stats_csv"].tobytes()
    assert (tmp_path / "reprojectionerror.hist.csv").read_bytes() == g["hist_csv"].tobytes()
    assert (tmp_path / "pointcloud_sparse.ply").read_bytes() == g["cloud_ply"].tobytes()
    assert (tmp_path / "cameras_recovered.ply").read_bytes() == g["cameras_ply"].tobytes()
