"""CPU: the host layer of the point-cloud statistics (csrc/cloud_host.hpp behind the C ABI of
include/sfmx_cloud.h) equals the numpy restatement tests/cloud_ref.py: statistics and histogram as bit
patterns, the three files byte for byte, on the golden mesh (tests/golden/cloud_small.npz) and on hand cases;
the PLY reader round-trips what cloud_ref.write_ply writes and refuses every malformed file with SFMX_EINVAL.
Fails without the feature: sfmx.cloud does not exist."""
import os

import numpy as np
import pytest

import cloud_cases
import cloud_ref
import fixtures
from sfmx import _lib, cloud

FIELDS = ("n_points", "max", "min", "mean", "median", "variance", "deviation")


@pytest.fixture(scope="module")
def golden():
    return fixtures.load("cloud_small")


def same_stats(a, b):
    return all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() or (np.isnan(a[k]) and np.isnan(b[k])) for k in FIELDS)


def same_hist(a, b):
    (ka, ca), (kb, cb) = a, b
    return ka.dtype == np.float64 and ca.dtype == np.uint64 and np.array_equal(ka, kb, equal_nan=True) and \
        ka.tobytes()[:8 * int((~np.isnan(ka)).sum())] == kb.tobytes()[:8 * int((~np.isnan(kb)).sum())] and np.array_equal(ca, cb)


def test_restatement_reproduces_the_golden_fixture(golden):
    d, nb = cloud_ref.neighbor_distances(golden["xyz"])
    assert d.tobytes() == golden["distance"].tobytes() and np.array_equal(nb, golden["neighbor"])
    assert len(golden["xyz"]) == 600 and len(golden["face_sizes"]) == 200 and 256 in golden["face_sizes"]
    assert golden["face_indices"].max() >= 600 and (d == 0).sum() == 140


def test_statistics_and_histogram_equal_the_golden_fixture(golden):
    d = golden["distance"]
    s = cloud.statistics(d, 600)
    assert s["n_points"] == 600 and s["min"] == 0
    assert np.array([s[k] for k in FIELDS[1:]]).tobytes() == golden["stats"].tobytes()
    k, c = cloud.neighbor_histogram(d)
    assert k.tobytes() == golden["hist_key"].tobytes() and np.array_equal(c, golden["hist_count"])
    assert int(c.sum()) == 600 and np.all(np.diff(k) > 0)


def test_files_equal_the_golden_fixture(golden, tmp_path):
    d = golden["distance"]
    p = str(tmp_path / "out")
    cloud.write_stats_csv(p, cloud.statistics(d, 600))
    assert open(p, "rb").read() == golden["stats_csv"].tobytes()
    cloud.write_neighbors_csv(p, *cloud.neighbor_histogram(d))
    assert open(p, "rb").read() == golden["neighbors_csv"].tobytes()
    cloud.write_quality_ply(p, golden["xyz"], d, golden["face_sizes"], golden["face_indices"])
    got = open(p, "rb").read()
    assert got == golden["quality_ply"].tobytes()
    # 200 faces announced; the 256-vertex face and the face that leaves the cloud are not written
    head = got[:got.index(b"end_header\n")]
    assert b"element vertex 600\n" in head and b"element face 200\n" in head
    assert len(got) == len(head) + 11 + 600 * 19 + 150 * 20 + 40 * 24 + 8 * 28


HAND = {
    "empty": np.zeros(0),
    "one": np.array([0.75]),
    "two": np.array([0.5, 0.25]),
    "all_equal": np.full(9, 0.125),
    "all_zero": np.zeros(6),
    "odd": np.array([3.0, 0.0, 1e-20, 2.5, 0.1, 0.1, 7.0]),
    "even_with_inf": np.array([1.0, np.inf, 0.0, 2.0]),
    "many": np.abs(np.random.default_rng(8).normal(size=1001)) * 1e3,
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name, tmp_path):
    d = HAND[name]
    s, e = cloud.statistics(d, len(d) + 1), cloud_ref.statistics(d, len(d) + 1)
    assert same_stats(s, e), (s, e)
    if len(d):
        assert s["min"] == 0                                  # the reference starts min at 0
    else:
        assert [s[k] for k in FIELDS[1:]] == [0.0] * 6
    if name == "one":
        assert np.isnan(s["variance"])                        # 0 / 0: the reference divides by size - 1
    if name in ("all_equal", "all_zero"):
        assert s["variance"] == 0                             # so the automatic resolution is 0: key = distance
    for res in (-1.0, 0.0, 0.3, -0.0):
        assert same_hist(cloud.neighbor_histogram(d, res), cloud_ref.histogram(d, res)), res
    p = str(tmp_path / "f")
    cloud.write_stats_csv(p, s)
    assert open(p, "rb").read() == cloud_ref.stats_csv(e)
    k, c = cloud.neighbor_histogram(d)
    cloud.write_neighbors_csv(p, k, c)
    assert open(p, "rb").read() == cloud_ref.neighbors_csv(*cloud_ref.histogram(d))
    x = np.random.default_rng(5).normal(size=(len(d), 3)).astype(np.float32)
    n = len(d)
    fs = [3, 4, 0, 3] if n >= 4 else []
    fi = [0, 1, 2, 3, 2, 1, 0, 1, 1, n] if n >= 4 else []
    for cutoff in (-1.0, 0.2):
        cloud.write_quality_ply(p, x, d, fs, fi, cutoff)
        assert open(p, "rb").read() == cloud_ref.quality_ply(x, d, fs, fi, cutoff), cutoff


def test_quality_ply_of_a_cloud_without_distances(tmp_path):
    """n <= 1: the distance list is empty, the vertex block too; maxDistance == 0 writes r = b = 0."""
    p = str(tmp_path / "q.ply")
    cloud.write_quality_ply(p, np.array([[1, 2, 3]], np.float32), np.zeros(0), [3], [0, 0, 0])
    got = open(p, "rb").read()
    assert got == cloud_ref.quality_ply(np.zeros((1, 3)), np.zeros(0), [3], [0, 0, 0])
    assert b"element vertex 0\n" in got and b"element face 1\n" in got and got.endswith(b"end_header\n")
    x = np.zeros((3, 3), np.float32)
    cloud.write_quality_ply(p, x, np.zeros(3), [3], [0, 1, 2])
    got = open(p, "rb").read()
    assert got == cloud_ref.quality_ply(x, np.zeros(3), [3], [0, 1, 2])
    body = got[got.index(b"end_header\n") + 11:]
    assert body[12:15] == b"\0\0\0" and body[-7:-4] == b"\0\0\0"


def test_color_sums_wrap_like_the_reference_build():
    """Three vertices at ratio 1: b = 255, then (uchar)(255 + 255) = 254, then (uchar)(254 + 255) = 253."""
    x = np.zeros((3, 3), np.float32)
    got = cloud_ref.quality_ply(x, np.full(3, 2.0), [3], [0, 1, 2])
    assert got[-7:-4] == bytes([0, 0, 253 // 3])
    assert cloud_ref.to_u8(510.0) == 254 and cloud_ref.to_u8(float("nan")) == 0 and cloud_ref.to_u8(3e9) == 0


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cloud_ply"))
    return cloud_cases.good_files(d), cloud_cases.bad_files(d)


def test_ply_round_trips(files):
    good, _ = files
    assert len(good) == 13
    for name, path, x, fs, fi in good:
        p = cloud.read_ply(path)
        assert p["xyz"].dtype == np.float32 and p["xyz"].tobytes() == np.ascontiguousarray(x, np.float32).tobytes(), name
        assert p["face_sizes"].tolist() == list(fs) and p["face_indices"].tolist() == list(fi), name


def test_malformed_ply_is_einval(files):
    _, bad = files
    assert len(bad) >= 20
    n, f, k = (_lib.C.c_int64(0) for _ in range(3))
    for name, path in bad:
        rc = _lib.lib.sfmx_ply_read(os.fsencode(path), None, 0, _lib.C.byref(n), None, 0, _lib.C.byref(f), None, 0, _lib.C.byref(k))
        assert rc == _lib.SFMX_EINVAL, (name, rc)
        assert _lib.lib.sfmx_last_error(), name
        with pytest.raises(ValueError):
            cloud.read_ply(path)


def test_capacity_and_argument_errors(files, tmp_path):
    good, _ = files
    _, path, x, fs, fi = good[0]
    C = _lib.C
    n, f, k = (C.c_int64(0) for _ in range(3))
    buf = np.zeros((len(x) - 1, 3), np.float32)
    rc = _lib.lib.sfmx_ply_read(os.fsencode(path), buf.ctypes.data, len(buf), C.byref(n), None, 0, C.byref(f), None, 0, C.byref(k))
    assert rc == _lib.SFMX_ECAPACITY and (n.value, f.value, k.value) == (len(x), len(fs), len(fi))
    need = C.c_int64(0)
    d = np.array([0.5, 0.25, 0.5])
    assert _lib.lib.sfmx_cloud_histogram(d.ctypes.data, 3, 0.0, None, None, 0, C.byref(need)) == _lib.SFMX_ECAPACITY
    assert need.value == 2
    assert _lib.lib.sfmx_cloud_statistics(None, 3, 3, None) == _lib.SFMX_EINVAL
    assert _lib.lib.sfmx_cloud_write_stats_csv(None, None) == _lib.SFMX_EINVAL
    with pytest.raises(ValueError):
        cloud.write_stats_csv(str(tmp_path / "no_such_dir" / "s.csv"), cloud.statistics(d))
    with pytest.raises(ValueError):
        cloud.write_quality_ply(str(tmp_path / "q"), np.zeros((3, 3)), np.zeros(2))
