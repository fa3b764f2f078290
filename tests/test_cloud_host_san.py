"""CPU: csrc/cloud_host.hpp under AddressSanitizer and UndefinedBehaviorSanitizer.

A stand-alone program (tests/cpp/cloud_host_main.cpp, its own main) includes the header, reads the PLY files of
tests/test_cloud_host.py (the malformed ones included: the reader takes files written by anyone) and writes the
three outputs for the golden mesh and for hand cases.  It runs as a child process, must exit clean, and its
outputs must equal the bytes of the numpy restatement.  The sanitizer runtimes are linked into the program, so it
needs nothing from the environment it is started in.  Fails without the feature: the header does not exist."""
import os
import subprocess

import numpy as np
import pytest

import cloud_cases
import cloud_ref
import fixtures

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cloud_host") / "cloud_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", os.path.join(REPO, "tests", "cpp", "cloud_host_main.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def test_reader_under_sanitizers(driver, tmp_path):
    good, bad = cloud_cases.good_files(str(tmp_path)), cloud_cases.bad_files(str(tmp_path))
    manifest = tmp_path / "manifest.txt"
    rows = [(p, str(tmp_path / f"out_{i}.bin")) for i, p in enumerate([g[1] for g in good] + [b[1] for b in bad])]
    manifest.write_text("".join(f"{a}\t{b}\n" for a, b in rows))
    r = subprocess.run([driver, "read", str(manifest)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
    codes = [int(v) for v in r.stdout.split()]
    assert codes == [0] * len(good) + [-1] * len(bad), list(zip([g[0] for g in good] + [b[0] for b in bad], codes))
    for (name, _, x, fs, fi), (_, out) in zip(good, rows):
        raw = open(out, "rb").read()
        n, f, k = np.frombuffer(raw[:24], np.int64)
        assert (n, f, k) == (len(x), len(fs), len(fi)), name
        exp = np.ascontiguousarray(x, np.float32).tobytes() + np.asarray(fs, np.int32).tobytes() + np.asarray(fi, np.int32).tobytes()
        assert raw[24:] == exp, name


def _write_case(driver, tmp_path, tag, x, d, fs, fi):
    d_in = tmp_path / f"{tag}.bin"
    out = tmp_path / tag
    out.mkdir()
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float64)
    fs, fi = np.asarray(fs, np.int32), np.asarray(fi, np.int32)
    with open(d_in, "wb") as f:
        np.array([len(x), len(d), len(fs), len(fi)], np.int64).tofile(f)
        for a in (x, d, fs, fi):
            a.tofile(f)
    r = subprocess.run([driver, "write", str(d_in), str(out)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and r.stderr == "", (tag, r.stdout + r.stderr)
    assert (out / "stats.csv").read_bytes() == cloud_ref.stats_csv(cloud_ref.statistics(d, len(x))), tag
    assert (out / "neighbors.csv").read_bytes() == cloud_ref.neighbors_csv(*cloud_ref.histogram(d)), tag
    assert (out / "quality.ply").read_bytes() == cloud_ref.quality_ply(x, d, fs, fi), tag
    assert (out / "quality_cut.ply").read_bytes() == cloud_ref.quality_ply(x, d, fs, fi, 0.2), tag


def test_writers_under_sanitizers(driver, tmp_path):
    g = fixtures.load("cloud_small")
    _write_case(driver, tmp_path, "golden", g["xyz"], g["distance"], g["face_sizes"], g["face_indices"])
    assert (tmp_path / "golden" / "quality.ply").read_bytes() == g["quality_ply"].tobytes()
    x = np.random.default_rng(5).normal(size=(6, 3))
    faces = ([3, 0, 4, 3], [0, 1, 2, 3, 2, 1, 0, 5, 6, -1])
    _write_case(driver, tmp_path, "zeros", x, np.zeros(6), *faces)                       # maxDistance == 0
    _write_case(driver, tmp_path, "equal", x, np.full(6, 0.125), *faces)                 # variance 0
    _write_case(driver, tmp_path, "inf", x, np.array([0, 1, np.inf, 2, 0.5, 0.5]), *faces)
    _write_case(driver, tmp_path, "empty", x[:1], np.zeros(0), [3], [0, 0, 0])           # n <= 1
    _write_case(driver, tmp_path, "nothing", np.zeros((0, 3)), np.zeros(0), [], [])
